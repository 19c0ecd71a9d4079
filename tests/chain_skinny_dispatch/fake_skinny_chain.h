// fake_skinny_chain.h - TEST INFRASTRUCTURE for tests/test_chain_skinny_dispatch.py, never part of the product library: what the stand-in of
// launch_bf16_skinny_chain (fake_skinny_chain.cpp) records, and its knobs. tests/chain_dispatch/fake_chain.cpp, compiled unchanged, supplies
// the HIP host entry points, the single calls and the other chain launchers.
#pragma once
#include "../../tpp-mlir_amd/csrc/xsmm_desc.h"
#include "../../tpp-mlir_amd/csrc/chain_args.h"

struct FakeSkinnyLaunch {
  int b_kind, bn;   // the launcher's arguments
  tpp::ChainArgs a; // the argument block as the launcher received it
  int starved;      // the stand-in wrote the error word and stored nothing
};

extern "C" {
int fake_skinny_launches(void);
const FakeSkinnyLaunch *fake_skinny_launch(int i);
void fake_skinny_clear(void);
void fake_skinny_starve(int nth, int layer); // the nth launch from now (1 = the next) writes 1 + layer into its error word and stores nothing
int fake_skinny_counter_mismatches(void);    // seams whose counter did not hold target - G before the launch, or lay outside its block
}
