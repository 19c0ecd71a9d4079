// fake_skinny_f32_chain.h - TEST INFRASTRUCTURE for tests/test_chain_skinny_f32_dispatch.py, never part of the product library: what the stand-in
// of launch_f32_skinny_chain (fake_skinny_f32_chain.cpp) records, and its knobs. tests/chain_dispatch/fake_chain.cpp, compiled unchanged,
// supplies the HIP host entry points, the single calls and the other chain launchers; tests/chain_skinny_dispatch/fake_skinny_chain.cpp,
// compiled unchanged, the bf16 skinny chain's stand-in.
#pragma once
#include "../../tpp-mlir_amd/csrc/xsmm_desc.h"
#include "../../tpp-mlir_amd/csrc/chain_args.h"

struct FakeSkinnyF32Launch {
  int bn;           // the launcher's argument
  int waves;        // the waves the real launcher would give the workgroups: the deepest layer's (brgemm_f32_skinny_chain.h skfc_layer_waves)
  tpp::ChainArgs a; // the argument block as the launcher received it
  int starved;      // the stand-in wrote the error word and stored nothing
};

extern "C" {
int fake_skinny_f32_launches(void);
const FakeSkinnyF32Launch *fake_skinny_f32_launch(int i);
void fake_skinny_f32_clear(void);
void fake_skinny_f32_starve(int nth, int layer); // the nth launch from now (1 = the next) writes 1 + layer into its error word and stores nothing
int fake_skinny_f32_counter_mismatches(void);    // seams whose counter did not hold target - G before the launch, or lay outside its block
}
