// fake_chain.h - TEST INFRASTRUCTURE for tests/test_chain_dispatch.py, never part of the product library: what the launch stand-ins of
// fake_chain.cpp record, and the knobs the driver turns. One record per chain launch that reached a launcher.
#pragma once
#include "../../tpp-mlir_amd/csrc/xsmm_desc.h"
#include "../../tpp-mlir_amd/csrc/chain_args.h"

// the nine launch forms of rt_chain.h try_chain_launch
enum FakeChainForm : int { FC_PLAIN, FC_F32, FC_EDGE, FC_ROUNDS, FC_RAGGED, FC_WIDTHS, FC_WROUNDS, FC_WRAGGED, FC_DMA256, FC_FORMS };
inline const char *fake_chain_form_name(int f) {
  static const char *const names[FC_FORMS] = {"plain", "f32", "edge", "rounds", "ragged", "widths", "wrounds", "wragged", "dma256"};
  return f >= 0 && f < FC_FORMS ? names[f] : "?";
}

struct FakeChainLaunch {
  int form;          // FakeChainForm
  int tile;          // the launcher's tile argument (3 for the 256x256 tile's launcher, which takes none)
  int b_kind;        // 0 VNNI-2, 2 flat, 4 VNNI-4 (0 for f32)
  int bm, bn;        // the tile's rows and columns
  int tiles_m, grid_n; // row blocks; workgroup columns of the launch (the grid is rows x grid_n, rows = groups in the row-round forms)
  long long grid;    // resident workgroups
  tpp::ChainArgs a;  // the argument block as the launcher received it
  int starved;       // the stand-in wrote the error word and stored nothing (fake_chain_starve)
};
// one record per launch_gemm (the call-by-call path and the re-runs)
struct FakeGemmLaunch {
  const tpp::GemmDesc *d;
  const void *A, *B, *D;
  void *C;
  long long br;
};

extern "C" {
int fake_chain_launches(void);
const FakeChainLaunch *fake_chain_launch(int i);
int fake_gemm_launches(void);
const FakeGemmLaunch *fake_gemm_launch(int i);
void fake_chain_clear(void);            // forget the records (counters of the model live in the "device" blocks and stay)
void fake_chain_set_compute(int on);    // 0: the stand-ins record and count, and store nothing (decision sweeps on large shapes)
void fake_chain_starve(int nth, int layer); // the nth chain launch from now (1 = the next) writes 1 + layer into its error word and stores nothing
int fake_chain_counter_mismatches(void); // seams at which a counter did not hold expected_after - arrivals, or lay outside its block
int fake_hip_compute_units(void);
long fake_hip_cu_mask_queries(void);     // calls of hipExtStreamGetCUMask so far (tests/tsan/fake_hip_host.h): how often the stream's compute units were asked for
}
