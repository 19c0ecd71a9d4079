// chain_args.h - kernel arguments of brgemm_bf16_lw.hip: one whole-layer (fused) bf16 BRGEMM, or a CHAIN of them run in
// one launch (layer l+1 reads layer l's output rows; xsmm_hip_fused_brgemm_chain_invoke in runtime.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "brgemm_bf16_lw_launch.h" // the launch modes (BLW_*) of the bf16 loader-wave launchers below

namespace tpp {

constexpr int CH_MAXL = 8;                                  // layers per chain launch
constexpr int CHAIN_CNT_STRIDE = 32;                         // counters 128 B apart: device-scope atomics on ONE line serialise (~12 ns each)
constexpr unsigned long long CHAIN_TIMEOUT_TICKS = 5000000; // bound of every in-kernel spin: 50 ms of s_memrealtime (100 MHz)

struct ChainLayer {
  const void *B;   // VNNI-2 weights [K/2][ldb][2]
  const void *D;   // bias row (EP_BIAS)
  void *C;         // output [m][ldc]; the A operand of the next layer
  int64_t ldb, ldc, stride_a, stride_b; // elements (stride_a applies to this layer's A = previous C / the chain input)
  int k, br, ep, pad;                   // k per batch element (multiple of 64), batch count, EP_* bits; pad: 0 - a mixed-width chain: the layer's n
};

struct ChainArgs {
  const void *A;   // input of layer 0 [m][lda]
  int64_t lda;
  unsigned *cnt;   // chain mode: arrival counters [nlayers - 1][tiles_m] (CHAIN_CNT_STRIDE words apart), monotonic across launches
  unsigned *err;   // chain mode: set to 1 + layer by a workgroup whose hand-off wait timed out
  unsigned target; // chain mode: value every counter reaches in this launch (epoch * tiles_n); a mixed-width chain: the epoch itself
  int m, n;        // rows and columns of every layer's output (a mixed-width chain: n of the widest layer, L[l].pad per layer)
  int nlayers;
  int tiles_m, tiles_n; // filled by the launcher
  int xm;               // filled by the launcher: XCD grid xm x (8 / xm) over the tile grid, 0 = linear tile order
  int groups;           // a multi-round chain (launch_bf16_chain, BLW_CHAIN_ROUNDS): resident row groups G, the grid is G x tiles_n; column rounds (launch_bf16_chain_wrounds): resident workgroup columns W; a skinny-batch chain (launch_bf16_skinny_chain): the resident workgroups G; 0 in every other launch
  // Unused. Keeps L at byte 72 of the argument block: without these bytes every L[] load moves and the compiler assigns
  // registers differently in the f32 chain kernels' K loop, a code change that would have to be measured on its own.
  char reserved[8];
  ChainLayer L[CH_MAXL];
  // GROUPED launches (round 6, the tile queue's bf16 groups: launch_bf16_lw_grouped): a work list of tile invokes of ONE descriptor - every
  // workgroup takes A, B, C, D and the batch count of ITS item from the list, everything else (leading dimensions, strides, k, epilogue)
  // from L[0] / lda as in a single layer; m x n is then ONE item's shape and item_subs = tiles_m * tiles_n the workgroups per item
  const void *items; // WorkItem[n] in device-visible memory, nullptr in every other launch
  int item_subs;
  int pad_items;
};
static_assert(offsetof(ChainArgs, L) == 72, "the kernels' code depends on where the layer table lies");

// The bf16 loader-wave launchers (brgemm_bf16_lw.hip). mode: a launch mode of brgemm_bf16_lw_launch.h (BLW_*), whose blw_launch_ok says what each
// refuses - hipErrorInvalidValue, nothing launched. tile: 0 = 32x64 (K split over two wave groups), 1 = 64x64, 2 = 64x128, 3 = 128x128,
// 4 = 32x32 + K2 (gemm_plan.h blw_tile_dims). b_kind: the B image, 0 VNNI-2, 2 flat [k][ldb], 4 VNNI-4 [k/4][ldb][4] (every layer the same).
// one layer: BLW_LAYER, BLW_EDGE (xsmm_hip_set_edge_tiles), BLW_KEDGE (xsmm_hip_set_edge_k_bf16), BLW_KEDGE8 (xsmm_hip_set_edge_k8_bf16)
hipError_t launch_bf16_lw(int mode, int tile, int b_kind, const ChainArgs &a, hipStream_t s);
// a chain: BLW_LAYER, BLW_CHAIN_EDGE (xsmm_hip_set_chain_edge), BLW_CHAIN_ROUNDS (xsmm_hip_set_chain_rounds; a.groups row groups, the caller
// guarantees groups * (n / BN) <= the stream's compute units)
hipError_t launch_bf16_chain(int mode, int tile, int b_kind, const ChainArgs &a, hipStream_t s);
// a ragged-WIDTH chain (brgemm_bf16_lw_chain_ragged.hip, BLW_CHAIN_RAGGED, xsmm_hip_set_chain_ragged): ceil(m / BM) x ceil(n / BN) workgroups,
// at most the stream's compute units (the caller's guarantee); per layer k >= 64 and k % 8 == 0; blw_chain_ragged_launch_ok is what it refuses
hipError_t launch_bf16_chain_ragged(int tile, int b_kind, const ChainArgs &a, hipStream_t s);
// a MIXED-WIDTH chain (brgemm_bf16_lw_chain_widths.hip, BLW_CHAIN_WIDTHS, xsmm_hip_set_chain_widths): layer l has a.L[l].pad columns, a.n is
// the widest layer's (the grid: m / BM x a.n / BN workgroups, at most the stream's compute units - the caller's guarantee) and a.target
// the launch's EPOCH: cnt[l][*] reaches epoch * (a.L[l].pad / BN). blw_chain_widths_launch_ok is what it refuses
hipError_t launch_bf16_chain_widths(int tile, int b_kind, const ChainArgs &a, hipStream_t s);
// a mixed-width chain in COLUMN ROUNDS (brgemm_bf16_lw_chain_wrounds.hip, BLW_CHAIN_WROUNDS, xsmm_hip_set_chain_width_rounds): the arguments of
// launch_bf16_chain_widths + a.groups = W resident workgroup columns, 1 <= W < a.n / BN (the grid: m / BM x W workgroups, at most the
// stream's compute units - the caller's guarantee). blw_chain_wrounds_launch_ok is what it refuses
hipError_t launch_bf16_chain_wrounds(int tile, int b_kind, const ChainArgs &a, hipStream_t s);
// a RAGGED mixed-width chain (brgemm_bf16_lw_chain_wragged.hip, BLW_CHAIN_WRAGGED, xsmm_hip_set_chain_widths_ragged): launch_bf16_chain_widths'
// arguments with any m >= BM, n(l) >= BN in multiples of 8 and k(l) >= 64 in multiples of 8; the grid is ceil(m / BM) x ceil(a.n / BN)
// workgroups, at most the stream's compute units - the caller's guarantee -, cnt[l][*] reaches epoch * ceil(a.L[l].pad / BN).
// blw_chain_wragged_launch_ok is what it refuses
hipError_t launch_bf16_chain_wragged(int tile, int b_kind, const ChainArgs &a, hipStream_t s);
// a chain on the 256x256 LDS-DMA tile (brgemm_bf16_dma256_chain.hip, xsmm_hip_set_chain_dma256; maps in brgemm_bf16_dma256_chain.h): every layer
// m x n with 256 dividing both, k(l) in 32-k chunks, beta 0; b_kind 0 VNNI-2 / 2 flat / 4 VNNI-4; a.groups = resident row groups G (0: one
// round, G = m / 256); the grid is G x n / 256 workgroups, at most the stream's compute units - the caller's guarantee. Refuses with
// hipErrorInvalidValue, launching nothing, whatever the kernel cannot run
hipError_t launch_bf16_dma256_chain(int b_kind, const ChainArgs &a, hipStream_t s);
// a chain of SKINNY-BATCH layers (brgemm_bf16_skinny_chain.hip, xsmm_hip_set_chain_skinny; schedule in brgemm_bf16_skinny_chain.h): 1 <= m <= 31
// rows, layer l of a.L[l].pad columns (n >= bn, n % 8 == 0) and k(l) >= 8 in multiples of 8, beta 0, on column blocks of bn = 16 / 32 / 64;
// b_kind 0 VNNI-2 / 2 flat / 4 VNNI-4; a.groups = G resident workgroups, the grid, at most the stream's compute units - the caller's
// guarantee; ONE counter per seam, cnt[l] reaches a.target = epoch * G. Refuses with hipErrorInvalidValue, launching nothing, whatever
// the kernel does not assume (the list stands at the launcher)
hipError_t launch_bf16_skinny_chain(int b_kind, int bn, const ChainArgs &a, hipStream_t s);
// tile invokes of one bf16 descriptor in one launch (tile 0 = 32x64 + K2, 1 = 64x64, 4 = 32x32 + K2; b_kind 0 VNNI-2 / 4 VNNI-4; a.m x a.n = one item's
// shape, a.L[0] / a.lda its leading dimensions and strides; every item's batch count >= 1; even_chunks: every item has an even chunk count)
hipError_t launch_bf16_lw_grouped(int tile, int b_kind, const ChainArgs &a, const void *items, int n_items, bool even_chunks, hipStream_t s);
// 2 x 2 blocks of 64x64 items on the 128x128 tile (quads: QuadItem[n_quads], xsmm_desc.h; a.m = a.n = 128, leading dimensions / strides / k the items')
hipError_t launch_bf16_lw_quads(int b_kind, const ChainArgs &a, const void *quads, int n_quads, hipStream_t s);

// f32 chains (brgemm_f32_lw.hip): tile 1 = 64x64 + K2, 2 = 64x32 + K4 - the 64-row K-split loader-wave tiles (gemm_plan.h f32_chain_tile_dims)
hipError_t launch_f32_chain(int tile, const ChainArgs &a, hipStream_t s);

} // namespace tpp
