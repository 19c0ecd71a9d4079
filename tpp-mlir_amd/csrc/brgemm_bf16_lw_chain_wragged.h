// brgemm_bf16_lw_chain_wragged.h - the schedule of a RAGGED MIXED-WIDTH layer chain on the bf16 loader-wave tiles (brgemm_bf16_lw.hip GRP = 11,
// opt-in: xsmm_hip_set_chain_widths_ragged), written once as plain functions: the loader, the MFMA waves, the launcher
// (brgemm_bf16_lw_chain_wragged.hip), the planner (gemm_plan.cpp plan_chain_widths_ragged) and a CPU test
// (tests/test_chain_wragged_schedule.py) all include this file. Nothing here needs a device: it compiles with any C++14 host compiler.
//
// The mixed-width chain (brgemm_bf16_lw_chain_widths.h) with the ragged-width chain's layers (brgemm_bf16_lw_chain_ragged.h): a chain of L
// layers, layer l of n(l) columns - n(l) >= BN, n(l) % 8 == 0, ANY such n -, on ceil(m / BM) x max_l ceil(n(l) / BN) co-resident workgroups.
// What is said here is what the two differ in when combined; everything else is those headers' functions, used as they are.
//   active   : workgroup (tm, tn) is active in layer l iff tn < ceil(n(l) / BN) (chain_widths_active: tn * BN < n(l)). It sits out the other
//              layers, all its waves alike, with no barrier and no ring slot.
//   columns  : PER LAYER. In layer l the tile's first column is chain_ragged_col0(tn, n(l), BN) and its first own column
//              chain_ragged_own_col(tn, n(l), BN): the same workgroup can be the shifted last tile of one layer and an interior tile of the
//              next. Both are recomputed at every active layer; neither is fixed at kernel entry. The bias row and the 16-byte pieces a tile
//              stores follow from them.
//   rows     : brgemm_bf16_lw_chain_edge.h - the last row block shifted back to end at row m, storing its own rows only, and waiting at a
//              seam on the counters of chain_edge_first_block .. chain_edge_last_block.
//   k        : per layer, chain_ragged_k_ok(k): a batch element is bkedge_chunks(k) chunks, the last one shifted back; the skipped half steps
//              are chain_ragged_skip_halves', the test period chain_ragged_test_period's.
//   counters : cnt[l][tm] receives one arrival from every workgroup of row block tm that is ACTIVE in layer l: ceil(n(l) / BN) per launch.
//              The argument block carries the epoch; the wait in front of an active layer l > 0 is for epoch * ceil(n(l - 1) / BN) on each of
//              the one or two row-block counters, in the wrap-around unsigned arithmetic of chain_widths_target. A workgroup waits in front
//              of EVERY active layer l > 0, whether or not it took part in layer l - 1, and signals after every active layer but the
//              chain's last. The producers of a counter of layer l - 1 wait only for counters of layer l - 2: no wait is cyclic.
//   ring     : carried through the workgroup's ACTIVE layers only: s0 advances by chain_ragged_layer_chunks(k(l), br(l)) on an active layer
//              and not at all on a sat-out one. A layer may start at any slot. Loader and MFMA waves count with the same function.
//   run-ahead: NONE across a seam, from either loader, as in the ragged-width chain: every active layer's first request goes to s0 behind
//              the seam. This is the one form built.
//   barriers : one chunk per barrier (SUP = 1) only.
#pragma once
#include "brgemm_bf16_lw_chain_edge.h"
#include "brgemm_bf16_lw_chain_ragged.h"
#include "brgemm_bf16_lw_chain_widths.h"

namespace tpp {

// column tiles of a layer (ceil-divided); of the grid (the widest layer's). n_of(l) = layer l's n.
constexpr int chain_wragged_tiles(int n_l, int bn) { return chain_ragged_tiles_n(n_l, bn); }
template <class NF> constexpr int chain_wragged_grid(int L, int bn, NF n_of) {
  int w = 0;
  for (int l = 0; l < L; ++l)
    if (chain_wragged_tiles(n_of(l), bn) > w) w = chain_wragged_tiles(n_of(l), bn);
  return w;
}
// is workgroup column tn active in a layer of n_l columns? (chain_widths_active: tn * bn < n_l, i.e. tn < ceil(n_l / bn))
constexpr bool chain_wragged_active(int tn, int n_l, int bn) { return chain_widths_active(tn, n_l, bn); }
// what cnt[l][*] has reached when every producer of layer l of launch `epoch` has arrived (wrap-around, as chain_widths_target)
constexpr unsigned chain_wragged_target(unsigned epoch, int n_l, int bn) { return epoch * (unsigned)chain_wragged_tiles(n_l, bn); }
// the ring: s0 of the layer behind layer (k, br) - it moves on an active layer only
constexpr int chain_wragged_next_s0(int s0, bool active, int k, int br, int nslot) { return active ? chain_ragged_next_s0(s0, k, br, nslot) : s0; }
// s0 of layer l for workgroup column tn, given the layers before it
template <class NF> constexpr int chain_wragged_s0(int tn, int l, int bn, NF n_of, const int *k, const int *br, int nslot) {
  int s0 = 0;
  for (int i = 0; i < l; ++i) s0 = chain_wragged_next_s0(s0, chain_wragged_active(tn, n_of(i), bn), k[i], br[i], nslot);
  return s0;
}

} // namespace tpp
