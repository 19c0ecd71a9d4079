// brgemm_bf16_lw_chain_widths.h - the schedule of a MIXED-WIDTH layer chain on the bf16 loader-wave tiles (brgemm_bf16_lw.hip GRP = 9, opt-in:
// xsmm_hip_set_chain_widths), written once as plain functions: the loader, the MFMA waves, the launcher (brgemm_bf16_lw_chain_widths.hip) and
// a CPU test (tests/test_chain_widths_schedule.py) all include this file. Nothing here needs a device: it compiles with any C++14 host compiler.
//
// A chain of L layers, layer l of n(l) columns, every n(l) in whole column tiles of BN, on m / BM x max_l(n(l) / BN) co-resident workgroups.
// Workgroup (tm, tn) computes tile (tm, tn) of every layer that HAS a column tile tn - the layer is ACTIVE for it - and sits out the others:
// all its waves skip an inactive layer alike, without a barrier and without a ring slot (s0 advances on active layers only).
//   counters : cnt[l][tm] receives one arrival from every ACTIVE workgroup of row block tm, n(l) / BN per launch. The argument block carries
//              the launch's EPOCH (the block's launches so far, this one included); the value cnt[l][*] has reached when layer l is stored
//              is epoch * (n(l) / BN), in wrap-around unsigned arithmetic like the comparison it goes into.
//   waits    : a workgroup polls cnt[l - 1][tm] in front of EVERY active layer l > 0 - its first one included, whether or not it took part
//              in layer l - 1. The producers of that counter wait only for counters of layer l - 2: no wait is cyclic.
//   seams    : after every active layer but the chain's LAST one (l + 1 < L) the workgroup drains its write-through stores, meets at the
//              barriers R1 (tiles with a K split) and S1 and adds 1 to cnt[l][tm] - also when the layer is the workgroup's own last active
//              one: its consumers are other workgroups. Only layer L - 1 goes unsignalled.
//   run-ahead: the B loaders request the first panels of the workgroup's next ACTIVE layer during the tail of the current one (weights
//              depend on no hand-off), under the plain chain's condition: every layer has at least a ring of barrier intervals.
#pragma once

namespace tpp {

// does layer l (n_l columns) have a column tile tn on tiles of bn columns?
constexpr bool chain_widths_active(int tn, int n_l, int bn) { return tn * bn < n_l; }
// column tiles of a layer; of the grid (the widest layer's). n_of(l) = layer l's n.
constexpr int chain_widths_tiles(int n_l, int bn) { return n_l / bn; }
template <class NF> constexpr int chain_widths_grid(int L, int bn, NF n_of) {
  int w = 0;
  for (int l = 0; l < L; ++l)
    if (chain_widths_tiles(n_of(l), bn) > w) w = chain_widths_tiles(n_of(l), bn);
  return w;
}
// the first active layer of column tile tn behind layer l (l = -1: the first of all); L when there is none
template <class NF> constexpr int chain_widths_next(int tn, int l, int L, int bn, NF n_of) {
  for (int i = l + 1; i < L; ++i)
    if (chain_widths_active(tn, n_of(i), bn)) return i;
  return L;
}
template <class NF> constexpr int chain_widths_first(int tn, int L, int bn, NF n_of) { return chain_widths_next(tn, -1, L, bn, n_of); }
// ... and its last one; -1 when there is none (never: tn lies inside the widest layer)
template <class NF> constexpr int chain_widths_last(int tn, int L, int bn, NF n_of) {
  for (int i = L - 1; i >= 0; --i)
    if (chain_widths_active(tn, n_of(i), bn)) return i;
  return -1;
}
// what cnt[l][*] has reached when every producer of layer l of launch `epoch` has arrived
constexpr unsigned chain_widths_target(unsigned epoch, int n_l, int bn) { return epoch * (unsigned)chain_widths_tiles(n_l, bn); }
// does a workgroup signal after its active layer l? (every layer but the chain's last)
constexpr bool chain_widths_signals(int l, int L) { return l + 1 < L; }
// ... and wait in front of it?
constexpr bool chain_widths_waits(int l) { return l > 0; }
// the ring: slot of the next active layer's chunk 0 after an active layer of T barrier intervals
constexpr int chain_widths_next_s0(int s0, int T, int nslot) { return (s0 + T) % nslot; }

} // namespace tpp
