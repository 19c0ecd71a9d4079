// brgemm_bf16_lw_chain_wrounds.h - the schedule of a MIXED-WIDTH layer chain in COLUMN ROUNDS on the bf16 loader-wave tiles (brgemm_bf16_lw.hip
// GRP = 10, opt-in: xsmm_hip_set_chain_width_rounds), written once as plain functions: the loader, the MFMA waves, the launcher
// (brgemm_bf16_lw_chain_wrounds.hip), the planner (gemm_plan.cpp plan_chain_width_rounds) and a CPU test
// (tests/test_chain_width_rounds_schedule.py) all include this file. Nothing here needs a device: it compiles with any C++14 host compiler.
//
// A chain of L layers, layer l of T(l) = n(l) / BN column tiles, on m / BM x W RESIDENT workgroups, 1 <= W < max_l T(l): W column GROUPS.
// Workgroup (tm, c) walks LAYER-MAJOR - for l: for tn = c, c + W, .. while tn < T(l) - one STEP (l, tn) being tile (tm, tn) of layer l. A
// layer with c >= T(l) has no step for the group: it is sat out as in the one-round mixed-width chain (brgemm_bf16_lw_chain_widths.h), all
// waves alike, without a barrier and without a ring slot. Groups may make unequal numbers of steps in a layer.
//   counters : exactly the mixed-width chain's. cnt[l][tm] receives one arrival after EVERY step of layer l < L - 1 on row block tm, T(l)
//              per launch, whichever group made the step; the argument block carries the EPOCH and the value waited for is
//              chain_widths_target(epoch, n(l), BN). The counter block is keyed like that chain's (row blocks, the widest layer's column
//              tiles, every layer's own): a launch of either mode adds the same numbers.
//   waits    : a workgroup polls cnt[l - 1][tm] in front of EVERY step of an active layer l > 0. After the first step of a layer the poll
//              passes at once (the counter only grows).
//   progress : step (l, .) waits only for cnt[l - 1][tm], whose producers are the steps of layer l - 1 on row block tm. Those lie EARLIER in
//              their own workgroups' walks than any step of layer l or later (layer-major) and wait in turn only for counters of layer
//              l - 2. All m / BM x W workgroups are resident, so by induction over the layers every step of layer l - 1 is made and no
//              wait is cyclic.
//   seams    : after every step but those of the chain's LAST layer the workgroup drains its write-through stores, meets at R1 (tiles with
//              a K split) and S1 and adds 1 to cnt[l][tm]. After a step of layer L - 1 that another step follows: S1 alone (the staging
//              tiles in retired A halves have been read back before the A loader requests the next step's panels).
//   ring     : s0 advances by the step's barrier intervals after every step (chain_widths_next_s0). One chunk per barrier only (SUP = 1).
//   run-ahead: the B loaders request the first panels of the workgroup's NEXT STEP - the next column tile of the same layer, or else the
//              first tile of its next active layer - during the tail of the current one, under the plain chain's condition: every layer
//              has at least a ring of barrier intervals. THE A LOADERS NEVER RUN AHEAD, neither across a layer boundary (the rows are not
//              released yet) nor into a next step of the same layer: the epilogue's staging tiles live in the A halves of the ring slots
//              the run-ahead would fill, so the A panels of every step are requested behind S1, as in the multi-round chain (GRP = 7).
#pragma once
#include "brgemm_bf16_lw_chain_widths.h"

namespace tpp {

// steps column group c of W makes in a layer of T column tiles; 0 for a group that does not exist or sits the layer out
constexpr int chain_wrounds_steps(int c, int W, int T) { return c >= 0 && c < W && c < T ? (T - c + W - 1) / W : 0; }
// the r-th column tile of group c
constexpr int chain_wrounds_tile(int c, int r, int W) { return c + r * W; }
// the group that owns column tile tn
constexpr int chain_wrounds_group(int tn, int W) { return tn % W; }
// The WALK of a workgroup, as the kernel makes it: tn starts as the group c = its first column tile, l = 0; T = the column tiles of layer l.
// Does the group own a further column tile of this layer behind tn? (false for a layer it sits out: c >= T)
constexpr bool chain_wrounds_more(int tn, int W, int T) { return tn + W < T; }
// from the step (or the sat-out layer) l at column tile tn to the next: the group's next column tile of the same layer, or back to its
// first tile in the next layer. The walk has ended when l reaches the layer count.
constexpr void chain_wrounds_next(int &tn, int &l, int W, int T) {
  if (chain_wrounds_more(tn, W, T)) {
    tn += W;
  } else {
    tn = chain_wrounds_group(tn, W);
    ++l;
  }
}
// rounds of a layer of T column tiles on W groups: the steps of group 0, the longest walk of the layer
constexpr int chain_wrounds_rounds(int T, int W) { return (T + W - 1) / W; }
// the largest W that fits: fewer than the widest layer's column tiles, and m / BM x W within the compute units (0: not even W = 1 fits;
// maxT = 1 gives 0 as well - nothing to round)
constexpr int chain_wrounds_max_groups(int maxT, int tiles_m, long long cus) {
  return tiles_m <= 0 ? 0 : (long long)(maxT - 1) < cus / tiles_m ? maxT - 1 : (int)(cus / tiles_m);
}
// the rule's W for maxT column tiles when at most wfit fit (wfit >= 1): as few rounds of the widest layer as wfit allows, balanced
constexpr int chain_wrounds_groups(int maxT, int wfit) {
  return (maxT + chain_wrounds_rounds(maxT, wfit) - 1) / chain_wrounds_rounds(maxT, wfit);
}

} // namespace tpp
