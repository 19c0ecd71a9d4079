// brgemm_bf16_lw_chain_rounds.h - the step maps of a MULTI-ROUND layer chain (brgemm_bf16_lw.hip GRP = 7, opt-in: xsmm_hip_set_chain_rounds),
// written once as plain functions: the kernel, its launcher, the planner (gemm_plan.cpp) and a CPU test (tests/test_chain_rounds_steps.py)
// all include this file. Nothing here needs a device: it compiles with any C++14 host compiler.
//
// A chain of L layers on tiles_m x tiles_n output tiles, more than the compute units hold at once, runs on G x tiles_n RESIDENT workgroups:
// G row GROUPS. Workgroup (g, tn) owns the row blocks tm = g + r * G, r = 0, 1, .. while tm < tiles_m - groups may own unequal numbers of
// blocks - and walks them LAYER-MAJOR: step (l, r) = layer l of its r-th block, in the order  for l: for r:. A step of layer l > 0 waits
// for the counter of ITS row block in layer l - 1, i.e. for step (l - 1, r) of the workgroups (g, *): a step that lies earlier in their own
// order. All workgroups are resident, so no wait is cyclic.
#pragma once

namespace tpp {

// row blocks group g of G owns among tiles_m (= the steps it makes per layer); 0 for a group that does not exist
constexpr int chain_rounds_steps(int g, int G, int tiles_m) { return g >= 0 && g < G && g < tiles_m ? (tiles_m - g + G - 1) / G : 0; }
// the r-th row block of group g
constexpr int chain_rounds_block(int g, int r, int G) { return g + r * G; }
// the group that owns row block tm
constexpr int chain_rounds_group(int tm, int G) { return tm % G; }
// The WALK of a workgroup, as the kernel makes it: tm starts as the group g = its first row block, l = 0.
// Does the group own a further row block behind tm?
constexpr bool chain_rounds_more(int tm, int G, int tiles_m) { return tm + G < tiles_m; }
// from the step of layer l on row block tm to the next one: the group's next row block of the same layer, or back to its first block
// in the next layer. The walk has ended when l reaches the layer count.
constexpr void chain_rounds_next(int &tm, int &l, int G, int tiles_m) {
  if (chain_rounds_more(tm, G, tiles_m)) {
    tm += G;
  } else {
    tm = chain_rounds_group(tm, G);
    ++l;
  }
}
// rounds of G groups over tiles_m row blocks: the steps per layer of group 0, the longest walk
constexpr int chain_rounds_rounds(int tiles_m, int G) { return (tiles_m + G - 1) / G; }
// most groups tiles_n-wide rows of workgroups fit on cus compute units (0: a row of tiles is wider than the compute units)
constexpr int chain_rounds_max_groups(int tiles_n, long long cus) { return tiles_n > 0 ? (int)(cus / tiles_n) : 0; }
// the rule's groups for tiles_m row blocks when at most gmax fit (gmax >= 1): as few rounds as gmax allows, the rounds balanced
constexpr int chain_rounds_groups(int tiles_m, int gmax) {
  return (tiles_m + chain_rounds_rounds(tiles_m, gmax) - 1) / chain_rounds_rounds(tiles_m, gmax);
}

} // namespace tpp
