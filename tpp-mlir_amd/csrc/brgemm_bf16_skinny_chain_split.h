// brgemm_bf16_skinny_chain_split.h - the schedule of a skinny-batch bf16 LAYER CHAIN whose layers are K-split over workgroups inside the one
// launch (brgemm_bf16_skinny_chain_split.hip, opt-in: xsmm_hip_set_chain_skinny_split), on top of brgemm_bf16_skinny_chain.h (the seam, the counter
// block, what the launcher refuses of a layer) and brgemm_bf16_skinny_split.h (a part's steps, the deal over its waves, the scratch slots). The
// kernel, its launcher, the planner (gemm_plan.cpp plan_chain_skinny) and a CPU test (tests/test_chain_skinny_split_cpu.py) include this file.
// Nothing here needs a device: it compiles with any C++14 host compiler.
//
// Layer l has blocks_l = skn_blocks(n_l, BN) column blocks and S_l = br_l * skn_steps(k_l) steps. Every block gets P_l = sks_parts(P, S_l) =
// min(P, S_l) parts (a layer of one step has one: its blocks are the unsplit chain's). The layer's work is blocks_l * P_l UNITS, part-major as
// sks_grid_part: unit u = part * blocks_l + block. Workgroup w of G takes the units w, w + G, .. - none where w is at or beyond the unit
// count -, and arrives at the seam ONCE per layer, behind its last unit or at once: a launch adds exactly G to each seam counter, as the
// unsplit chain.
#pragma once
#include "brgemm_bf16_skinny_chain.h"
#include "brgemm_bf16_skinny_split.h"

namespace tpp {

// the parts asked for: 2 .. 16 (the switch's forced values); below 2 the launch is the unsplit chain's
constexpr bool skcs_parts_ok(int P) { return P >= 2 && P <= SKS_PMAX; }
// PER LAYER: steps, parts, units
constexpr int skcs_steps(long long br, int k) { return (int)(br * skn_steps(k)); }
constexpr int skcs_layer_parts(int P, long long br, int k) { return sks_parts(P, br * skn_steps(k)); }
constexpr int skcs_units(int n, int bn, int P, long long br, int k) { return skn_blocks(n, bn) * skcs_layer_parts(P, br, k); }
// UNITS: unit -> (part, block), and the walk of a workgroup - skc_owned / skc_block / skc_arrive_after over units instead of blocks
constexpr int skcs_unit_part(int u, int blocks) { return sks_grid_part(u, blocks); }
constexpr int skcs_unit_block(int u, int blocks) { return sks_grid_block(u, blocks); }
constexpr int skcs_owned(int w, int G, int units) { return skc_owned(w, G, units); }
constexpr int skcs_unit(int w, int G, int i) { return skc_block(w, G, i); }
// G by rule: a workgroup per unit of the layer with the most units, at most the compute units (every workgroup must be resident)
constexpr int skcs_groups(long long max_units, long long cus) { return max_units < cus ? (int)max_units : (int)cus; }
// WAVES of a layer: its deepest part's (part 0); the launch has the most over the layers. A layer with P_l = 1 has the unsplit layer's.
constexpr int skcs_layer_waves(int P, long long br, int k) { return sks_block_waves(skcs_layer_parts(P, br, k), skcs_steps(br, k)); }
// THE SCRATCH a layer needs: one slot of MB * BN floats per (block, part) and one arrival counter per block, if it is split at all. The
// launch asks for the most over its layers - every layer reuses the one region (the order of events: the kernel's header).
constexpr long long skcs_layer_floats(int n, int bn, int mb, int P, long long br, int k) {
  return skcs_layer_parts(P, br, k) >= 2 ? sks_floats(skn_blocks(n, bn), skcs_layer_parts(P, br, k), mb, bn) : 0;
}
constexpr long long skcs_layer_counters(int n, int bn, int P, long long br, int k) { return skcs_layer_parts(P, br, k) >= 2 ? skn_blocks(n, bn) : 0; }
// what the launcher refuses of a layer (the limits: split_scratch.h SPLIT_MAX_TILES, SPLIT_MAX, SPLIT_SCRATCH_FLOATS - for the planner, which
// cannot include that file, the first and the last once more; the launcher asserts that they are the same); an unsplit layer fits
constexpr long long SKCS_MAX_TILES = 4096, SKCS_MAX_FLOATS = 8LL << 20;
constexpr bool skcs_layer_fits(int n, int bn, int mb, int P, long long br, int k, long long max_tiles, int max_parts, long long max_floats) {
  return skcs_layer_parts(P, br, k) < 2 || sks_launch_fits(skn_blocks(n, bn), skcs_layer_parts(P, br, k), mb, bn, max_tiles, max_parts, max_floats);
}

} // namespace tpp
