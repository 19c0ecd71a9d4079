// brgemm_bf16_skinny_split.h - the maps of the K split ACROSS workgroups of the skinny-batch bf16 kernel (brgemm_bf16_skinny_split.hip,
// xsmm_hip_set_skinny_split), on top of brgemm_bf16_skinny.h: which steps a part takes, how a part's run is dealt over its waves, which
// workgroup of the linear grid is which (part, column block), and where a partial accumulator register lands in the stream's scratch block.
// The kernel, its launcher, the planner (gemm_plan.cpp) and a CPU test (tests/test_skinny_split_map.py) all include this file. Nothing here
// needs a device: it compiles with any C++14 host compiler.
//
// The S_all = br * skn_steps(k) steps of a call, numbered as in the unsplit kernel, go to P_eff = min(P, S_all) parts in contiguous runs
// (the first S_all % P_eff parts take one step more); a part's run goes to skn_waves(run length) waves exactly as a whole call's steps do.
// blocks * P_eff workgroups: blockIdx.x = part * blocks + block, so workgroups that start together share a k range - A's bytes.
#pragma once
#include "brgemm_bf16_skinny.h"

namespace tpp {

constexpr int SKS_PMAX = 16; // most parts (= SPLIT_MAX of split_scratch.h: the launcher asserts it)

// P_eff; below 2 the call is the plain skinny launch
constexpr int sks_parts(int P, long long s_all) { return P < s_all ? P : (int)s_all; }
// THE PARTS: part p of P_eff takes steps [first, first + count) of S_all - the formulas of the deal over waves
constexpr int sks_part_count(int p, int P_eff, int S_all) { return skn_wave_count(p, P_eff, S_all); }
constexpr int sks_part_first(int p, int P_eff, int S_all) { return skn_wave_first(p, P_eff, S_all); }
// THE DEAL inside a part: wave w of skn_waves(run) takes steps [first, first + count) of the CALL. The workgroups of a launch all have the
// waves of part 0 (the longest run: sks_block_waves); a part with a shorter run leaves its last wave idle.
constexpr int sks_block_waves(int P_eff, int S_all) { return skn_waves(sks_part_count(0, P_eff, S_all)); }
constexpr int sks_wave_count(int w, int p, int P_eff, int S_all) {
  return w < skn_waves(sks_part_count(p, P_eff, S_all)) ? skn_wave_count(w, skn_waves(sks_part_count(p, P_eff, S_all)), sks_part_count(p, P_eff, S_all)) : 0;
}
constexpr int sks_wave_first(int w, int p, int P_eff, int S_all) {
  return sks_part_first(p, P_eff, S_all) + skn_wave_first(w, skn_waves(sks_part_count(p, P_eff, S_all)), sks_part_count(p, P_eff, S_all));
}
// the ragged-k mask follows a step's position in its BATCH ELEMENT: step t of the call is step t % skn_steps(k) of element t / skn_steps(k)
constexpr bool sks_step_masked(int t, int k) { return t % skn_steps(k) == skn_steps(k) - 1 && k % SKN_KSTEP != 0; }
// THE GRID: linear, part-major
constexpr int sks_grid(int blocks, int P_eff) { return blocks * P_eff; }
constexpr int sks_grid_part(int bid, int blocks) { return bid / blocks; }
constexpr int sks_grid_block(int bid, int blocks) { return bid % blocks; }
// THE SCRATCH: partial [block][part][s * C + j][lane] as f32x4 - MB * BN floats per (block, part), 1 KiB contiguous per wave store
// instruction. Float index of element e (0 .. 3) of accumulator register reg = s * C + j of lane l; one arrival counter per block.
constexpr long long sks_slot_floats(int mb, int bn) { return (long long)mb * bn; }
constexpr long long sks_floats(long long blocks, int P_eff, int mb, int bn) { return blocks * P_eff * sks_slot_floats(mb, bn); }
constexpr long long sks_float_index(int block, int part, int P_eff, int mb, int bn, int reg, int l, int e) {
  return ((long long)block * P_eff + part) * sks_slot_floats(mb, bn) + (long long)reg * 256 + 4 * l + e;
}
// what the launcher refuses (the limits: split_scratch.h SPLIT_MAX_TILES, SPLIT_MAX, SPLIT_SCRATCH_FLOATS)
constexpr bool sks_launch_fits(long long blocks, int P_eff, int mb, int bn, long long max_tiles, int max_parts, long long max_floats) {
  return P_eff >= 2 && P_eff <= max_parts && blocks >= 1 && blocks <= max_tiles && sks_floats(blocks, P_eff, mb, bn) <= max_floats;
}

} // namespace tpp
