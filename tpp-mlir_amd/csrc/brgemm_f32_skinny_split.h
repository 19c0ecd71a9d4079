// brgemm_f32_skinny_split.h - the maps of the K split ACROSS workgroups of the skinny-batch f32 kernel (brgemm_f32_skinny_split.hip,
// xsmm_hip_set_skinny_f32_split), on top of brgemm_f32_skinny.h: which steps a part takes, how a part's run is dealt over its waves, which
// workgroup of the linear grid is which (part, column block), and where a partial accumulator register lands in the stream's scratch block.
// The kernel, its launcher, the planner (gemm_plan.cpp) and a CPU test (tests/test_skinny_f32_split_cpu.py) all include this file. Nothing
// here needs a device: it compiles with any C++14 host compiler.
//
// The S_all = br * skf_steps(k) steps of a call, numbered as in the unsplit kernel, go to P_eff = min(P, S_all) parts in contiguous runs
// (the first S_all % P_eff parts take one step more); a part's run goes to skf_waves(run length) waves exactly as a whole call's steps do.
// blocks * P_eff workgroups: blockIdx.x = part * blocks + block, so workgroups that start together share a k range - A's bytes.
#pragma once
#include "brgemm_f32_skinny.h"

namespace tpp {

constexpr int SKFS_PMAX = 16; // most parts (= SPLIT_MAX of split_scratch.h: the launcher asserts it)

// P_eff; below 2 the call is the plain skinny launch
constexpr int skfs_parts(int P, long long s_all) { return P < s_all ? P : (int)s_all; }
// THE PARTS: part p of P_eff takes steps [first, first + count) of S_all - the formulas of the deal over waves
constexpr int skfs_part_count(int p, int P_eff, int S_all) { return skf_wave_count(p, P_eff, S_all); }
constexpr int skfs_part_first(int p, int P_eff, int S_all) { return skf_wave_first(p, P_eff, S_all); }
// THE DEAL inside a part: wave w of skf_waves(run) takes steps [first, first + count) of the CALL. The workgroups of a launch all have the
// waves of part 0 (the longest run: skfs_block_waves); a part with a shorter run leaves its last wave idle (count 0, first = the part's).
constexpr int skfs_part_waves(int p, int P_eff, int S_all) { return skf_waves(skfs_part_count(p, P_eff, S_all)); }
constexpr int skfs_block_waves(int P_eff, int S_all) { return skfs_part_waves(0, P_eff, S_all); }
constexpr int skfs_wave_count(int w, int p, int P_eff, int S_all) {
  return w < skfs_part_waves(p, P_eff, S_all) ? skf_wave_count(w, skfs_part_waves(p, P_eff, S_all), skfs_part_count(p, P_eff, S_all)) : 0;
}
constexpr int skfs_wave_first(int w, int p, int P_eff, int S_all) {
  return skfs_part_first(p, P_eff, S_all) +
         (w < skfs_part_waves(p, P_eff, S_all) ? skf_wave_first(w, skfs_part_waves(p, P_eff, S_all), skfs_part_count(p, P_eff, S_all)) : 0);
}
// THE GRID: linear, part-major
constexpr long long skfs_grid(long long blocks, int P_eff) { return blocks * P_eff; }
constexpr int skfs_grid_part(int bid, int blocks) { return bid / blocks; }
constexpr int skfs_grid_block(int bid, int blocks) { return bid % blocks; }
// THE SCRATCH: partial [block][part][s * C + j][lane] as f32x4 - MB * BN floats per (block, part), 1 KiB contiguous per wave store
// instruction. Float index of element e (0 .. 3) of accumulator register reg = s * C + j of lane l; one arrival counter per block.
constexpr long long skfs_slot_floats(int mb, int bn) { return (long long)mb * bn; }
constexpr long long skfs_floats(long long blocks, int P_eff, int mb, int bn) { return blocks * P_eff * skfs_slot_floats(mb, bn); }
constexpr long long skfs_float_index(int block, int part, int P_eff, int mb, int bn, int reg, int l, int e) {
  return ((long long)block * P_eff + part) * skfs_slot_floats(mb, bn) + (long long)reg * 256 + 4 * l + e;
}
// what the launcher refuses (the limits: split_scratch.h SPLIT_MAX_TILES, SPLIT_MAX, SPLIT_SCRATCH_FLOATS)
constexpr bool skfs_launch_fits(long long blocks, int P_eff, int mb, int bn, long long max_tiles, int max_parts, long long max_floats) {
  return P_eff >= 2 && P_eff <= max_parts && blocks >= 1 && blocks <= max_tiles && skfs_floats(blocks, P_eff, mb, bn) <= max_floats;
}

} // namespace tpp
