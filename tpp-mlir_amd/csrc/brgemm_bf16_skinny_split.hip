// brgemm_bf16_skinny_split.hip - the skinny-batch bf16 kernel (brgemm_bf16_skinny.hip) with its K range split ACROSS workgroups (opt-in:
// xsmm_hip_set_skinny_split, a refinement of xsmm_hip_set_skinny_bf16). The unsplit kernel gives a layer ceil(n / BN) workgroups, too few
// to keep enough bytes of B in flight; here P_eff = min(P, steps) workgroups share a column block, each streaming a contiguous run of the
// call's 32-k steps (the maps: brgemm_bf16_skinny_split.h, walked on a CPU by tests/test_skinny_split_map.py). Grid blocks * P_eff, linear,
// part-major: workgroups that start together share a k range, and with it A's bytes.
//   Inside a part everything is the unsplit kernel's: the run dealt over skn_waves(run) waves, B straight into the MFMA operands, the
//   ragged-k mask by the step's position in its batch element, the LDS combine into wave 0 in wave order.
//   THE HAND-OFF, wave 0 alone, the one of brgemm_bf16_small.hip / brgemm_f32_lw.hip (split_scratch.h): the partial accumulators parked
//   with write-through 16-byte stores in the stream's scratch block, s_waitcnt vmcnt(0), ONE relaxed agent-scope fetch_add on the block's
//   arrival counter; every workgroup but the last arriver ends there. The last arriver - whichever it is - resets the counter, loads ALL
//   P_eff partials (its own included) past the caches and adds them in part order 0 .. P_eff - 1, then runs the unsplit epilogue: ownership
//   skip, beta 1's C, bias, relu, ONE rounding. Nobody waits for anybody: no spin, no fence, no co-residency assumed. An element's chain
//   of additions depends on br, k and P_eff alone - the same bits on every run, whatever m, n, the block's position or the arrival order.
// The K loop, the combine, the epilogue and the instance switch are the unsplit kernel's: brgemm_bf16_skinny_tile.h.
#include "brgemm_bf16_skinny_tile.h"
#include "brgemm_bf16_skinny_split.h"
#include "split_scratch.h"

namespace tpp {

static_assert(SKS_PMAX == SPLIT_MAX, "the planner's most parts is the scratch block's");

typedef __attribute__((address_space(1))) unsigned int sks_gu32;

template <int IMG, int BN, int MB> __global__ __launch_bounds__(64 * SKN_WMAX) void brgemm_bf16_skinny_split(GemmArgs p) {
  constexpr int C = skn_cols(BN), SETS = MB / 16, REGS = SETS * C;
  constexpr int NACC = REGS * 4;
  __shared__ float part[(SKN_WMAX - 1) * NACC * 64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int blocks = skn_blocks(p.n, BN), P_eff = p.split;
  const int prt = sks_grid_part((int)blockIdx.x, blocks), blk = (int)blockIdx.x - prt * blocks;
  const int n0 = skn_origin(blk, p.n, BN);
  const int S_all = skn_steps(p.k) * p.br;
  const int Wp = skn_waves(sks_part_count(prt, P_eff, S_all)); // the waves of this part that have steps: blockDim.x / 64 or one fewer
  SknAcc<BN, MB> acc;
  skn_k_loop<IMG, BN, MB>(p, lane, n0, sks_wave_first(wave, prt, P_eff, S_all), sks_wave_count(wave, prt, P_eff, S_all), acc);
  skn_combine<BN, MB>(part, lane, wave, Wp, acc); // the part's waves into wave 0
  if (wave > 0) return;

  // the hand-off (wave 0): park the part's sum at sks_float_index - [block][part][register][lane] f32x4, 1 KiB per store instruction -,
  // arrive, and only the last arriver goes on
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc((void *)(p.scratch + (size_t)blk * P_eff * (MB * BN)), 0, 0x7fffffff, 0x00020000);
  const unsigned vo = (unsigned)(lane * 16);
#pragma unroll
  for (int s = 0; s < SETS; ++s)
#pragma unroll
    for (int j = 0; j < C; ++j)
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc.v[s][j]), rs, vo, (unsigned)((prt * REGS + s * C + j) * 1024), 16);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  unsigned arrived = 0;
  if (lane == 0) arrived = __hip_atomic_fetch_add((sks_gu32 *)(p.split_cnt + blk), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  arrived = __builtin_amdgcn_readfirstlane(arrived);
  if (arrived != (unsigned)(P_eff - 1)) return;
  if (lane == 0) __hip_atomic_store((sks_gu32 *)(p.split_cnt + blk), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // ALL partials, this workgroup's own included, in part order: the bits do not depend on who arrived last
#pragma unroll
  for (int s = 0; s < SETS; ++s)
#pragma unroll
    for (int j = 0; j < C; ++j)
      acc.v[s][j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, vo, (unsigned)((s * C + j) * 1024), 16));
  for (int q = 1; q < P_eff; ++q)
#pragma unroll
    for (int s = 0; s < SETS; ++s)
#pragma unroll
      for (int j = 0; j < C; ++j)
        acc.v[s][j] += __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, vo, (unsigned)((q * REGS + s * C + j) * 1024), 16));

  skn_epilogue<BN, MB>(p, lane, blk, n0, acc);
}

template <int IMG, int BN> static hipError_t launch_bf16_skinny_split_t(const GemmArgs &a, int blocks, hipStream_t s) {
  const dim3 grid(sks_grid(blocks, a.split)), block(64 * sks_block_waves(a.split, a.br * skn_steps(a.k)));
  if (skn_mb(a.m) == 16) hipLaunchKernelGGL((brgemm_bf16_skinny_split<IMG, BN, 16>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((brgemm_bf16_skinny_split<IMG, BN, 32>), grid, block, 0, s, a);
  return hipGetLastError();
}

bool bf16_skinny_args_ok(int b_kind, int bn, const GemmArgs &a); // brgemm_bf16_skinny.hip

// launch_bf16_skinny's call over `parts` = P_eff workgroups per column block (gemm_plan.cpp plan_gemm_call: 2 <= parts <= steps).
// Refuses with hipErrorInvalidValue what launch_bf16_skinny refuses, and a launch the stream's scratch block cannot hold: more column
// blocks than arrival counters (SPLIT_MAX_TILES), more parts than SPLIT_MAX, more partial floats than a block has, or no block at all (no
// memory, a 17th stream, a stream being captured) - the caller then runs the UNSPLIT skinny launch of the same bn.
hipError_t launch_bf16_skinny_split(int b_kind, int bn, int parts, const GemmArgs &a, hipStream_t s) {
  if (!bf16_skinny_args_ok(b_kind, bn, a)) return hipErrorInvalidValue;
  const int blocks = skn_blocks(a.n, bn), mb = skn_mb(a.m);
  if (parts > (long long)a.br * skn_steps(a.k) || !sks_launch_fits(blocks, parts, mb, bn, SPLIT_MAX_TILES, SPLIT_MAX, (long long)SPLIT_SCRATCH_FLOATS))
    return hipErrorInvalidValue;
  const SplitScratch *sc = split_scratch_for(s, blocks, sks_floats(blocks, parts, mb, bn));
  if (!sc) return hipErrorInvalidValue;
  GemmArgs args = a;
  args.split = parts;
  args.scratch = sc->partial;
  args.split_cnt = sc->cnt;
  return skn_for_instance(b_kind, bn, [&](auto i) { return launch_bf16_skinny_split_t<decltype(i)::IMG, decltype(i)::BN>(args, blocks, s); });
}

} // namespace tpp
