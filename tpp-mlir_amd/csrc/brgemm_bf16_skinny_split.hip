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
// The K loop and the epilogue below are the unsplit kernel's text, kept here as a copy: moved into a shared header they compiled the
// unsplit kernels to other instructions (register allocation, scheduling), and those stay the measured ones.
#include "gemm_common.h"
#include "brgemm_bf16_skinny_split.h"
#include "split_scratch.h"

namespace tpp {

static_assert(SKS_PMAX == SPLIT_MAX, "the planner's most parts is the scratch block's");

typedef __bf16 skn_bf16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(1))) const char skn_gchar;
typedef unsigned int skn_u32x2 __attribute__((ext_vector_type(2)));
constexpr int SKN_DEPTH = 4; // steps of loads in flight per wave

template <int P> __device__ __forceinline__ void skn_load_row(uint32_t (&d)[P], skn_gchar *p) {
  if constexpr (P == 1) {
    d[0] = *(__attribute__((address_space(1))) const uint32_t *)p;
  } else if constexpr (P == 2) {
    const skn_u32x2 v = *(__attribute__((address_space(1))) const skn_u32x2 *)p;
    d[0] = v.x, d[1] = v.y;
  } else {
#pragma unroll
    for (int q = 0; q < P / 4; ++q) {
      const u32x4 v = ((__attribute__((address_space(1))) const u32x4 *)p)[q];
      d[4 * q] = v.x, d[4 * q + 1] = v.y, d[4 * q + 2] = v.z, d[4 * q + 3] = v.w;
    }
  }
}

// one step of one lane: its R x P dwords of B and its 8 k values of one row of A per accumulator set
template <int IMG, int BN, int MB> struct SknStep {
  uint32_t b[skn_rows(IMG)][skn_dwords(IMG, BN)];
  u32x4 a[MB / 16];
};

// steps t0 .. t0 + cnt - 1 of the call's stream (numbered batch element by batch element) of the column block at n0, into acc (zeroed here)
template <int IMG, int BN, int MB>
__device__ __forceinline__ void skn_k_loop(const GemmArgs &p, const int lane, const int n0, const int t0, const int cnt, f32x4 (&acc)[MB / 16][BN / 16]) {
  constexpr int C = skn_cols(BN), R = skn_rows(IMG), P = skn_dwords(IMG, BN), SETS = MB / 16, VF = skn_vfac(IMG);
  const int g = lane >> 4, l15 = lane & 15;
  const int spb = skn_steps(p.k);
  const int klast = skn_step_klim(p.k, spb - 1); // k values of the last step of a batch element: 8 .. 32
  const bool tail_masked = !skn_group_kept(lane, klast);

  const int64_t row_pitch = 2 * VF * p.ldb, step_pitch = 2 * (int64_t)SKN_KSTEP * p.ldb; // bytes: an image row, 32 k values of any image
  skn_gchar *const Bl = (skn_gchar *)p.B + skn_load_byte(IMG, BN, lane, 0, p.ldb) + 2 * VF * (int64_t)n0;
  skn_gchar *Al[SETS];
#pragma unroll
  for (int s = 0; s < SETS; ++s) {
    const int row = 16 * s + l15 < p.m ? 16 * s + l15 : p.m - 1; // a row at or beyond m: read from the last row, never stored
    Al[s] = (skn_gchar *)p.A + 2 * ((int64_t)row * p.lda + 8 * g);
  }
  // the load cursor: batch element, step within it
  int cb = t0 / spb, cks = t0 - cb * spb;

  auto load = [&] __device__(SknStep<IMG, BN, MB> &f) {
    if (cks == spb - 1 && tail_masked) { // (never true for k % 32 == 0)
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int q = 0; q < P; ++q) f.b[r][q] = 0;
#pragma unroll
      for (int s = 0; s < SETS; ++s) f.a[s] = u32x4{0, 0, 0, 0};
    } else {
      skn_gchar *pb = Bl + 2 * (int64_t)cb * p.stride_b + (int64_t)cks * step_pitch;
#pragma unroll
      for (int r = 0; r < R; ++r) skn_load_row<P>(f.b[r], pb + r * row_pitch);
#pragma unroll
      for (int s = 0; s < SETS; ++s)
        f.a[s] = *(__attribute__((address_space(1))) const u32x4 *)(Al[s] + 2 * ((int64_t)cb * p.stride_a + cks * SKN_KSTEP));
    }
    if (++cks == spb) cks = 0, ++cb;
  };

#pragma unroll
  for (int s = 0; s < SETS; ++s)
#pragma unroll
    for (int j = 0; j < C; ++j) acc[s][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto compute = [&] __device__(const SknStep<IMG, BN, MB> &f) {
#pragma unroll
    for (int j = 0; j < C; ++j) {
      u32x4 bj;
#pragma unroll
      for (int q = 0; q < 4; ++q) { // dword q of the operand: k = 8 g + 2 q (low half), + 1 (high half)
        const SknSrc lo = skn_frag_src(IMG, j, 2 * q), hi = skn_frag_src(IMG, j, 2 * q + 1);
        const uint32_t x = f.b[lo.row][lo.dword], y = f.b[hi.row][hi.dword];
        bj[q] = (lo.half ? x >> 16 : x & 0xffffu) | (hi.half ? y & 0xffff0000u : y << 16);
      }
#pragma unroll
      for (int s = 0; s < SETS; ++s)
        acc[s][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(skn_bf16x8, f.a[s]), __builtin_bit_cast(skn_bf16x8, bj), acc[s][j], 0, 0, 0);
    }
  };

  SknStep<IMG, BN, MB> ring[SKN_DEPTH];
#pragma unroll
  for (int d = 0; d < SKN_DEPTH; ++d)
    if (d < cnt) load(ring[d]);
  int i = 0;
  for (; i + 2 * SKN_DEPTH <= cnt; i += SKN_DEPTH) { // steady state: every slot is computed and refilled
#pragma unroll
    for (int d = 0; d < SKN_DEPTH; ++d) {
      compute(ring[d]);
      load(ring[d]);
    }
  }
  for (; i < cnt; i += SKN_DEPTH) {
#pragma unroll
    for (int d = 0; d < SKN_DEPTH; ++d)
      if (i + d < cnt) {
        compute(ring[d]);
        if (i + d + SKN_DEPTH < cnt) load(ring[d]);
      }
  }
}

// wave 0, with the sum of the call's steps in acc: a lane holds columns n0 + C l15 .. + C - 1 of rows 16 s + 4 g + r - one piece of 2 C bytes
// per row. The ownership skip of a shifted last block, beta 1's C, the bias, relu and ONE rounding to bf16.
template <int BN, int MB>
__device__ __forceinline__ void skn_epilogue(const GemmArgs &p, const int lane, const int blk, const int n0, const f32x4 (&acc)[MB / 16][BN / 16]) {
  constexpr int C = skn_cols(BN), SETS = MB / 16;
  const int col = skn_out_col(BN, lane, 0);
  if (col < skn_skip(blk, p.n, BN)) return; // the block in front owns these columns
  float bias[C];
#pragma unroll
  for (int j = 0; j < C; ++j) bias[j] = 0.f;
  if (p.ep & EP_BIAS) {
    unsigned short h[C];
    const unsigned short *src = (const unsigned short *)p.D + n0 + col;
    if constexpr (C == 1) h[0] = *src;
    else if constexpr (C == 2) {
      const uint32_t v = *(const uint32_t *)src;
      h[0] = (unsigned short)v, h[1] = (unsigned short)(v >> 16);
    } else {
      const uint2 v = *(const uint2 *)src;
      h[0] = (unsigned short)v.x, h[1] = (unsigned short)(v.x >> 16), h[2] = (unsigned short)v.y, h[3] = (unsigned short)(v.y >> 16);
    }
#pragma unroll
    for (int j = 0; j < C; ++j) bias[j] = bf16_bits_to_f32(h[j]);
  }
#pragma unroll
  for (int s = 0; s < SETS; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = skn_out_row(s, lane, r);
      if (row >= p.m) continue;
      unsigned short *dst = (unsigned short *)p.C + (int64_t)row * p.ldc + n0 + col;
      unsigned short h[C];
      if (!(p.ep & EP_BETA0)) {
        if constexpr (C == 1) h[0] = *dst;
        else if constexpr (C == 2) {
          const uint32_t v = *(const uint32_t *)dst;
          h[0] = (unsigned short)v, h[1] = (unsigned short)(v >> 16);
        } else {
          const uint2 v = *(const uint2 *)dst;
          h[0] = (unsigned short)v.x, h[1] = (unsigned short)(v.x >> 16), h[2] = (unsigned short)v.y, h[3] = (unsigned short)(v.y >> 16);
        }
      }
#pragma unroll
      for (int j = 0; j < C; ++j) {
        float v = acc[s][j][r];
        if (!(p.ep & EP_BETA0)) v += bf16_bits_to_f32(h[j]);
        v += bias[j];
        if (p.ep & EP_RELU) v = v > 0.f ? v : 0.f;
        h[j] = f32_to_bf16_bits(v);
      }
      if constexpr (C == 1) *dst = h[0];
      else if constexpr (C == 2) *(uint32_t *)dst = (uint32_t)h[0] | ((uint32_t)h[1] << 16);
      else *(uint2 *)dst = uint2{(uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16)};
    }
}

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
  f32x4 acc[SETS][C];
  skn_k_loop<IMG, BN, MB>(p, lane, n0, sks_wave_first(wave, prt, P_eff, S_all), sks_wave_count(wave, prt, P_eff, S_all), acc);

  // the partial accumulators of the part's waves through LDS, added by wave 0 in wave order
  if (wave > 0 && wave < Wp) {
#pragma unroll
    for (int s = 0; s < SETS; ++s)
#pragma unroll
      for (int j = 0; j < C; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[((wave - 1) * NACC + (s * C + j) * 4 + r) * 64 + lane] = acc[s][j][r];
  }
  __syncthreads();
  if (wave > 0) return;
  for (int w = 1; w < Wp; ++w)
#pragma unroll
    for (int s = 0; s < SETS; ++s)
#pragma unroll
      for (int j = 0; j < C; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[s][j][r] += part[((w - 1) * NACC + (s * C + j) * 4 + r) * 64 + lane];

  // the hand-off (wave 0): park the part's sum at sks_float_index - [block][part][register][lane] f32x4, 1 KiB per store instruction -,
  // arrive, and only the last arriver goes on
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc((void *)(p.scratch + (size_t)blk * P_eff * (MB * BN)), 0, 0x7fffffff, 0x00020000);
  const unsigned vo = (unsigned)(lane * 16);
#pragma unroll
  for (int s = 0; s < SETS; ++s)
#pragma unroll
    for (int j = 0; j < C; ++j)
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[s][j]), rs, vo, (unsigned)((prt * REGS + s * C + j) * 1024), 16);
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
      acc[s][j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, vo, (unsigned)((s * C + j) * 1024), 16));
  for (int q = 1; q < P_eff; ++q)
#pragma unroll
    for (int s = 0; s < SETS; ++s)
#pragma unroll
      for (int j = 0; j < C; ++j)
        acc[s][j] += __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, vo, (unsigned)((q * REGS + s * C + j) * 1024), 16));

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
  switch (b_kind * 100 + bn) {
  case 16: return launch_bf16_skinny_split_t<0, 16>(args, blocks, s);
  case 32: return launch_bf16_skinny_split_t<0, 32>(args, blocks, s);
  case 64: return launch_bf16_skinny_split_t<0, 64>(args, blocks, s);
  case 232: return launch_bf16_skinny_split_t<2, 32>(args, blocks, s);
  case 264: return launch_bf16_skinny_split_t<2, 64>(args, blocks, s);
  case 416: return launch_bf16_skinny_split_t<4, 16>(args, blocks, s);
  case 432: return launch_bf16_skinny_split_t<4, 32>(args, blocks, s);
  case 464: return launch_bf16_skinny_split_t<4, 64>(args, blocks, s);
  }
  return hipErrorInvalidValue;
}

} // namespace tpp
