// brgemm_bf16_skinny_tile.h - the skinny-batch bf16 tile (1 .. 31 rows on a block of BN = 16 / 32 / 64 columns), written ONCE for the two
// kernels built from it: brgemm_bf16_skinny.hip (a call) and brgemm_bf16_skinny_split.hip (a call with its K range split across
// workgroups). The split's contract is "inside a part everything is the unsplit kernel's": it runs this text, not a copy of it. Device
// code and the launchers' instance switch; the maps it walks are brgemm_bf16_skinny.h (host-only, tests/test_skinny_map.py).
//   skn_k_loop        a wave's run of 32-k steps into its accumulators: B from global memory straight into the MFMA operands
//   skn_combine       the waves' partial accumulators through LDS into wave 0, in wave order
//   skn_epilogue      ownership skip, beta 1's C, bias, relu, ONE rounding to bf16, the store
//   skn_for_instance  (b_kind, bn) -> <IMG, BN>
// brgemm_bf16_skinny_chain.hip (a chain of such layers in one launch) keeps a text of its own: built from this tile its forced BN 64
// launches measured 2 .. 4 % slower, cause not found (profiles/skinny_tile_refactor_ab.txt, part 4). Its results must stay bit for bit
// this tile's: change the two together.
#pragma once
#include "gemm_common.h"
#include "brgemm_bf16_skinny.h"

namespace tpp {

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

// the accumulators of one wave: v[s][j] = rows 16 s .. 16 s + 15 of the lane's j-th column. A struct on purpose: handed from function to
// function as a bare array f32x4[SETS][C], the compiler's alloca promotion takes the whole array for ONE vector of up to 32 floats before
// the loops over it are unrolled - 8 .. 16 VGPRs more, a register copy of every accumulator in front of the combine, an occupancy step
// lost in several instances (profiles/skinny_tile_refactor_isa.txt). It leaves a struct alone, and the unrolled loops then split it.
template <int BN, int MB> struct SknAcc {
  f32x4 v[MB / 16][BN / 16];
};

// Steps t0 .. t0 + cnt - 1 of the stream of 32-k steps (numbered batch element by batch element) of the column block at n0, into acc
// (zeroed here); cnt may be 0.
//   Rows at or beyond m are CLAMPED: read from row m - 1 and never stored.
//   RAGGED k (k % 32 != 0): in the last step of a batch element the lane groups whose k values do not exist load nothing and feed zeros
//   on BOTH sides - a product of a stray B with a zero A could still be a NaN.
//   Each wave keeps SKN_DEPTH steps of loads in flight, B then A of a step, the mask tested once per step.
template <int IMG, int BN, int MB>
__device__ __forceinline__ void skn_k_loop(const GemmArgs &p, const int lane, const int n0, const int t0, const int cnt, SknAcc<BN, MB> &acc) {
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
    for (int j = 0; j < C; ++j) acc.v[s][j] = f32x4{0.f, 0.f, 0.f, 0.f};

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
        acc.v[s][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(skn_bf16x8, f.a[s]), __builtin_bit_cast(skn_bf16x8, bj), acc.v[s][j], 0, 0, 0);
    }
  };

  // a ring of SKN_DEPTH steps: the first slots filled, a steady state that computes and refills every slot, a drain that refills only
  // while steps are left
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
  for (; i < cnt; i += SKN_DEPTH) { // drain
#pragma unroll
    for (int d = 0; d < SKN_DEPTH; ++d)
      if (i + d < cnt) {
        compute(ring[d]);
        if (i + d + SKN_DEPTH < cnt) load(ring[d]);
      }
  }
}

// The partial accumulators through LDS, added by wave 0 in wave order: waves 1 .. W - 1 park theirs in part[] ((SKN_WMAX - 1) * NACC * 64
// floats), ONE barrier, wave 0 adds them as w = 1 .. W - 1 - a fixed order of additions. Every wave of the workgroup calls this (a wave at
// or beyond W parks nothing). What follows differs by kernel and stays there: who returns, and whether part[] is needed again.
template <int BN, int MB>
__device__ __forceinline__ void skn_combine(float *part, const int lane, const int wave, const int W, SknAcc<BN, MB> &acc) {
  constexpr int C = skn_cols(BN), SETS = MB / 16, NACC = SETS * C * 4;
  if (wave > 0 && wave < W) {
#pragma unroll
    for (int s = 0; s < SETS; ++s)
#pragma unroll
      for (int j = 0; j < C; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[((wave - 1) * NACC + (s * C + j) * 4 + r) * 64 + lane] = acc.v[s][j][r];
  }
  __syncthreads();
  if (wave == 0)
    for (int w = 1; w < W; ++w)
#pragma unroll
      for (int s = 0; s < SETS; ++s)
#pragma unroll
        for (int j = 0; j < C; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc.v[s][j][r] += part[((w - 1) * NACC + (s * C + j) * 4 + r) * 64 + lane];
}

// a lane's piece of C bf16 values (2 / 4 / 8 bytes, naturally aligned) of a row of the bias or of C
template <int C> __device__ __forceinline__ void skn_load_piece(unsigned short (&h)[C], const unsigned short *src) {
  if constexpr (C == 1) h[0] = *src;
  else if constexpr (C == 2) {
    const uint32_t v = *(const uint32_t *)src;
    h[0] = (unsigned short)v, h[1] = (unsigned short)(v >> 16);
  } else {
    const uint2 v = *(const uint2 *)src;
    h[0] = (unsigned short)v.x, h[1] = (unsigned short)(v.x >> 16), h[2] = (unsigned short)v.y, h[3] = (unsigned short)(v.y >> 16);
  }
}

// Wave 0, with the sum of all steps in acc: a lane holds columns n0 + C l15 .. + C - 1 of rows 16 s + 4 g + r - one piece of 2 C bytes per
// row. The ownership skip of a shifted last block, beta 1's C, the bias, relu and ONE rounding to bf16.
template <int BN, int MB>
__device__ __forceinline__ void skn_epilogue(const GemmArgs &p, const int lane, const int blk, const int n0, const SknAcc<BN, MB> &acc) {
  constexpr int C = skn_cols(BN), SETS = MB / 16;
  const int col = skn_out_col(BN, lane, 0);
  if (col < skn_skip(blk, p.n, BN)) return; // the block in front owns these columns
  float bias[C];
#pragma unroll
  for (int j = 0; j < C; ++j) bias[j] = 0.f;
  if (p.ep & EP_BIAS) {
    unsigned short h[C];
    skn_load_piece<C>(h, (const unsigned short *)p.D + n0 + col);
#pragma unroll
    for (int j = 0; j < C; ++j) bias[j] = bf16_bits_to_f32(h[j]);
  }
  // what no row changes, read once: the flags, and the lane's piece of row 0
  const bool beta1 = !(p.ep & EP_BETA0), relu = p.ep & EP_RELU;
  unsigned short *const c0 = (unsigned short *)p.C + n0 + col;
#pragma unroll
  for (int s = 0; s < SETS; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = skn_out_row(s, lane, r);
      if (row >= p.m) continue;
      unsigned short *const dst = c0 + (int64_t)row * p.ldc;
      unsigned short h[C];
      if (beta1) skn_load_piece<C>(h, dst);
#pragma unroll
      for (int j = 0; j < C; ++j) {
        float v = acc.v[s][j][r];
        if (beta1) v += bf16_bits_to_f32(h[j]);
        v += bias[j];
        if (relu) v = v > 0.f ? v : 0.f;
        h[j] = f32_to_bf16_bits(v);
      }
      if constexpr (C == 1) *dst = h[0];
      else if constexpr (C == 2) *(uint32_t *)dst = (uint32_t)h[0] | ((uint32_t)h[1] << 16);
      else *(uint2 *)dst = uint2{(uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16)};
    }
}

// the instance table, once: B image b_kind (0 VNNI-2, 2 flat, 4 VNNI-4) on column blocks of bn -> f(SknInstance<IMG, BN>()); a pair
// that has no instance (skn_instance_exists) is hipErrorInvalidValue
template <int IMG_, int BN_> struct SknInstance {
  static constexpr int IMG = IMG_, BN = BN_;
};
template <typename F> static hipError_t skn_for_instance(const int b_kind, const int bn, F &&f) {
  switch (b_kind * 100 + bn) {
  case 16: return f(SknInstance<0, 16>());
  case 32: return f(SknInstance<0, 32>());
  case 64: return f(SknInstance<0, 64>());
  case 232: return f(SknInstance<2, 32>());
  case 264: return f(SknInstance<2, 64>());
  case 416: return f(SknInstance<4, 16>());
  case 432: return f(SknInstance<4, 32>());
  case 464: return f(SknInstance<4, 64>());
  }
  return hipErrorInvalidValue;
}

} // namespace tpp
