// brgemm_bf16_skinny.hip - skinny-batch bf16 layers (opt-in: xsmm_hip_set_skinny_bf16): a whole-layer call with 1 .. 31 rows. Such a layer
// is a weight stream - its time is the bytes of B -, so one workgroup takes ALL rows of one block of BN = 16 / 32 / 64 columns, the grid is
// ceil(n / BN) workgroups, and B goes from global memory straight into the operand registers of v_mfma_f32_16x16x32_bf16: no LDS on the B
// path, the k dimension is where the MFMA wants it in all three images, and the width of a lane's row piece decides BN. The maps - load,
// fragment selection, output, ragged-k mask, column blocks, the deal of steps over waves - are brgemm_bf16_skinny.h, walked on a CPU by
// tests/test_skinny_map.py.
//   K split inside the workgroup: the stream of 32-k steps over (batch element, k) is dealt over W = min(SKN_WMAX, steps) waves in
//   contiguous runs (W depends on br and k alone). Waves 1 .. W - 1 leave their partial accumulators in LDS, wave 0 adds them in wave
//   order, then beta 1's C, the bias, relu and ONE rounding to bf16: a fixed order of additions, the same bits on every run, whatever m, n
//   or the position of the column block. No cross-workgroup synchronisation of any kind: legal on a captured stream.
//   Rows at or beyond m are read from row m - 1 and never stored. For k % 32 != 0 the lane groups of the last step of a batch element
//   whose k values do not exist load nothing and feed zeros on BOTH sides. The last column block is shifted back to end at n and stores
//   only the columns no other block owns.
// Each wave keeps SKN_DEPTH steps of loads in flight.
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

template <int IMG, int BN, int MB> __global__ __launch_bounds__(64 * SKN_WMAX) void brgemm_bf16_skinny(GemmArgs p) {
  constexpr int C = skn_cols(BN), R = skn_rows(IMG), P = skn_dwords(IMG, BN), SETS = MB / 16, VF = skn_vfac(IMG);
  constexpr int NACC = SETS * C * 4;
  __shared__ float part[(SKN_WMAX - 1) * NACC * 64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), W = blockDim.x >> 6;
  const int g = lane >> 4, l15 = lane & 15;
  const int blk = blockIdx.x;
  const int n0 = skn_origin(blk, p.n, BN);
  const int spb = skn_steps(p.k), S = spb * p.br;
  const int klast = skn_step_klim(p.k, spb - 1); // k values of the last step of a batch element: 8 .. 32
  const bool tail_masked = !skn_group_kept(lane, klast);
  const int cnt = skn_wave_count(wave, W, S);
  const int t0 = skn_wave_first(wave, W, S);

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

  f32x4 acc[SETS][C];
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

  // the partial accumulators through LDS, added by wave 0 in wave order
  if (wave > 0) {
#pragma unroll
    for (int s = 0; s < SETS; ++s)
#pragma unroll
      for (int j = 0; j < C; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[((wave - 1) * NACC + (s * C + j) * 4 + r) * 64 + lane] = acc[s][j][r];
  }
  __syncthreads();
  if (wave > 0) return;
  for (int w = 1; w < W; ++w)
#pragma unroll
    for (int s = 0; s < SETS; ++s)
#pragma unroll
      for (int j = 0; j < C; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[s][j][r] += part[((w - 1) * NACC + (s * C + j) * 4 + r) * 64 + lane];

  // epilogue: a lane holds columns n0 + C l15 .. + C - 1 of rows 16 s + 4 g + r - one piece of 2 C bytes per row
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

template <int IMG, int BN> static hipError_t launch_bf16_skinny_t(const GemmArgs &a, hipStream_t s) {
  const int W = skn_waves((long long)a.br * skn_steps(a.k));
  const dim3 grid(skn_blocks(a.n, BN)), block(64 * W);
  if (skn_mb(a.m) == 16) hipLaunchKernelGGL((brgemm_bf16_skinny<IMG, BN, 16>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((brgemm_bf16_skinny<IMG, BN, 32>), grid, block, 0, s, a);
  return hipGetLastError();
}

// B image b_kind (0 VNNI-2, 2 flat, 4 VNNI-4) on column blocks of bn (gemm_plan.cpp plan_gemm_call). Refuses with hipErrorInvalidValue
// everything the kernel does not assume - the caller then runs the launch the call has with the mode off:
//   an instance (not flat with bn = 16); 1 <= m <= 31, n >= bn, n % 8 == 0, k >= 8, k % 8 == 0, a batch element (skn_shape_ok);
//   lda >= k, ldb >= n, ldc >= n; lda, ldb, ldc, stride_a and stride_b multiples of 8 elements; A, B and C 16-byte aligned - every load of A
//   (16 bytes), of a row piece of B (4 .. 16 bytes) and every piece of C (2 .. 8 bytes) is then naturally aligned -; the bias row 8-byte
//   aligned (pieces of 2 .. 8 bytes at multiples of 8 columns); no VNNI C.
// (bf16_skinny_args_ok: the same answer for the split launcher, brgemm_bf16_skinny_split.hip)
bool bf16_skinny_args_ok(int b_kind, int bn, const GemmArgs &a) {
  if (!skn_instance_exists(b_kind, bn) || !skn_shape_ok(a.m, a.n, a.k, a.br, bn)) return false;
  if (a.lda < a.k || a.ldb < a.n || a.ldc < a.n || ((a.lda | a.ldb | a.ldc | a.stride_a | a.stride_b) & 7) || a.stride_a < 0 || a.stride_b < 0) return false;
  return !((((uintptr_t)a.A | (uintptr_t)a.B | (uintptr_t)a.C) & 15) || ((a.ep & EP_BIAS) && (!a.D || ((uintptr_t)a.D & 7))) || (a.ep & EP_VNNI_C));
}
hipError_t launch_bf16_skinny(int b_kind, int bn, const GemmArgs &a, hipStream_t s) {
  if (!bf16_skinny_args_ok(b_kind, bn, a)) return hipErrorInvalidValue;
  switch (b_kind * 100 + bn) {
  case 16: return launch_bf16_skinny_t<0, 16>(a, s);
  case 32: return launch_bf16_skinny_t<0, 32>(a, s);
  case 64: return launch_bf16_skinny_t<0, 64>(a, s);
  case 232: return launch_bf16_skinny_t<2, 32>(a, s);
  case 264: return launch_bf16_skinny_t<2, 64>(a, s);
  case 416: return launch_bf16_skinny_t<4, 16>(a, s);
  case 432: return launch_bf16_skinny_t<4, 32>(a, s);
  case 464: return launch_bf16_skinny_t<4, 64>(a, s);
  }
  return hipErrorInvalidValue;
}

} // namespace tpp
