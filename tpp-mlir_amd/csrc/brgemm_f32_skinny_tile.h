// brgemm_f32_skinny_tile.h - the skinny-batch f32 tile (1 .. 31 rows on a block of BN = 16 / 32 / 64 columns), written ONCE for the two
// kernels built from it: brgemm_f32_skinny.hip (a call), brgemm_f32_skinny_split.hip (a call with its K range split across workgroups)
// and brgemm_f32_skinny_chain.hip (a chain of such layers in one launch). The split's and the chain's contract is "inside a part / a block
// everything is the unsplit kernel's": they run this text, not a copy of it. The chain's needs - handed-off A through sc1 buffer loads, the
// seam wait between the B and the A loads of the first ring slots, sc1 buffer stores - are DEFAULTED template parameters: with the
// defaults the text is what it was, and the twelve kernels of the other two files compile to the parent's instructions
// (profiles/chain_skinny_f32_isa.txt). Device code only; the maps it walks are brgemm_f32_skinny.h (host-only, tests/test_skinny_f32_cpu.py).
//   skf_k_loop    a wave's run of 16-k steps into its accumulators: B from global memory straight into the MFMA operands
//   skf_park, skf_gather  the waves' partial accumulators through LDS into wave 0, in wave order
//   skf_epilogue  ownership skip, beta 1's C, bias, relu, the store
#pragma once
#include "gemm_common.h"
#include "brgemm_f32_skinny.h"

namespace tpp {

typedef __attribute__((address_space(1))) const char skf_gchar;
typedef float skf_f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int skf_u32x2 __attribute__((ext_vector_type(2)));
constexpr int SKF_DEPTH = 4; // steps of loads in flight per wave
constexpr int SKF_SC1 = 16;  // aux of a raw buffer access: sc1 (write-through store / a load past the CU's L1)
// what a HANDED K loop calls between the B loads and the A loads of its first ring slots: every wave, once, also one without a step
struct SkfNoWait {
  __device__ __forceinline__ void operator()() const {}
};

// a lane's piece of C floats (4 / 8 / 16 bytes, naturally aligned) of a row of B, of the bias or of C
template <int C> __device__ __forceinline__ void skf_load_piece(float (&d)[C], skf_gchar *p) {
  if constexpr (C == 1) {
    d[0] = *(__attribute__((address_space(1))) const float *)p;
  } else if constexpr (C == 2) {
    const skf_f32x2 v = *(__attribute__((address_space(1))) const skf_f32x2 *)p;
    d[0] = v.x, d[1] = v.y;
  } else {
    const f32x4 v = *(__attribute__((address_space(1))) const f32x4 *)p;
    d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
  }
}
template <int C> __device__ __forceinline__ void skf_store_piece(float *dst, const float (&d)[C]) {
  if constexpr (C == 1) *dst = d[0];
  else if constexpr (C == 2) *(skf_f32x2 *)dst = skf_f32x2{d[0], d[1]};
  else *(f32x4 *)dst = f32x4{d[0], d[1], d[2], d[3]};
}

// one step of one lane: its 4 rows x C floats of B and its 4 k values of one row of A per accumulator set
template <int BN, int MB> struct SkfStep {
  float b[4][BN / 16];
  f32x4 a[MB / 16];
};
// the accumulators of one wave: v[s][j] = rows 16 s .. 16 s + 15 of the lane's j-th column (a struct: see SknAcc, brgemm_bf16_skinny_tile.h)
template <int BN, int MB> struct SkfAcc {
  f32x4 v[MB / 16][BN / 16];
};

// Steps t0 .. t0 + cnt - 1 of the stream of 16-k steps (numbered batch element by batch element) of the column block at n0, into acc
// (zeroed here); cnt may be 0. A ring of SKF_DEPTH steps: B then A of a step, the ragged-k mask tested once per step.
// HANDED (the chain, layers > 0): A is a predecessor's output of this launch - every load of it is an sc1 buffer load (byte offsets below
// 2^31: skfc_ld_ok) -, and the first ring slots load all their B, call wait() and only then load their A: weights do not depend on
// activations. The same values reach the same MFMAs in the same order either way.
template <int BN, int MB, bool HANDED = false, class Wait = SkfNoWait>
__device__ __forceinline__ void skf_k_loop(const GemmArgs &p, const int lane, const int n0, const int t0, const int cnt, SkfAcc<BN, MB> &acc,
                                           const Wait wait = Wait{}) {
  constexpr int C = skf_cols(BN), SETS = MB / 16;
  const int spb = skf_steps(p.k);
  const int klast = skf_step_klim(p.k, spb - 1); // k values of the last step of a batch element: 4 .. 16
  const bool tail_masked = !skf_group_kept(lane, klast);

  const int64_t row_pitch = 4 * p.ldb, step_pitch = 4 * (int64_t)SKF_KSTEP * p.ldb; // bytes
  skf_gchar *const Bl = (skf_gchar *)p.B + skf_load_byte(BN, lane, 0, p.ldb) + 4 * (int64_t)n0;
  skf_gchar *Al[SETS];
#pragma unroll
  for (int s = 0; s < SETS; ++s) {
    const int row = skf_a_row(s, lane) < p.m ? skf_a_row(s, lane) : p.m - 1; // a row at or beyond m: read from the last row, never stored
    Al[s] = (skf_gchar *)p.A + 4 * ((int64_t)row * p.lda + skf_a_k(lane, 0));
  }
  // HANDED: the lane's byte offset into the buffer of A, and the step's (inside the row: below 4 lda)
  auto a_off = [&] __device__(const int s) {
    const int row = skf_a_row(s, lane) < p.m ? skf_a_row(s, lane) : p.m - 1;
    return (unsigned)(4 * (row * (int)p.lda + skf_a_k(lane, 0)));
  };
  auto a_step = [&] __device__(const int b, const int ks) { return (unsigned)(4 * (b * (int)p.stride_a + ks * SKF_KSTEP)); };

  // the load cursor: batch element, step within it
  int cb = t0 / spb, cks = t0 - cb * spb;

  auto load = [&] __device__(SkfStep<BN, MB> &f) {
    if (cks == spb - 1 && tail_masked) { // (never true for k % 16 == 0)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int j = 0; j < C; ++j) f.b[r][j] = 0.f;
#pragma unroll
      for (int s = 0; s < SETS; ++s) f.a[s] = f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
      skf_gchar *pb = Bl + 4 * (int64_t)cb * p.stride_b + (int64_t)cks * step_pitch;
#pragma unroll
      for (int r = 0; r < 4; ++r) skf_load_piece<C>(f.b[r], pb + r * row_pitch);
#pragma unroll
      for (int s = 0; s < SETS; ++s) {
        if constexpr (HANDED) {
          const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void *)p.A, 0, 0x7fffffff, 0x00020000);
          f.a[s] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsA, a_off(s), a_step(cb, cks), SKF_SC1));
        } else {
          f.a[s] = *(__attribute__((address_space(1))) const f32x4 *)(Al[s] + 4 * ((int64_t)cb * p.stride_a + cks * SKF_KSTEP));
        }
      }
    }
    if (++cks == spb) cks = 0, ++cb;
  };

#pragma unroll
  for (int s = 0; s < SETS; ++s)
#pragma unroll
    for (int j = 0; j < C; ++j) acc.v[s][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto compute = [&] __device__(const SkfStep<BN, MB> &f) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int j = 0; j < C; ++j)
#pragma unroll
        for (int s = 0; s < SETS; ++s)
          acc.v[s][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.a[s][skf_mfma_a_elem(r, j)], f.b[skf_mfma_b_row(r, j)][skf_mfma_b_elem(r, j)], acc.v[s][j], 0, 0, 0);
  };

  // the first slots filled, a steady state that computes and refills every slot, a drain that refills only while steps are left
  SkfStep<BN, MB> ring[SKF_DEPTH];
  if constexpr (HANDED) { // the first slots in two halves around the wait: the step's B or zeros, then its A or zeros
    int ab = cb, aks = cks;
#pragma unroll
    for (int d = 0; d < SKF_DEPTH; ++d)
      if (d < cnt) {
        const bool masked = cks == spb - 1 && tail_masked;
        skf_gchar *pb = Bl + 4 * (int64_t)cb * p.stride_b + (int64_t)cks * step_pitch;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (masked) {
#pragma unroll
            for (int j = 0; j < C; ++j) ring[d].b[r][j] = 0.f;
          } else skf_load_piece<C>(ring[d].b[r], pb + r * row_pitch);
        }
        if (++cks == spb) cks = 0, ++cb;
      }
    wait();
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void *)p.A, 0, 0x7fffffff, 0x00020000);
#pragma unroll
    for (int d = 0; d < SKF_DEPTH; ++d)
      if (d < cnt) {
        const bool masked = aks == spb - 1 && tail_masked;
#pragma unroll
        for (int s = 0; s < SETS; ++s)
          ring[d].a[s] = masked ? f32x4{0.f, 0.f, 0.f, 0.f} : __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsA, a_off(s), a_step(ab, aks), SKF_SC1));
        if (++aks == spb) aks = 0, ++ab;
      }
  } else {
#pragma unroll
    for (int d = 0; d < SKF_DEPTH; ++d)
      if (d < cnt) load(ring[d]);
  }
  int i = 0;
  for (; i + 2 * SKF_DEPTH <= cnt; i += SKF_DEPTH) {
#pragma unroll
    for (int d = 0; d < SKF_DEPTH; ++d) {
      compute(ring[d]);
      load(ring[d]);
    }
  }
  for (; i < cnt; i += SKF_DEPTH) {
#pragma unroll
    for (int d = 0; d < SKF_DEPTH; ++d)
      if (i + d < cnt) {
        compute(ring[d]);
        if (i + d + SKF_DEPTH < cnt) load(ring[d]);
      }
  }
}

// The partial accumulators through LDS, added by wave 0 in wave order - the combine, in two halves around the kernel's "every wave but
// wave 0 ends here". skf_park: waves 1 .. leave theirs in part[] ((SKF_WMAX - 1) * NACC * 64 floats), then ONE barrier; every wave of the
// workgroup calls it (a wave of the split kernel that had no steps parks its zeros, which nobody reads). skf_gather: wave 0 adds the
// partials of waves 1 .. W - 1 in that order - a fixed order of additions.
template <int BN, int MB> __device__ __forceinline__ void skf_park(float *part, const int lane, const int wave, const SkfAcc<BN, MB> &acc) {
  constexpr int C = skf_cols(BN), SETS = MB / 16, NACC = SETS * C * 4;
  if (wave > 0) {
#pragma unroll
    for (int s = 0; s < SETS; ++s)
#pragma unroll
      for (int j = 0; j < C; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[((wave - 1) * NACC + (s * C + j) * 4 + r) * 64 + lane] = acc.v[s][j][r];
  }
  __syncthreads();
}
template <int BN, int MB> __device__ __forceinline__ void skf_gather(const float *part, const int lane, const int W, SkfAcc<BN, MB> &acc) {
  constexpr int C = skf_cols(BN), SETS = MB / 16, NACC = SETS * C * 4;
  for (int w = 1; w < W; ++w)
#pragma unroll
    for (int s = 0; s < SETS; ++s)
#pragma unroll
      for (int j = 0; j < C; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc.v[s][j][r] += part[((w - 1) * NACC + (s * C + j) * 4 + r) * 64 + lane];
}

// Wave 0, with the sum of all steps in acc: a lane holds columns n0 + C l15 .. + C - 1 of rows 16 s + 4 g + r - one piece of 4 C bytes per
// row. The ownership skip of a shifted last block, beta 1's C, the bias, relu. SC1 (the chain; beta 0 only, its launcher's refusal): every
// piece leaves through a write-through raw buffer store (byte offsets below 2^31: skfc_ld_ok).
template <int BN, int MB, bool SC1 = false>
__device__ __forceinline__ void skf_epilogue(const GemmArgs &p, const int lane, const int blk, const int n0, const SkfAcc<BN, MB> &acc) {
  constexpr int C = skf_cols(BN), SETS = MB / 16;
  const int col = skf_out_col(BN, lane, 0);
  if (col < skf_skip(blk, p.n, BN)) return; // the block in front owns these columns
  float bias[C];
#pragma unroll
  for (int j = 0; j < C; ++j) bias[j] = 0.f;
  if (p.ep & EP_BIAS) skf_load_piece<C>(bias, (skf_gchar *)((const float *)p.D + n0 + col));
  const bool beta1 = !(p.ep & EP_BETA0), relu = p.ep & EP_RELU;
  float *const c0 = (float *)p.C + n0 + col;
#pragma unroll
  for (int s = 0; s < SETS; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = skf_out_row(s, lane, r);
      if (row >= p.m) continue;
      float *const dst = c0 + (int64_t)row * p.ldc;
      float h[C];
      if constexpr (!SC1)
        if (beta1) skf_load_piece<C>(h, (skf_gchar *)dst);
#pragma unroll
      for (int j = 0; j < C; ++j) {
        float v = acc.v[s][j][r];
        if constexpr (!SC1)
          if (beta1) v += h[j];
        if (p.ep & EP_BIAS) v += bias[j];
        if (relu) v = v > 0.f ? v : 0.f;
        h[j] = v;
      }
      if constexpr (SC1) {
        const __amdgpu_buffer_rsrc_t rsC = __builtin_amdgcn_make_buffer_rsrc(p.C, 0, 0x7fffffff, 0x00020000);
        const unsigned off = (unsigned)(4 * (row * (int)p.ldc + n0 + col));
        if constexpr (C == 1) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, h[0]), rsC, off, 0, SKF_SC1);
        else if constexpr (C == 2) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(skf_u32x2, skf_f32x2{h[0], h[1]}), rsC, off, 0, SKF_SC1);
        else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, f32x4{h[0], h[1], h[2], h[3]}), rsC, off, 0, SKF_SC1);
      } else {
        skf_store_piece<C>(dst, h);
      }
    }
}

} // namespace tpp
