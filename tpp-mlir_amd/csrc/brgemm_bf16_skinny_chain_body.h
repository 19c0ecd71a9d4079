// brgemm_bf16_skinny_chain_body.h - the text of a skinny-batch bf16 layer chain's block: the K loop with the consumer's side of the seam, the
// epilogue with write-through stores, and how the chain kernels read their argument block. Moved here as it stood from
// brgemm_bf16_skinny_chain.hip, which shares it with brgemm_bf16_skinny_chain_split.hip (the former's header says why the chains have a text of
// their own beside brgemm_bf16_skinny_tile.h; the two must stay bit for bit the same). Device code only.
#pragma once
#include "gemm_common.h"
#include "chain_args.h"
#include "brgemm_bf16_skinny_chain.h"

namespace tpp {

typedef __bf16 skn_bf16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(1))) const char skn_gchar;
typedef unsigned int skn_u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) unsigned int skc_gu32;
// the argument block, read where it lies (kernarg segment): the layer table is indexed at run time (brgemm_bf16_lw.hip chain_kernarg_t)
typedef const __attribute__((address_space(4))) ChainArgs skc_kernarg_t;
constexpr int SKN_DEPTH = 4; // steps of loads in flight per wave
constexpr int SKC_SC1 = 16;  // aux of a raw buffer access: sc1

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

// one layer's operands and shape, as the single call's GemmArgs has them
struct SkcLayer {
  const void *A, *B, *D;
  void *C;
  int64_t lda, ldb, ldc, stride_a, stride_b;
  int m, n, k, br, ep;
};

// the seam wait of a consumer: wave 0 polls, everybody meets the barrier (the file's header)
__device__ __forceinline__ void skc_seam_wait(const unsigned *cnt, unsigned target, unsigned *err, int layer, int wave, int lane) {
  if (wave == 0) {
    skc_gu32 *c = (skc_gu32 *)cnt;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    for (;;) {
      const unsigned v = __hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((int)(v - target) >= 0) break;
      if (__builtin_amdgcn_s_memrealtime() - t0 > CHAIN_TIMEOUT_TICKS) { // never hang the GPU: flag it and go on
        if (lane == 0) __hip_atomic_store((skc_gu32 *)err, 1u + (unsigned)layer, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
  }
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); // (no instruction: the A loads below stay behind the poll)
}

// steps t0 .. t0 + cnt - 1 of the layer's stream (numbered batch element by batch element) of the column block at n0, into acc (zeroed
// here). HANDED: A is a predecessor's output of this launch - sc1 buffer loads -, and with `wait` the seam wait stands between the B loads
// and the A loads of the first ring slots. Every wave of the workgroup calls this, one with cnt = 0 included (the barrier of the wait).
template <int IMG, int BN, int MB, bool HANDED>
__device__ __forceinline__ void skc_k_loop(const SkcLayer &p, const int lane, const int wave, const int n0, const int t0, const int cnt, const bool wait,
                                           const unsigned *seam, const unsigned target, unsigned *err, const int layer,
                                           f32x4 (&acc)[MB / 16][BN / 16]) {
  constexpr int C = skn_cols(BN), R = skn_rows(IMG), P = skn_dwords(IMG, BN), SETS = MB / 16, VF = skn_vfac(IMG);
  const int g = lane >> 4, l15 = lane & 15;
  const int spb = skn_steps(p.k);
  const int klast = skn_step_klim(p.k, spb - 1); // k values of the last step of a batch element: 8 .. 32
  const bool tail_masked = !skn_group_kept(lane, klast);

  const int64_t row_pitch = 2 * VF * p.ldb, step_pitch = 2 * (int64_t)SKN_KSTEP * p.ldb; // bytes: an image row, 32 k values of any image
  skn_gchar *const Bl = (skn_gchar *)p.B + skn_load_byte(IMG, BN, lane, 0, p.ldb) + 2 * VF * (int64_t)n0;
  skn_gchar *Al[SETS];
  unsigned Ao[SETS]; // HANDED: the lane's byte offset into the buffer of A (below 2^30: skc_ld_ok)
#pragma unroll
  for (int s = 0; s < SETS; ++s) {
    const int row = 16 * s + l15 < p.m ? 16 * s + l15 : p.m - 1; // a row at or beyond m: read from the last row, never stored
    Al[s] = (skn_gchar *)p.A + 2 * ((int64_t)row * p.lda + 8 * g);
    Ao[s] = (unsigned)(2 * (row * (int)p.lda + 8 * g));
  }
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void *)p.A, 0, 0x7fffffff, 0x00020000);

  auto load_b = [&] __device__(SknStep<IMG, BN, MB> &f, const int cb, const int cks) {
    if (cks == spb - 1 && tail_masked) { // (never true for k % 32 == 0)
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int q = 0; q < P; ++q) f.b[r][q] = 0;
    } else {
      skn_gchar *pb = Bl + 2 * (int64_t)cb * p.stride_b + (int64_t)cks * step_pitch;
#pragma unroll
      for (int r = 0; r < R; ++r) skn_load_row<P>(f.b[r], pb + r * row_pitch);
    }
  };
  auto load_a = [&] __device__(SknStep<IMG, BN, MB> &f, const int cb, const int cks) {
    if (cks == spb - 1 && tail_masked) {
#pragma unroll
      for (int s = 0; s < SETS; ++s) f.a[s] = u32x4{0, 0, 0, 0};
    } else if constexpr (HANDED) {
      const unsigned so = (unsigned)(2 * (cb * (int)p.stride_a + cks * SKN_KSTEP)); // (inside the row: below 2 lda)
#pragma unroll
      for (int s = 0; s < SETS; ++s) f.a[s] = __builtin_amdgcn_raw_buffer_load_b128(rsA, Ao[s], so, SKC_SC1);
    } else {
#pragma unroll
      for (int s = 0; s < SETS; ++s)
        f.a[s] = *(__attribute__((address_space(1))) const u32x4 *)(Al[s] + 2 * ((int64_t)cb * p.stride_a + cks * SKN_KSTEP));
    }
  };
  // the load cursor: batch element, step within it
  int cb = t0 / spb, cks = t0 - cb * spb;
  auto advance = [&] __device__(int &b, int &ks) {
    if (++ks == spb) ks = 0, ++b;
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
  // the first ring slots: the weights, then - behind the seam wait, where there is one - the activations
  {
    int ab = cb, aks = cks;
#pragma unroll
    for (int d = 0; d < SKN_DEPTH; ++d)
      if (d < cnt) {
        load_b(ring[d], cb, cks);
        advance(cb, cks);
      }
    if constexpr (HANDED)
      if (wait) skc_seam_wait(seam, target, err, layer, wave, lane);
#pragma unroll
    for (int d = 0; d < SKN_DEPTH; ++d)
      if (d < cnt) {
        load_a(ring[d], ab, aks);
        advance(ab, aks);
      }
  }
  int i = 0;
  for (; i + 2 * SKN_DEPTH <= cnt; i += SKN_DEPTH) { // steady state: every slot is computed and refilled
#pragma unroll
    for (int d = 0; d < SKN_DEPTH; ++d) {
      compute(ring[d]);
      load_b(ring[d], cb, cks);
      load_a(ring[d], cb, cks);
      advance(cb, cks);
    }
  }
  for (; i < cnt; i += SKN_DEPTH) {
#pragma unroll
    for (int d = 0; d < SKN_DEPTH; ++d)
      if (i + d < cnt) {
        compute(ring[d]);
        if (i + d + SKN_DEPTH < cnt) {
          load_b(ring[d], cb, cks);
          load_a(ring[d], cb, cks);
          advance(cb, cks);
        }
      }
  }
}

// wave 0, with the sum of the layer's steps in acc: a lane holds columns n0 + C l15 .. + C - 1 of rows 16 s + 4 g + r - one piece of 2 C bytes
// per row. The ownership skip of a shifted last block, the bias, relu and ONE rounding to bf16 (beta 0: the launcher takes nothing else);
// every piece leaves through a write-through store.
template <int BN, int MB>
__device__ __forceinline__ void skc_epilogue(const SkcLayer &p, const int lane, const int blk, const int n0, const f32x4 (&acc)[MB / 16][BN / 16]) {
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
  const __amdgpu_buffer_rsrc_t rsC = __builtin_amdgcn_make_buffer_rsrc(p.C, 0, 0x7fffffff, 0x00020000);
#pragma unroll
  for (int s = 0; s < SETS; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = skn_out_row(s, lane, r);
      if (row >= p.m) continue;
      const unsigned off = (unsigned)(2 * (row * (int)p.ldc + n0 + col)); // (below 2^30: skc_ld_ok)
      unsigned short h[C];
#pragma unroll
      for (int j = 0; j < C; ++j) {
        float v = acc[s][j][r];
        v += bias[j];
        if (p.ep & EP_RELU) v = v > 0.f ? v : 0.f;
        h[j] = f32_to_bf16_bits(v);
      }
      if constexpr (C == 1) __builtin_amdgcn_raw_buffer_store_b16(h[0], rsC, off, 0, SKC_SC1);
      else if constexpr (C == 2) __builtin_amdgcn_raw_buffer_store_b32((uint32_t)h[0] | ((uint32_t)h[1] << 16), rsC, off, 0, SKC_SC1);
      else
        __builtin_amdgcn_raw_buffer_store_b64(skn_u32x2{(uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16)}, rsC, off, 0,
                                              SKC_SC1);
    }
}

// the argument block's address, opaque to the compiler from here on: what is read through the result is loaded HERE, not ahead of the K
// loop in front - the layer's facts would otherwise all stay in scalar registers across it, more than there are
template <class Args> __device__ __forceinline__ Args *skc_args_again(Args *pp) {
  asm volatile("" : "+s"(pp));
  return pp;
}

} // namespace tpp
