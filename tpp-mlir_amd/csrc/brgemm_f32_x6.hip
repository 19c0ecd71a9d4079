// brgemm_f32_x6.hip - f32-in / f32-out batch-reduce GEMM on the bf16 MFMA: the bf16x6 split (opt-in, xsmm_hip_set_f32_precision(6) /
// TPP_HIP_F32_PRECISION=bf16x6).
//
// Numerics. Every f32 operand is written as a = hi + mid + lo, three bf16 parts rounded to nearest-even one after another
// (hi = bf16(a), mid = bf16(a - hi), lo = bf16(a - hi - mid); both differences are exact in f32), which leaves |a - hi - mid - lo| of
// about 2^-27 |a|. Of the nine part products the six down to order 2^-18 |a b| are formed - hi.lo, lo.hi, mid.mid, hi.mid, mid.hi,
// hi.hi, in that order, small terms first - on v_mfma_f32_32x32x16_bf16 into ONE f32 accumulator per output element; the three
// dropped ones (mid.lo, lo.mid, lo.lo) are about 2^-26 relative, below the f32 rounding of the accumulation itself. A k-step of 16 then
// costs 6 x 32 MFMA cycles against 8 x 64 on v_mfma_f32_32x32x2_f32. The summation order is fixed (chunk by chunk, k-steps in order,
// the six products in the order above, K groups summed in group order): results are bit-reproducible run to run.
// Special values: a finite a above the bf16 range must not round hi to infinity - it is rounded toward zero instead (the rest goes to
// mid / lo as for any other value); a non-finite hi (inf, NaN) gets mid = lo = 0, else inf - inf would turn it into a NaN. That is not
// enough for the OUTPUT: an infinite a still meets b's mid and lo parts in hi.mid / hi.lo, and those are 0 (inf x 0 = NaN) whenever b
// is exactly a bf16 value, or of the opposite sign to b's hi (inf - inf). Finite operands large enough that a part product overflows
// do the same (hi.hi = +inf, hi.mid = -inf). So the loaders track the largest |a| and |b| they split, and a workgroup whose panels
// held an inf or a NaN, or whose max |a| max |b| reaches 2^126, computes its tile again with an f32 fma loop in k order: non-finite
// outputs then sit where the exact path puts them, NaN stays NaN; other tiles never take that path. Subnormal lo parts (|a| below
// ~2^-110) lose bits below 2^-133, far under the element-wise bar's floor: not special-cased.
//
// Structure: one workgroup per output tile of BM x BN = 32 WM x 32 WN. WM * WN * WK MFMA waves, each one 32x32 accumulator and 1 / WK
// of every 64-k chunk's k-steps: they only read bf16 fragments from LDS and issue MFMAs. NL LOADER waves do all the global loads and
// the split: in chunk t they split chunk t + 1 (loaded during chunk t - 1) into the free slot of a two-slot LDS ring and request
// chunk t + 2 into their registers. One barrier per chunk. Split (vector ALU) and MFMA then run on different waves of the same SIMD,
// which the SIMD issues side by side. The three bf16 planes of A are [row][k], those of B transposed to [col][k] (the k-contiguous
// 8-element runs both MFMA operands read). Planes are 128-byte rows of 8 16-byte pieces, piece index XOR (row & 7): the ds_read_b128 of 8 consecutive rows of one
// piece hit 8 different bank groups. Epilogue of the f32 family: beta 0 / 1, bias (bcast_col_in0), relu, write-through C stores.
#include "gemm_common.h"
#include "xsmm_desc.h"

namespace tpp {

constexpr int X6_BK = 64; // k per chunk
constexpr int X6_LOADERS = 4; // loader (split) waves per workgroup
typedef __bf16 x6_bf16x2 __attribute__((ext_vector_type(2)));
typedef float x6_f32x2 __attribute__((ext_vector_type(2)));

// RNE, NaN -> quiet NaN (the oracle's recipe); a finite value above the bf16 range is rounded toward zero
__device__ __forceinline__ unsigned x6_hi_bits_safe(float f) {
  const unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
  if ((u & 0x7fffffffu) == 0x7f800000u) return u >> 16;
  const unsigned r = (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
  return (r & 0x7fffu) == 0x7f80u ? u >> 16 : r;
}
__device__ __forceinline__ unsigned x6_rne_bits(float f) { // finite, in range
  const unsigned u = __float_as_uint(f);
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

// split 8 values into the three bf16 planes (one 16-byte piece each). safe = false: every |v| < 2^127 (no overflow, no inf / NaN):
// the hardware's packed RNE conversion (v_cvt_pk_bf16_f32), five vector instructions per value and part pair
__device__ __forceinline__ void x6_split8(const float *v, bool safe, u32x4 &h, u32x4 &m, u32x4 &l) {
  if (!safe) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const x6_f32x2 a = {v[2 * j], v[2 * j + 1]};
      const unsigned hp = __builtin_bit_cast(unsigned, __builtin_convertvector(a, x6_bf16x2));
      const x6_f32x2 r = {a[0] - __uint_as_float(hp << 16), a[1] - __uint_as_float(hp & 0xffff0000u)};
      const unsigned mp = __builtin_bit_cast(unsigned, __builtin_convertvector(r, x6_bf16x2));
      const x6_f32x2 s = {r[0] - __uint_as_float(mp << 16), r[1] - __uint_as_float(mp & 0xffff0000u)};
      const unsigned lp = __builtin_bit_cast(unsigned, __builtin_convertvector(s, x6_bf16x2));
      h[j] = hp, m[j] = mp, l[j] = lp;
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    unsigned hh[2], mm[2], ll[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const float a = v[2 * j + e];
      hh[e] = x6_hi_bits_safe(a);
      const float hf = __uint_as_float(hh[e] << 16);
      if ((hh[e] & 0x7f80u) == 0x7f80u) { // hi is inf or NaN: the value is carried by hi alone
        mm[e] = ll[e] = 0;
      } else {
        const float r = a - hf;
        mm[e] = x6_rne_bits(r);
        ll[e] = x6_rne_bits(r - __uint_as_float(mm[e] << 16));
      }
    }
    h[j] = hh[0] | (hh[1] << 16), m[j] = mm[0] | (mm[1] << 16), l[j] = ll[0] | (ll[1] << 16);
  }
}

constexpr unsigned X6_BIG = 0x7f000000u; // |v| bits from here on (|v| >= 2^127, inf, NaN): the software split
template <int WM, int WN, int WK, int NL, bool VEC>
__global__ __launch_bounds__(64 * (WM * WN * WK + NL)) void brgemm_f32_x6(GemmArgs p) {
  constexpr int NMW = WM * WN * WK, NT = 64 * (NMW + NL), LT = 64 * NL, BM = 32 * WM, BN = 32 * WN;
  constexpr int PA = BM * X6_BK * 2, PB = BN * X6_BK * 2; // bytes of one bf16 plane of A / B
  constexpr int SLOT = 3 * (PA + PB);
  constexpr int UA = BM * 8, UB = 4 * BN;            // loader units: A = one row x 8 k, B = 8 k x 2 columns
  constexpr int NUA = (UA + LT - 1) / LT, NUB = (UB + LT - 1) / LT; // per loader thread
  constexpr int KS = 4 / WK;                         // k-steps of 16 per wave and chunk
  static_assert(KS >= 1 && 4 % WK == 0, "K groups");
  extern __shared__ __attribute__((aligned(16))) char smem_x6[];
  __shared__ unsigned x6_mag[2]; // the largest |a| / |b| bits the loaders split (special values, overflow: the fma fallback below)

  // the NL loader waves are the first hardware waves (their first loads go out before the MFMA waves start); role index of an MFMA wave
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool loader = wave < NL;
  const int mw = loader ? 0 : wave - NL;
  const int wm = mw % WM, wn = (mw / WM) % WN, wk = mw / (WM * WN);
  const int m0 = (int)blockIdx.y * BM, n0 = (int)blockIdx.x * BN;
  const int kchunks = p.k / X6_BK, T = p.br * kchunks;
  const float *__restrict__ A = (const float *)p.A + (int64_t)m0 * p.lda;
  const float *__restrict__ B = (const float *)p.B + n0;

  float ra[NUA][8], rb[NUB][16];
  unsigned magA = 0, magB = 0; // largest |a| / |b| bits this loader thread split
  auto load = [&](int t) {
    const int b = t / kchunks, kc = t - b * kchunks;
    const float *Ac = A + (int64_t)b * p.stride_a + kc * X6_BK;
    const float *Bc = B + (int64_t)b * p.stride_b + (int64_t)(kc * X6_BK) * p.ldb;
#pragma unroll
    for (int i = 0; i < NUA; ++i) {
      const int u = tid + i * LT;
      if (UA % LT == 0 || u < UA) {
        const float *src = Ac + (int64_t)(u >> 3) * p.lda + 8 * (u & 7);
        if constexpr (VEC) {
          const f32x4 x = *(const f32x4 *)src, y = *(const f32x4 *)(src + 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) ra[i][e] = x[e], ra[i][4 + e] = y[e];
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) ra[i][e] = src[e];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NUB; ++i) {
      const int u = tid + i * LT;
      if (UB % LT == 0 || u < UB) {
        const int kg = u / (BN / 2), cp = u - kg * (BN / 2);
        const float *src = Bc + (int64_t)(8 * kg) * p.ldb + 2 * cp;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if constexpr (VEC) {
            const x6_f32x2 x = *(const x6_f32x2 *)(src + (int64_t)j * p.ldb);
            rb[i][j] = x[0], rb[i][8 + j] = x[1];
          } else {
            rb[i][j] = src[(int64_t)j * p.ldb], rb[i][8 + j] = src[(int64_t)j * p.ldb + 1];
          }
        }
      }
    }
  };
  // split the registers and write the six planes of ring slot `slot`
  auto store = [&](int slot) {
    char *base = smem_x6 + slot * SLOT;
#pragma unroll
    for (int i = 0; i < NUA; ++i) {
      const int u = tid + i * LT;
      if (UA % LT == 0 || u < UA) {
        const int row = u >> 3, pc = u & 7;
        unsigned g = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) g = max(g, __float_as_uint(ra[i][e]) & 0x7fffffffu);
        magA = max(magA, g);
        u32x4 h, m, l;
        x6_split8(ra[i], g >= X6_BIG, h, m, l);
        const int off = row * 128 + ((pc ^ (row & 7)) << 4);
        *(u32x4 *)(base + off) = h;
        *(u32x4 *)(base + PA + off) = m;
        *(u32x4 *)(base + 2 * PA + off) = l;
      }
    }
#pragma unroll
    for (int i = 0; i < NUB; ++i) {
      const int u = tid + i * LT;
      if (UB % LT == 0 || u < UB) {
        const int kg = u / (BN / 2), cp = u - kg * (BN / 2);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const int col = 2 * cp + c;
          unsigned g = 0;
#pragma unroll
          for (int e = 0; e < 8; ++e) g = max(g, __float_as_uint(rb[i][8 * c + e]) & 0x7fffffffu);
          magB = max(magB, g);
          u32x4 h, m, l;
          x6_split8(&rb[i][8 * c], g >= X6_BIG, h, m, l);
          const int off = 3 * PA + col * 128 + ((kg ^ (col & 7)) << 4);
          *(u32x4 *)(base + off) = h;
          *(u32x4 *)(base + PB + off) = m;
          *(u32x4 *)(base + 2 * PB + off) = l;
        }
      }
    }
  };

  f32x16 acc = {};
  const int fr = lane & 31, fh = lane >> 5;
  const int arow = wm * 32 + fr, bcol = wn * 32 + fr;
  auto compute = [&](int slot) {
    const char *base = smem_x6 + slot * SLOT;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int pc = 2 * (wk * KS + s) + fh; // 16-byte piece: k 8 pc .. 8 pc + 7 of the chunk
      const int oa = arow * 128 + ((pc ^ (arow & 7)) << 4), ob = 3 * PA + bcol * 128 + ((pc ^ (bcol & 7)) << 4);
      const bf16x8 ah = *(const bf16x8 *)(base + oa), am = *(const bf16x8 *)(base + PA + oa), al = *(const bf16x8 *)(base + 2 * PA + oa);
      const bf16x8 bh = *(const bf16x8 *)(base + ob), bm = *(const bf16x8 *)(base + PB + ob), bl = *(const bf16x8 *)(base + 2 * PB + ob);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
    }
  };

  if (tid == 0) x6_mag[0] = x6_mag[1] = 0;
  if (loader && T > 0) {
    load(0);
    store(0);
    if (T > 1) load(1);
  }
  __syncthreads();
  // chunk t: the MFMA waves read slot t & 1 while the loader waves split chunk t + 1 (loaded one chunk ago) into slot (t + 1) & 1 -
  // the slot the MFMA waves finished with before the previous barrier - and request chunk t + 2 into their registers
  for (int t = 0; t < T; ++t) {
    if (loader) {
      if (t + 1 < T) store((t + 1) & 1);
      if (t + 2 < T) load(t + 2);
    } else {
      compute(t & 1);
    }
    __syncthreads();
  }

  if (loader) {
    atomicMax(&x6_mag[0], magA);
    atomicMax(&x6_mag[1], magB);
  }
  __syncthreads();
  const unsigned mA = x6_mag[0], mB = x6_mag[1];
  // an inf or NaN operand, or operands large enough that a part product could overflow (max |a| max |b| >= 2^126: biased exponents
  // adding up to 379): the tile again, element by element, f32 fma in k order (see the head of the file)
  if (mA >= 0x7f800000u || mB >= 0x7f800000u || (mA >> 23) + (mB >> 23) >= 379u) {
    for (int e = tid; e < BM * BN; e += NT) {
      const int i = e / BN, j = e - i * BN;
      float v = 0.0f;
      for (int b = 0; b < p.br; ++b) {
        const float *a = A + (int64_t)b * p.stride_a + (int64_t)i * p.lda, *bb = B + (int64_t)b * p.stride_b + j;
        for (int k = 0; k < p.k; ++k) v = __builtin_fmaf(a[k], bb[(int64_t)k * p.ldb], v);
      }
      float *c = (float *)p.C + (int64_t)(m0 + i) * p.ldc + n0 + j;
      if (!(p.ep & EP_BETA0)) v += *c;
      if (p.ep & EP_BIAS) v += ((const float *)p.D)[n0 + j];
      if (p.ep & EP_RELU) v = v > 0.0f ? v : 0.0f;
      *c = v;
    }
    return;
  }
  if constexpr (WK > 1) {
    // K groups: every group parks its partial in LDS, group 0 sums them in group order
    float *red = (float *)smem_x6; // (the ring is free: every wave has passed the barrier behind the last chunk)
    if (!loader && wk > 0) {
#pragma unroll
      for (int r = 0; r < 16; ++r) red[((wk - 1) * (WM * WN) + wm + WM * wn) * 1024 + r * 64 + lane] = acc[r];
    }
    __syncthreads();
    if (loader || wk > 0) return;
#pragma unroll
    for (int g = 1; g < WK; ++g)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] += red[((g - 1) * (WM * WN) + wm + WM * wn) * 1024 + r * 64 + lane];
  }
  if (loader) return;
  // epilogue: lane = column, register r = row (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of the wave's 32x32 block
  const int col = n0 + bcol;
  float bias = 0.0f;
  if (p.ep & EP_BIAS) bias = ((const float *)p.D)[col];
  float *Ct = (float *)p.C + (int64_t)(m0 + wm * 32) * p.ldc + n0 + wn * 32;
  const __amdgpu_buffer_rsrc_t rsrcC = __builtin_amdgcn_make_buffer_rsrc((void *)Ct, 0, 0x7fffffff, 0x00020000);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * fh;
    const unsigned off = (unsigned)((row * (int)p.ldc + fr) * 4);
    float v = acc[r];
    if (!(p.ep & EP_BETA0)) v += __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrcC, off, 0, 0));
    v += bias;
    if (p.ep & EP_RELU) v = v > 0.0f ? v : 0.0f;
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsrcC, off, 0, C_STORE_AUX);
  }
}

template <int WM, int WN, int WK, bool VEC> static hipError_t launch_x6_t(const GemmArgs &a, hipStream_t s) {
  constexpr int NL = X6_LOADERS, BM = 32 * WM, BN = 32 * WN, NT = 64 * (WM * WN * WK + NL);
  constexpr size_t lds = 2 * 3 * (size_t)(BM + BN) * X6_BK * 2;
  static_assert(lds <= 160 * 1024, "LDS budget");
  static_assert(WK == 1 || (size_t)(WK - 1) * WM * WN * 4096 <= lds, "K-group partials fit in the ring");
  static std::atomic<unsigned long long> lds_set{0};
  if (hipError_t e = ensure_dynamic_lds((const void *)brgemm_f32_x6<WM, WN, WK, NL, VEC>, (int)lds, lds_set); e != hipSuccess) return e;
  if (a.n / BN > 65535 || a.m / BM > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL((brgemm_f32_x6<WM, WN, WK, NL, VEC>), dim3(a.n / BN, a.m / BM), dim3(NT), lds, s, a);
  return hipGetLastError();
}

// tile: 0 = 64x64, 1 = 64x32 + K2, 2 = 32x32 + K4, 3 = 128x64. vec: A and B 16-byte aligned (ld / strides are multiples of 4: plan_gemm)
hipError_t launch_f32_x6(int tile, const GemmArgs &a, bool vec, hipStream_t s) {
  switch (tile) {
  case 0: return vec ? launch_x6_t<2, 2, 1, true>(a, s) : launch_x6_t<2, 2, 1, false>(a, s);
  case 1: return vec ? launch_x6_t<2, 1, 2, true>(a, s) : launch_x6_t<2, 1, 2, false>(a, s);
  case 2: return vec ? launch_x6_t<1, 1, 4, true>(a, s) : launch_x6_t<1, 1, 4, false>(a, s);
  case 3: return vec ? launch_x6_t<4, 2, 1, true>(a, s) : launch_x6_t<4, 2, 1, false>(a, s);
  default: return hipErrorInvalidValue;
  }
}

} // namespace tpp
