// brgemm_bf16_narrow.hip - narrow-output bf16 layers (opt-in: xsmm_hip_set_narrow_bf16): a whole-layer call with m >= 32 rows and 1 .. 31
// columns - a classifier or regression head, a 16-wide bottleneck. Such a layer is an activation stream - its time is the bytes of A -, so
// one workgroup takes ALL n columns of one block of BM = 16 / 32 / 64 rows, the grid is ceil(m / BM) workgroups, and A goes from global
// memory straight into the A-operand registers of v_mfma_f32_16x16x32_bf16: a row of A is 8 consecutive k values per lane, one 16-byte load,
// every byte loaded by one lane, once, no LDS. B is a few KiB that every workgroup re-reads from L2 as its image stores it: four 4-byte
// pair-rows (VNNI-2), two 8-byte k-group rows (VNNI-4) or eight 2-byte elements (flat) per lane, column set and step - no selection. NB = 16
// (n <= 16) is one accumulator set per row piece, NB = 32 two that share every A fragment. The maps - loads, output, ragged-k mask, the deal
// of steps over waves - are brgemm_bf16_narrow.h, walked on a CPU by tests/test_narrow_bf16_cpu.py.
//   K split inside the workgroup: the stream of 32-k steps over (batch element, k) is dealt over W = min(NRW_WMAX, steps) waves in
//   contiguous runs (W depends on br and k alone). Waves 1 .. W - 1 leave their partial accumulators in LDS, wave 0 adds them in wave
//   order, then beta 1's C, the bias, relu and ONE rounding to bf16 (the scheme of brgemm_bf16_skinny_tile.h): a fixed order of additions,
//   the same bits on every run, whatever m, n or the position of the row block. No cross-workgroup synchronisation, no scratch block, no
//   counter in device memory: legal on a captured stream.
//   A row at or beyond m is read from row m - 1, a column at or beyond n from column n - 1; neither is stored. For k % 32 != 0 the lane
//   groups of the last step of a batch element whose k values do not exist load nothing and feed zeros on BOTH sides.
//   C is m * n elements - nothing next to A -, so a lane stores its single elements of four rows as 2-byte elements: ldc, ldb, the C
//   pointer and the bias pointer need their natural 2-byte alignment only.
// Each wave keeps NRW_DEPTH steps of loads in flight.
#include "gemm_common.h"
#include "brgemm_bf16_narrow.h"

namespace tpp {

typedef __bf16 nrw_bf16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(1))) const char nrw_gchar;
typedef unsigned int nrw_u32x2 __attribute__((ext_vector_type(2)));
constexpr int NRW_DEPTH = 4; // steps of loads in flight per wave

// one step of one lane: its 8 k values of one row of A per row piece, and of one column of B per column set as the image's loads deliver
// them - whole operand dwords (VNNI), or eight zero-extended elements (flat) that compute() pairs
template <int IMG, int BM, int NB> struct NrwStep {
  u32x4 a[BM / 16];
  uint32_t b[NB / 16][IMG == 2 ? 8 : 4];
};
// (a struct, not a bare array: brgemm_bf16_skinny_tile.h SknAcc says why)
template <int BM, int NB> struct NrwAcc {
  f32x4 v[BM / 16][NB / 16];
};

template <int IMG, int BM, int NB> __global__ __launch_bounds__(64 * NRW_WMAX) void brgemm_bf16_narrow(GemmArgs p) {
  constexpr int SM = BM / 16, SN = NB / 16, VF = nrw_vfac(IMG), R = nrw_b_loads(IMG), NACC = SM * SN * 4;
  __shared__ float part[(NRW_WMAX - 1) * NACC * 64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), W = blockDim.x >> 6;
  const int g = lane >> 4;
  const int64_t m0 = (int64_t)blockIdx.x * BM;
  const int spb = nrw_steps(p.k), S = spb * p.br;
  const int t0 = nrw_wave_first(wave, W, S), cnt = nrw_wave_count(wave, W, S);
  const bool tail_masked = !nrw_group_kept(lane, nrw_step_klim(p.k, spb - 1)); // (never true for k % 32 == 0)

  nrw_gchar *Al[SM], *Bl[SN];
#pragma unroll
  for (int j = 0; j < SM; ++j) {
    const int64_t row = m0 + nrw_a_row(lane, j) < p.m ? m0 + nrw_a_row(lane, j) : p.m - 1; // a row at or beyond m: the last row, never stored
    Al[j] = (nrw_gchar *)p.A + 2 * (row * p.lda + nrw_a_k(lane));
  }
#pragma unroll
  for (int t = 0; t < SN; ++t) // a column at or beyond n: the last column, never stored
    Bl[t] = (nrw_gchar *)p.B + 2 * nrw_b_elem(IMG, 8 * g, nrw_clamp(nrw_b_col(lane, t), p.n), p.ldb);
  const int64_t row_pitch = 2 * VF * p.ldb, step_pitch = 2 * (int64_t)NRW_KSTEP * p.ldb; // bytes: an image row, 32 k values of any image

  int cb = t0 / spb, cks = t0 - cb * spb; // the load cursor: batch element, step within it
  auto load = [&] __device__(NrwStep<IMG, BM, NB> &f) {
    if (cks == spb - 1 && tail_masked) {
#pragma unroll
      for (int j = 0; j < SM; ++j) f.a[j] = u32x4{0, 0, 0, 0};
#pragma unroll
      for (int t = 0; t < SN; ++t)
#pragma unroll
        for (int q = 0; q < (IMG == 2 ? 8 : 4); ++q) f.b[t][q] = 0;
    } else {
      const int64_t ao = 2 * ((int64_t)cb * p.stride_a + cks * NRW_KSTEP), bo = 2 * (int64_t)cb * p.stride_b + cks * step_pitch;
#pragma unroll
      for (int j = 0; j < SM; ++j) f.a[j] = *(__attribute__((address_space(1))) const u32x4 *)(Al[j] + ao);
#pragma unroll
      for (int t = 0; t < SN; ++t)
#pragma unroll
        for (int r = 0; r < R; ++r) {
          nrw_gchar *src = Bl[t] + bo + r * row_pitch;
          if constexpr (IMG == 0) {
            f.b[t][r] = *(__attribute__((address_space(1))) const uint32_t *)src;
          } else if constexpr (IMG == 4) {
            const nrw_u32x2 v = *(__attribute__((address_space(1))) const nrw_u32x2 *)src;
            f.b[t][2 * r] = v.x, f.b[t][2 * r + 1] = v.y;
          } else {
            f.b[t][r] = *(__attribute__((address_space(1))) const unsigned short *)src;
          }
        }
    }
    if (++cks == spb) cks = 0, ++cb;
  };

  NrwAcc<BM, NB> acc;
#pragma unroll
  for (int j = 0; j < SM; ++j)
#pragma unroll
    for (int t = 0; t < SN; ++t) acc.v[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto compute = [&] __device__(const NrwStep<IMG, BM, NB> &f) {
#pragma unroll
    for (int t = 0; t < SN; ++t) {
      u32x4 bt;
#pragma unroll
      for (int q = 0; q < 4; ++q) bt[q] = IMG == 2 ? f.b[t][2 * q] | (f.b[t][2 * q + 1] << 16) : f.b[t][q];
#pragma unroll
      for (int j = 0; j < SM; ++j)
        acc.v[j][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(nrw_bf16x8, f.a[j]), __builtin_bit_cast(nrw_bf16x8, bt), acc.v[j][t], 0, 0, 0);
    }
  };

  // a ring of NRW_DEPTH steps: the first slots filled, a steady state that computes and refills every slot, a drain that refills only
  // while steps are left
  NrwStep<IMG, BM, NB> ring[NRW_DEPTH];
#pragma unroll
  for (int d = 0; d < NRW_DEPTH; ++d)
    if (d < cnt) load(ring[d]);
  int i = 0;
  for (; i + 2 * NRW_DEPTH <= cnt; i += NRW_DEPTH) {
#pragma unroll
    for (int d = 0; d < NRW_DEPTH; ++d) {
      compute(ring[d]);
      load(ring[d]);
    }
  }
  for (; i < cnt; i += NRW_DEPTH) {
#pragma unroll
    for (int d = 0; d < NRW_DEPTH; ++d)
      if (i + d < cnt) {
        compute(ring[d]);
        if (i + d + NRW_DEPTH < cnt) load(ring[d]);
      }
  }

  // the partial accumulators through LDS, added by wave 0 in wave order: ONE barrier, a fixed order of additions
  if (wave > 0) {
#pragma unroll
    for (int j = 0; j < SM; ++j)
#pragma unroll
      for (int t = 0; t < SN; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[((wave - 1) * NACC + (j * SN + t) * 4 + r) * 64 + lane] = acc.v[j][t][r];
  }
  __syncthreads();
  if (wave > 0) return;
  for (int w = 1; w < W; ++w)
#pragma unroll
    for (int j = 0; j < SM; ++j)
#pragma unroll
      for (int t = 0; t < SN; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc.v[j][t][r] += part[((w - 1) * NACC + (j * SN + t) * 4 + r) * 64 + lane];

  // wave 0, with the sum of all steps: beta 1's C, the bias, relu, ONE rounding to bf16, single 2-byte elements of four rows per row piece
  const bool beta1 = !(p.ep & EP_BETA0), relu = p.ep & EP_RELU;
#pragma unroll
  for (int t = 0; t < SN; ++t) {
    const int col = nrw_out_col(t, lane);
    if (col >= p.n) continue;
    const float bias = (p.ep & EP_BIAS) ? bf16_bits_to_f32(((const unsigned short *)p.D)[col]) : 0.f;
#pragma unroll
    for (int j = 0; j < SM; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = m0 + nrw_out_row(j, lane, r);
        if (row >= p.m) continue;
        unsigned short *const dst = (unsigned short *)p.C + row * p.ldc + col;
        float v = acc.v[j][t][r];
        if (beta1) v += bf16_bits_to_f32(*dst);
        v += bias;
        if (relu) v = v > 0.f ? v : 0.f;
        *dst = f32_to_bf16_bits(v);
      }
  }
}

template <int IMG, int BM> static hipError_t launch_bf16_narrow_t(const GemmArgs &a, hipStream_t s) {
  const int W = nrw_waves((long long)a.br * nrw_steps(a.k));
  const dim3 grid(nrw_blocks(a.m, BM)), block(64 * W);
  if (nrw_nb(a.n) == 16) hipLaunchKernelGGL((brgemm_bf16_narrow<IMG, BM, 16>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((brgemm_bf16_narrow<IMG, BM, 32>), grid, block, 0, s, a);
  return hipGetLastError();
}

// B image b_kind (0 VNNI-2, 2 flat, 4 VNNI-4) on row blocks of bm (gemm_plan.cpp plan_gemm_call). Refuses with hipErrorInvalidValue
// everything the kernel does not assume - the caller then runs the launch the call has with the mode off:
//   an instance; m >= 32, 1 <= n <= 31, k >= 8, k % 8 == 0, a batch element, rows, steps and k inside the offset arithmetic (nrw_shape_ok);
//   lda >= k, ldb >= n, ldc >= n, every leading dimension and stride inside the offset arithmetic and not negative (nrw_extents_ok);
//   lda and stride_a multiples of 8 elements and A 16-byte aligned - every 16-byte load of A is then naturally aligned;
//   VNNI-2: B 4-byte aligned and stride_b even; VNNI-4: B 8-byte aligned and stride_b % 4 == 0 - a pair-row / k-group row piece sits at a
//   multiple of its own size whatever ldb is; flat B, C and the bias: 2-byte elements, nothing asked; no VNNI C.
hipError_t launch_bf16_narrow(int b_kind, int bm, const GemmArgs &a, hipStream_t s) {
  if (!nrw_instance_exists(b_kind, bm, nrw_nb(a.n)) || !nrw_shape_ok(a.m, a.n, a.k, a.br) || !nrw_extents_ok(a.lda, a.ldb, a.ldc, a.stride_a, a.stride_b))
    return hipErrorInvalidValue;
  if (a.lda < a.k || a.ldb < a.n || a.ldc < a.n || ((a.lda | a.stride_a) & 7) || ((uintptr_t)a.A & 15) || (a.ep & EP_VNNI_C)) return hipErrorInvalidValue;
  const int piece = 2 * nrw_vfac(b_kind); // bytes of one load of B
  if (((uintptr_t)a.B & (piece - 1)) || (a.stride_b & (piece / 2 - 1))) return hipErrorInvalidValue;
  if ((a.ep & EP_BIAS) && !a.D) return hipErrorInvalidValue;
  switch (b_kind * 100 + bm) {
  case 16: return launch_bf16_narrow_t<0, 16>(a, s);
  case 32: return launch_bf16_narrow_t<0, 32>(a, s);
  case 64: return launch_bf16_narrow_t<0, 64>(a, s);
  case 216: return launch_bf16_narrow_t<2, 16>(a, s);
  case 232: return launch_bf16_narrow_t<2, 32>(a, s);
  case 264: return launch_bf16_narrow_t<2, 64>(a, s);
  case 416: return launch_bf16_narrow_t<4, 16>(a, s);
  case 432: return launch_bf16_narrow_t<4, 32>(a, s);
  case 464: return launch_bf16_narrow_t<4, 64>(a, s);
  }
  return hipErrorInvalidValue;
}

} // namespace tpp
