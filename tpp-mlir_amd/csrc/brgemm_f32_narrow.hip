// brgemm_f32_narrow.hip - narrow-output f32 layers (opt-in: xsmm_hip_set_narrow_f32): a whole-layer f32 call with m >= 32 rows and 1 .. 31
// columns - a classifier or regression head behind an f32 MLP, a 16-wide bottleneck. Such a layer is an activation stream - its time is the
// bytes of A -, so one workgroup takes ALL n columns of one block of BM = 16 / 32 / 64 rows, the grid is ceil(m / BM) workgroups, and A goes
// from global memory straight into the A-operand registers of v_mfma_f32_16x16x4_f32: no LDS on the operand path, every byte of A loaded by
// one lane, once. The maps - loads, operand selection, output, ragged-k mask, the deal of steps over waves - are brgemm_f32_narrow.h.
//   A step is 16 consecutive k of one batch element. Lane (g = l >> 4, c = l & 15) loads per row piece j ONE 16-byte piece A[row 16 j + c]
//   [k0 + 4 g .. + 3] and per column set t the four elements B[k0 + 4 g + r][16 t + c], r = 0 .. 3, of the flat B - a few KiB that every
//   workgroup re-reads from L2. MFMA r takes element r of the A piece and B element r: its k-slot g is the real k k0 + 4 g + r on both
//   sides. NB = 16 (n <= 16) is one accumulator set per row piece, NB = 32 two that share every A fragment.
//   K split inside the workgroup: the stream of steps over (batch element, k) is dealt over W = min(NRF_WMAX, steps) waves in contiguous
//   runs (W depends on br and k alone). Waves 1 .. W - 1 leave their partial accumulators in static LDS, wave 0 adds them in wave order,
//   then beta 1's C, the bias, relu: a fixed order of additions, the same bits on every run, whatever m, n or the position of the row
//   block. No cross-workgroup synchronisation, no scratch block, no counter in device memory: legal on a captured stream.
//   A row at or beyond m is read from row m - 1, a column at or beyond n from column n - 1; neither is stored. For k % 16 != 0 the lane
//   groups of the last step of a batch element whose k values do not exist load nothing and feed +0.0 on BOTH sides.
//   C is m * n elements - nothing next to A -, so a lane stores its single elements of four rows as 4-byte elements: ldc, ldb, B, the C
//   pointer and the bias pointer need their natural 4-byte alignment only.
// Each wave keeps NRF_DEPTH steps of loads in flight.
#include "gemm_common.h"
#include "brgemm_f32_narrow.h"

namespace tpp {

typedef __attribute__((address_space(1))) const char nrf_gchar;
constexpr int NRF_DEPTH = 4; // steps of loads in flight per wave

// one step of one lane: its 4 k values of one row of A per row piece, and of one column of B per column set
template <int BM, int NB> struct NrfStep {
  f32x4 a[BM / 16];
  float b[NB / 16][4];
};
// (a struct, not a bare array: brgemm_bf16_skinny_tile.h SknAcc says why)
template <int BM, int NB> struct NrfAcc {
  f32x4 v[BM / 16][NB / 16];
};

template <int BM, int NB> __global__ __launch_bounds__(64 * NRF_WMAX) void brgemm_f32_narrow(GemmArgs p) {
  constexpr int SM = BM / 16, SN = NB / 16, NACC = SM * SN * 4;
  __shared__ float part[(NRF_WMAX - 1) * NACC * 64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), W = blockDim.x >> 6;
  const int64_t m0 = (int64_t)blockIdx.x * BM;
  const int spb = nrf_steps(p.k), S = spb * p.br;
  const int t0 = nrf_wave_first(wave, W, S), cnt = nrf_wave_count(wave, W, S);
  const bool tail_masked = !nrf_group_kept(lane, nrf_step_klim(p.k, spb - 1)); // (never true for k % 16 == 0)

  nrf_gchar *Al[SM], *Bl[SN];
#pragma unroll
  for (int j = 0; j < SM; ++j) {
    const int64_t row = m0 + nrf_a_row(lane, j) < p.m ? m0 + nrf_a_row(lane, j) : p.m - 1; // a row at or beyond m: the last row, never stored
    Al[j] = (nrf_gchar *)p.A + 4 * (row * p.lda + nrf_a_k(lane, 0));
  }
#pragma unroll
  for (int t = 0; t < SN; ++t) // a column at or beyond n: the last column, never stored
    Bl[t] = (nrf_gchar *)p.B + 4 * ((int64_t)nrf_b_k(lane, 0) * p.ldb + nrf_clamp(nrf_b_col(lane, t), p.n));
  const int64_t row_pitch = 4 * p.ldb, step_pitch = 4 * (int64_t)NRF_KSTEP * p.ldb; // bytes: a row of B, 16 rows

  int cb = t0 / spb, cks = t0 - cb * spb; // the load cursor: batch element, step within it
  auto load = [&] __device__(NrfStep<BM, NB> &f) {
    if (cks == spb - 1 && tail_masked) {
#pragma unroll
      for (int j = 0; j < SM; ++j) f.a[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < SN; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) f.b[t][r] = 0.f;
    } else {
      const int64_t ao = 4 * ((int64_t)cb * p.stride_a + cks * NRF_KSTEP), bo = 4 * (int64_t)cb * p.stride_b + cks * step_pitch;
#pragma unroll
      for (int j = 0; j < SM; ++j) f.a[j] = *(__attribute__((address_space(1))) const f32x4 *)(Al[j] + ao);
#pragma unroll
      for (int t = 0; t < SN; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) f.b[t][r] = *(__attribute__((address_space(1))) const float *)(Bl[t] + bo + r * row_pitch);
    }
    if (++cks == spb) cks = 0, ++cb;
  };

  NrfAcc<BM, NB> acc;
#pragma unroll
  for (int j = 0; j < SM; ++j)
#pragma unroll
    for (int t = 0; t < SN; ++t) acc.v[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto compute = [&] __device__(const NrfStep<BM, NB> &f) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int t = 0; t < SN; ++t)
#pragma unroll
        for (int j = 0; j < SM; ++j)
          acc.v[j][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.a[j][nrf_mfma_a_elem(r)], f.b[t][nrf_mfma_b_load(r)], acc.v[j][t], 0, 0, 0);
  };

  // a ring of NRF_DEPTH steps: the first slots filled, a steady state that computes and refills every slot, a drain that refills only
  // while steps are left
  NrfStep<BM, NB> ring[NRF_DEPTH];
#pragma unroll
  for (int d = 0; d < NRF_DEPTH; ++d)
    if (d < cnt) load(ring[d]);
  int i = 0;
  for (; i + 2 * NRF_DEPTH <= cnt; i += NRF_DEPTH) {
#pragma unroll
    for (int d = 0; d < NRF_DEPTH; ++d) {
      compute(ring[d]);
      load(ring[d]);
    }
  }
  for (; i < cnt; i += NRF_DEPTH) {
#pragma unroll
    for (int d = 0; d < NRF_DEPTH; ++d)
      if (i + d < cnt) {
        compute(ring[d]);
        if (i + d + NRF_DEPTH < cnt) load(ring[d]);
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

  // wave 0, with the sum of all steps: beta 1's C, the bias, relu, single 4-byte elements of four rows per row piece
  const bool beta1 = !(p.ep & EP_BETA0), relu = p.ep & EP_RELU;
#pragma unroll
  for (int t = 0; t < SN; ++t) {
    const int col = nrf_out_col(t, lane);
    if (col >= p.n) continue;
    const float bias = (p.ep & EP_BIAS) ? ((const float *)p.D)[col] : 0.f;
#pragma unroll
    for (int j = 0; j < SM; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = m0 + nrf_out_row(j, lane, r);
        if (row >= p.m) continue;
        float *const dst = (float *)p.C + row * p.ldc + col;
        float v = acc.v[j][t][r];
        if (beta1) v += *dst;
        v += bias;
        if (relu) v = v > 0.f ? v : 0.f;
        *dst = v;
      }
  }
}

template <int BM> static hipError_t launch_f32_narrow_t(const GemmArgs &a, hipStream_t s) {
  const int W = nrf_waves((long long)a.br * nrf_steps(a.k));
  const dim3 grid(nrf_blocks(a.m, BM)), block(64 * W);
  if (nrf_nb(a.n) == 16) hipLaunchKernelGGL((brgemm_f32_narrow<BM, 16>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((brgemm_f32_narrow<BM, 32>), grid, block, 0, s, a);
  return hipGetLastError();
}

// A flat f32 B on row blocks of bm (gemm_plan.cpp plan_gemm_call). Refuses with hipErrorInvalidValue everything the kernel does not
// assume - the caller then runs the launch the call has with the mode off:
//   an instance; m >= 32, 1 <= n <= 31, k >= 4, k % 4 == 0, a batch element, rows, steps and k inside the offset arithmetic (nrf_shape_ok);
//   lda >= k, ldb >= n, ldc >= n, every leading dimension and stride inside the offset arithmetic and not negative (nrf_extents_ok);
//   lda and stride_a multiples of 4 elements and A 16-byte aligned - every 16-byte load of A is then naturally aligned;
//   no VNNI C, no transposed B (an f32 B has no VNNI image); a bias flag only with a bias row. B, C and the bias are read and written as 4-byte elements: their
//   natural alignment, which a float pointer has, is all that is asked (checked all the same).
hipError_t launch_f32_narrow(int bm, const GemmArgs &a, hipStream_t s) {
  if (!nrf_instance_exists(bm, nrf_nb(a.n)) || !nrf_shape_ok(a.m, a.n, a.k, a.br) || !nrf_extents_ok(a.lda, a.ldb, a.ldc, a.stride_a, a.stride_b))
    return hipErrorInvalidValue;
  if (a.lda < a.k || a.ldb < a.n || a.ldc < a.n || ((a.lda | a.stride_a) & 3) || ((uintptr_t)a.A & 15)) return hipErrorInvalidValue;
  if ((a.ep & EP_VNNI_C) || a.b_trans) return hipErrorInvalidValue;
  if ((((uintptr_t)a.B | (uintptr_t)a.C) & 3) || ((a.ep & EP_BIAS) && (!a.D || ((uintptr_t)a.D & 3)))) return hipErrorInvalidValue;
  return bm == 16 ? launch_f32_narrow_t<16>(a, s) : bm == 32 ? launch_f32_narrow_t<32>(a, s) : launch_f32_narrow_t<64>(a, s);
}

} // namespace tpp
