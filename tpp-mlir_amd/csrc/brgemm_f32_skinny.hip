// brgemm_f32_skinny.hip - skinny-batch f32 layers (opt-in: xsmm_hip_set_skinny_f32): a whole-layer f32 call with 1 .. 31 rows. Such a
// layer is a weight stream - its time is the bytes of B -, so one workgroup takes ALL rows of one block of BN = 16 / 32 / 64 columns, the
// grid is ceil(n / BN) workgroups, and the flat B goes from global memory straight into the operand registers of v_mfma_f32_16x16x4_f32:
// no LDS on the B path, every byte of B loaded by exactly one lane, once. The maps - load, operand selection, output, ragged-k mask, column
// blocks, the deal of steps over waves - are brgemm_f32_skinny.h, walked on a CPU by tests/test_skinny_f32_cpu.py.
//   A step is 16 consecutive k of one batch element. Lane (g = l >> 4, c = l & 15) loads rows k0 + 4 g + r, r = 0 .. 3, of B, each C = BN /
//   16 floats wide (one 4-, 8- or 16-byte load), and per accumulator set ONE 16-byte piece A[row][k0 + 4 g .. + 3]. MFMA (r, j) takes
//   B[r][j] and element r of the A piece: its k-slot g is the real k k0 + 4 g + r on both sides, and it accumulates into column j of the
//   lane, the matrix column n0 + C c + j. MB = 32 runs two accumulator sets on every B register.
//   K split inside the workgroup: the stream of steps over (batch element, k) is dealt over W = min(SKF_WMAX, steps) waves in contiguous
//   runs (W depends on br and k alone). Waves 1 .. W - 1 leave their partial accumulators in static LDS, wave 0 adds them in wave order,
//   then beta 1's C, the bias, relu: a fixed order of additions, the same bits on every run, whatever m, n or the position of the column
//   block. No cross-workgroup synchronisation of any kind - no counter, no scratch block, no spin: legal on a captured stream.
//   Rows at or beyond m are read from row m - 1 and never stored. For k % 16 != 0 the lane groups of the last step of a batch element
//   whose k values do not exist load nothing and feed +0.0 on BOTH sides. The last column block is shifted back to end at n and stores
//   only the columns no other block owns.
// Each wave keeps SKF_DEPTH steps of loads in flight.
#include "gemm_common.h"
#include "brgemm_f32_skinny.h"

namespace tpp {

typedef __attribute__((address_space(1))) const char skf_gchar;
typedef float skf_f32x2 __attribute__((ext_vector_type(2)));
constexpr int SKF_DEPTH = 4; // steps of loads in flight per wave

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
template <int BN, int MB>
__device__ __forceinline__ void skf_k_loop(const GemmArgs &p, const int lane, const int n0, const int t0, const int cnt, SkfAcc<BN, MB> &acc) {
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
      for (int s = 0; s < SETS; ++s)
        f.a[s] = *(__attribute__((address_space(1))) const f32x4 *)(Al[s] + 4 * ((int64_t)cb * p.stride_a + cks * SKF_KSTEP));
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
#pragma unroll
  for (int d = 0; d < SKF_DEPTH; ++d)
    if (d < cnt) load(ring[d]);
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

template <int BN, int MB> __global__ __launch_bounds__(64 * SKF_WMAX) void brgemm_f32_skinny(GemmArgs p) {
  constexpr int C = skf_cols(BN), SETS = MB / 16;
  constexpr int NACC = SETS * C * 4;
  __shared__ float part[(SKF_WMAX - 1) * NACC * 64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), W = blockDim.x >> 6;
  const int blk = blockIdx.x;
  const int n0 = skf_origin(blk, p.n, BN);
  const int S = skf_steps(p.k) * p.br;
  SkfAcc<BN, MB> acc;
  skf_k_loop<BN, MB>(p, lane, n0, skf_wave_first(wave, W, S), skf_wave_count(wave, W, S), acc);

  // the partial accumulators through LDS, added by wave 0 in wave order: ONE barrier, a fixed order of additions
  if (wave > 0) {
#pragma unroll
    for (int s = 0; s < SETS; ++s)
#pragma unroll
      for (int j = 0; j < C; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[((wave - 1) * NACC + (s * C + j) * 4 + r) * 64 + lane] = acc.v[s][j][r];
  }
  __syncthreads();
  if (wave > 0) return;
  for (int w = 1; w < W; ++w)
#pragma unroll
    for (int s = 0; s < SETS; ++s)
#pragma unroll
      for (int j = 0; j < C; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc.v[s][j][r] += part[((w - 1) * NACC + (s * C + j) * 4 + r) * 64 + lane];

  // wave 0, with the sum of all steps: a lane holds columns n0 + C l15 .. + C - 1 of rows 16 s + 4 g + r - one piece of 4 C bytes per row.
  // The ownership skip of a shifted last block, beta 1's C, the bias, relu.
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
      if (beta1) skf_load_piece<C>(h, (skf_gchar *)dst);
#pragma unroll
      for (int j = 0; j < C; ++j) {
        float v = acc.v[s][j][r];
        if (beta1) v += h[j];
        if (p.ep & EP_BIAS) v += bias[j];
        if (relu) v = v > 0.f ? v : 0.f;
        h[j] = v;
      }
      skf_store_piece<C>(dst, h);
    }
}

template <int BN> static hipError_t launch_f32_skinny_t(const GemmArgs &a, hipStream_t s) {
  const int W = skf_waves((long long)a.br * skf_steps(a.k));
  const dim3 grid(skf_blocks(a.n, BN)), block(64 * W);
  if (skf_mb(a.m) == 16) hipLaunchKernelGGL((brgemm_f32_skinny<BN, 16>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((brgemm_f32_skinny<BN, 32>), grid, block, 0, s, a);
  return hipGetLastError();
}

// A flat f32 B on column blocks of bn (gemm_plan.cpp plan_gemm_call). Refuses with hipErrorInvalidValue everything the kernel does not
// assume - the caller then runs the launch the call has with the mode off:
//   bn 16 / 32 / 64; 1 <= m <= 31, n >= bn, n % 4 == 0, k >= 4, k % 4 == 0, a batch element (skf_shape_ok); lda >= k, ldb >= n, ldc >= n;
//   lda, ldb, ldc, stride_a and stride_b multiples of 4 elements and not negative; A, B, C and the bias row 16-byte aligned - every load of
//   A (16 bytes), of a row piece of B or the bias (4 .. 16 bytes) and every piece of C is then naturally aligned -; no VNNI operand, no
//   transposed B.
hipError_t launch_f32_skinny(int bn, const GemmArgs &a, hipStream_t s) {
  if (!skf_shape_ok(a.m, a.n, a.k, a.br, bn) || a.b_trans || (a.ep & EP_VNNI_C)) return hipErrorInvalidValue;
  if (a.lda < a.k || a.ldb < a.n || a.ldc < a.n || ((a.lda | a.ldb | a.ldc | a.stride_a | a.stride_b) & 3) || a.stride_a < 0 || a.stride_b < 0) return hipErrorInvalidValue;
  if ((((uintptr_t)a.A | (uintptr_t)a.B | (uintptr_t)a.C) & 15) || ((a.ep & EP_BIAS) && (!a.D || ((uintptr_t)a.D & 15)))) return hipErrorInvalidValue;
  return bn == 16 ? launch_f32_skinny_t<16>(a, s) : bn == 32 ? launch_f32_skinny_t<32>(a, s) : launch_f32_skinny_t<64>(a, s);
}

} // namespace tpp
