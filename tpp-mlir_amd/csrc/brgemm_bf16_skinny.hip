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
// The K loop, the combine, the epilogue and the instance switch are brgemm_bf16_skinny_tile.h, shared with the split kernel.
#include "brgemm_bf16_skinny_tile.h"

namespace tpp {

template <int IMG, int BN, int MB> __global__ __launch_bounds__(64 * SKN_WMAX) void brgemm_bf16_skinny(GemmArgs p) {
  constexpr int C = skn_cols(BN), SETS = MB / 16;
  constexpr int NACC = SETS * C * 4;
  __shared__ float part[(SKN_WMAX - 1) * NACC * 64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), W = blockDim.x >> 6;
  const int blk = blockIdx.x;
  const int n0 = skn_origin(blk, p.n, BN);
  const int S = skn_steps(p.k) * p.br;
  SknAcc<BN, MB> acc;
  skn_k_loop<IMG, BN, MB>(p, lane, n0, skn_wave_first(wave, W, S), skn_wave_count(wave, W, S), acc);
  skn_combine<BN, MB>(part, lane, wave, W, acc);
  if (wave > 0) return;
  skn_epilogue<BN, MB>(p, lane, blk, n0, acc);
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
  return skn_for_instance(b_kind, bn, [&](auto i) { return launch_bf16_skinny_t<decltype(i)::IMG, decltype(i)::BN>(a, s); });
}

} // namespace tpp
