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
// The K loop, the combine and the epilogue are brgemm_f32_skinny_tile.h, shared with brgemm_f32_skinny_split.hip.
#include "brgemm_f32_skinny_tile.h"

namespace tpp {

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

  skf_park<BN, MB>(part, lane, wave, acc); // ONE barrier
  if (wave > 0) return;
  skf_gather<BN, MB>(part, lane, W, acc); // a fixed order of additions
  skf_epilogue<BN, MB>(p, lane, blk, n0, acc);
}

template <int BN> static hipError_t launch_f32_skinny_t(const GemmArgs &a, hipStream_t s) {
  const int W = skf_waves((long long)a.br * skf_steps(a.k));
  const dim3 grid(skf_blocks(a.n, BN)), block(64 * W);
  if (skf_mb(a.m) == 16) hipLaunchKernelGGL((brgemm_f32_skinny<BN, 16>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((brgemm_f32_skinny<BN, 32>), grid, block, 0, s, a);
  return hipGetLastError();
}

// What both launchers of the tile (this file's and brgemm_f32_skinny_split.hip's) ask of a call on column blocks of bn:
//   bn 16 / 32 / 64; 1 <= m <= 31, n >= bn, n % 4 == 0, k >= 4, k % 4 == 0, a batch element (skf_shape_ok); lda >= k, ldb >= n, ldc >= n;
//   lda, ldb, ldc, stride_a and stride_b multiples of 4 elements and not negative; A, B, C and the bias row 16-byte aligned - every load of
//   A (16 bytes), of a row piece of B or the bias (4 .. 16 bytes) and every piece of C is then naturally aligned -; no VNNI operand, no
//   transposed B.
bool f32_skinny_args_ok(int bn, const GemmArgs &a) {
  if (!skf_shape_ok(a.m, a.n, a.k, a.br, bn) || a.b_trans || (a.ep & EP_VNNI_C)) return false;
  if (a.lda < a.k || a.ldb < a.n || a.ldc < a.n || ((a.lda | a.ldb | a.ldc | a.stride_a | a.stride_b) & 3) || a.stride_a < 0 || a.stride_b < 0) return false;
  return !((((uintptr_t)a.A | (uintptr_t)a.B | (uintptr_t)a.C) & 15) || ((a.ep & EP_BIAS) && (!a.D || ((uintptr_t)a.D & 15))));
}

// A flat f32 B on column blocks of bn (gemm_plan.cpp plan_gemm_call). Refuses with hipErrorInvalidValue everything the kernel does not
// assume (f32_skinny_args_ok) - the caller then runs the launch the call has with the mode off.
hipError_t launch_f32_skinny(int bn, const GemmArgs &a, hipStream_t s) {
  if (!f32_skinny_args_ok(bn, a)) return hipErrorInvalidValue;
  return bn == 16 ? launch_f32_skinny_t<16>(a, s) : bn == 32 ? launch_f32_skinny_t<32>(a, s) : launch_f32_skinny_t<64>(a, s);
}

} // namespace tpp
