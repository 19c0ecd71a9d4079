// brgemm_f32_narrow.h - the maps of the narrow-output f32 kernel (brgemm_f32_narrow.hip, xsmm_hip_set_narrow_f32), written once as plain
// constexpr functions: which (row, k) of A and which (k, column) of B a lane's loads hold, which of them MFMA r pairs, where an
// accumulator register lands in C, which lane groups the last 16-k step of a ragged k keeps, and how the stream of 16-k steps is dealt
// over the waves of a workgroup. The kernel, its launcher and the planner (gemm_plan.cpp) include this file. Nothing here needs a device:
// it compiles with any C++14 host compiler.
//
// The f32 half of brgemm_bf16_narrow.h, and the skinny-batch f32 problem (brgemm_f32_skinny.h) with the operands' roles exchanged: a tall
// layer with 1 .. 31 output columns is an ACTIVATION stream - its time is the bytes of A -, so one workgroup computes ALL n columns of one
// block of BM rows (BM = 16, 32, 64) on v_mfma_f32_16x16x4_f32: lane l supplies A[row l & 15][k-slot l >> 4] and B[k-slot l >> 4][column
// l & 15] and receives C[row 4 (l >> 4) + i][column l & 15], i = 0 .. 3. A block is BM / 16 row pieces j high and NB / 16 column sets t wide
// (NB = 16 for n <= 16, else 32: two accumulator sets that share every A fragment). A step is 16 consecutive k of one batch element. Lane
// (g = l >> 4, c = l & 15) loads ONE 16-byte piece of A per row piece - row 16 j + c, k = 4 g .. 4 g + 3 of the step - and, per column set,
// the four elements B[k = 4 g + r][column 16 t + c], r = 0 .. 3, of the flat B [k][ldb]. MFMA r takes element r of the A piece and B
// element r: k-slot g of that MFMA is the real k 4 g + r on BOTH sides - a permutation of k inside the step, free because the step is a sum.
#pragma once

namespace tpp {

constexpr int NRF_KSTEP = 16; // k per step: 4 MFMAs of 4 k-slots per accumulator
constexpr int NRF_WMAX = 8;   // most waves of a workgroup: the K split inside the workgroup (nrf_waves)
constexpr int NRF_M_MIN = 32, NRF_N_MAX = 31; // the calls the kernel takes: m >= 32 (below: the skinny-batch kernel's side), 1 <= n <= 31
// THE BOUND OF THE OFFSET ARITHMETIC: every offset is a 64-bit byte count made of at most three products of two of these numbers, so with
// each below 2^30 (rows below 2^24: the grid times the workgroup stays below 2^32 threads) no sum reaches 2^63. Refused beyond it.
constexpr long long NRF_ROWS_MAX = 1LL << 24, NRF_EXTENT_MAX = 1LL << 30;

constexpr bool nrf_bm_ok(int bm) { return bm == 16 || bm == 32 || bm == 64; }
constexpr int nrf_nb(int n) { return n <= 16 ? 16 : 32; }
// every one of the 3 x 2 instances has no scratch and at most 256 VGPRs (profiles/narrow_f32_isa.txt): none is left out
constexpr bool nrf_instance_exists(int bm, int nb) { return nrf_bm_ok(bm) && (nb == 16 || nb == 32); }
constexpr int nrf_blocks(long long m, int bm) { return (int)((m + bm - 1) / bm); }
// an index at or beyond the limit is read from the last one that exists - and never stored
constexpr int nrf_clamp(int x, int lim) { return x < lim ? x : lim - 1; }
// A LOAD MAP: piece j (j = 0 .. BM / 16 - 1) of lane l is 4 k values, 16 bytes: row 16 j + (l & 15) of the block, k = 4 (l >> 4) .. + 3 of the step
constexpr int nrf_a_row(int l, int j) { return 16 * j + (l & 15); }
constexpr int nrf_a_k(int l, int e) { return 4 * (l >> 4) + e; }
// B LOAD MAP: load r (0 .. 3) of column set t of lane l is ONE element: k = 4 (l >> 4) + r of the step, column 16 t + (l & 15)
constexpr int nrf_b_k(int l, int r) { return 4 * (l >> 4) + r; }
constexpr int nrf_b_col(int l, int t) { return 16 * t + (l & 15); }
// OPERAND SELECTION: MFMA r of a step takes element r of the A piece and the B element of load r
constexpr int nrf_mfma_a_elem(int r) { return r; }
constexpr int nrf_mfma_b_load(int r) { return r; }
// OUTPUT MAP: register i of the accumulator of row piece j, column set t, of lane l -> row within the block, column
constexpr int nrf_out_row(int j, int l, int i) { return 16 * j + 4 * (l >> 4) + i; }
constexpr int nrf_out_col(int t, int l) { return 16 * t + (l & 15); }
// RAGGED k (k % 4 == 0): 16-k steps per batch element, the k values of step ks that exist, and whether lane l's group (k = 4 (l >> 4) ..
// + 3 of the step) lies below that limit. A group that does not issues no load and feeds +0.0 as A AND as B operand.
constexpr int nrf_steps(int k) { return (k + NRF_KSTEP - 1) / NRF_KSTEP; }
constexpr int nrf_step_klim(int k, int ks) { return k - ks * NRF_KSTEP < NRF_KSTEP ? k - ks * NRF_KSTEP : NRF_KSTEP; }
constexpr bool nrf_group_kept(int l, int klim) { return 4 * (l >> 4) < klim; }
// THE DEAL: S = br * nrf_steps(k) steps, numbered batch element by batch element, over W = min(NRF_WMAX, S) waves in contiguous runs - the
// first S % W waves take one step more. W depends on br and k alone.
constexpr int nrf_waves(long long steps) { return steps < NRF_WMAX ? (int)steps : NRF_WMAX; }
constexpr int nrf_wave_count(int w, int W, int S) { return S / W + (w < S % W ? 1 : 0); }
constexpr int nrf_wave_first(int w, int W, int S) { return w * (S / W) + (w < S % W ? w : S % W); }
// what the launcher asks of the shape (the alignment rules: launch_f32_narrow)
constexpr bool nrf_shape_ok(long long m, long long n, long long k, long long br) {
  return m >= NRF_M_MIN && m < NRF_ROWS_MAX && n >= 1 && n <= NRF_N_MAX && k >= 4 && k % 4 == 0 && k < NRF_EXTENT_MAX && br >= 1 &&
         br * nrf_steps((int)k) < NRF_EXTENT_MAX;
}
constexpr bool nrf_extents_ok(long long lda, long long ldb, long long ldc, long long stride_a, long long stride_b) {
  return lda < NRF_EXTENT_MAX && ldb < NRF_EXTENT_MAX && ldc < NRF_EXTENT_MAX && stride_a >= 0 && stride_a < NRF_EXTENT_MAX && stride_b >= 0 &&
         stride_b < NRF_EXTENT_MAX;
}

} // namespace tpp
