// brgemm_bf16_narrow.h - the maps of the narrow-output bf16 kernel (brgemm_bf16_narrow.hip, xsmm_hip_set_narrow_bf16), written once as plain
// constexpr functions: which (row, k) of A and which (k, column) of B a lane's loads hold, where a loaded B element sits in its image, where
// an accumulator register lands in C, which lane groups the last 32-k step of a ragged k keeps, and how the stream of 32-k steps is dealt
// over the waves of a workgroup. The kernel, its launcher, the planner (gemm_plan.cpp) and a CPU test (tests/test_narrow_bf16_cpu.py) all
// include this file. Nothing here needs a device: it compiles with any C++14 host compiler.
//
// The skinny-batch problem (brgemm_bf16_skinny.h) with the operands' roles exchanged: a tall layer with 1 .. 31 output columns is an
// ACTIVATION stream - its time is the bytes of A -, so one workgroup computes ALL n columns of one block of BM rows (BM = 16, 32, 64) on
// v_mfma_f32_16x16x32_bf16: lane l supplies A[row l & 15][k = 8 (l >> 4) + e] and B[k = 8 (l >> 4) + e][column l & 15], e = 0 .. 7, and receives
// C[row 4 (l >> 4) + i][column l & 15], i = 0 .. 3. A block is BM / 16 row pieces j high and NB / 16 column sets t wide (NB = 16 for n <= 16,
// else 32: two accumulator sets that share every A fragment). A row of A is what the MFMA wants as is: per step lane l loads ONE 16-byte
// piece per row piece, straight into the operand registers. B is a few KiB that every workgroup re-reads from L2, as its image stores it.
// B images are coded as everywhere (GemmLaunch::b_kind): 0 VNNI-2 [k/2][ldb][2], 2 flat [k][ldb], 4 VNNI-4 [k/4][ldb][4].
#pragma once

namespace tpp {

constexpr int NRW_KSTEP = 32; // k per MFMA step
constexpr int NRW_WMAX = 8;   // most waves of a workgroup: the K split inside the workgroup (nrw_waves)
constexpr int NRW_M_MIN = 32, NRW_N_MAX = 31; // the calls the kernel takes: m >= 32 (below: the skinny-batch kernel's side), 1 <= n <= 31
// THE BOUND OF THE OFFSET ARITHMETIC: every offset is a 64-bit byte count made of at most three products of two of these numbers, so with
// each below 2^30 (rows below 2^24: the grid times the workgroup stays below 2^32 threads) no sum reaches 2^63. Refused beyond it.
constexpr long long NRW_ROWS_MAX = 1LL << 24, NRW_EXTENT_MAX = 1LL << 30;

constexpr bool nrw_image_ok(int img) { return img == 0 || img == 2 || img == 4; }
constexpr bool nrw_bm_ok(int bm) { return bm == 16 || bm == 32 || bm == 64; }
constexpr int nrw_nb(int n) { return n <= 16 ? 16 : 32; }
// every one of the 3 x 3 x 2 instances has no scratch and at most 256 VGPRs (profiles/narrow_bf16_isa.txt): none is left out
constexpr bool nrw_instance_exists(int img, int bm, int nb) { return nrw_image_ok(img) && nrw_bm_ok(bm) && (nb == 16 || nb == 32); }
constexpr int nrw_blocks(long long m, int bm) { return (int)((m + bm - 1) / bm); }
// an index at or beyond the limit is read from the last one that exists - and never stored
constexpr int nrw_clamp(int x, int lim) { return x < lim ? x : lim - 1; }
// A LOAD MAP: piece j (j = 0 .. BM / 16 - 1) of lane l is 8 k values, 16 bytes: row 16 j + (l & 15) of the block, k = 8 (l >> 4) .. + 7 of the step
constexpr int nrw_a_row(int l, int j) { return 16 * j + (l & 15); }
constexpr int nrw_a_k(int l) { return 8 * (l >> 4); }
// B LOAD MAP: the lane's 8 k values of column 16 t + (l & 15) come as R loads of vfac elements - four 4-byte pair-rows (VNNI-2), two 8-byte
// k-group rows (VNNI-4), eight 2-byte elements (flat). Element e of load r is k = 8 (l >> 4) + vfac r + e: operand element vfac r + e, no selection.
constexpr int nrw_vfac(int img) { return img == 0 ? 2 : img == 4 ? 4 : 1; }
constexpr int nrw_b_loads(int img) { return 8 / nrw_vfac(img); }
constexpr int nrw_b_k(int img, int l, int r, int e) { return 8 * (l >> 4) + nrw_vfac(img) * r + e; }
constexpr int nrw_b_col(int l, int t) { return 16 * t + (l & 15); }
// element offset of (k, column) of one batch element in its image; ldb in elements. The lane's load r starts at nrw_b_elem(k of e = 0).
constexpr long long nrw_b_elem(int img, long long k, long long col, long long ldb) {
  return (k / nrw_vfac(img) * ldb + col) * nrw_vfac(img) + k % nrw_vfac(img);
}
// OUTPUT MAP: register i of the accumulator of row piece j, column set t, of lane l -> row within the block, column
constexpr int nrw_out_row(int j, int l, int i) { return 16 * j + 4 * (l >> 4) + i; }
constexpr int nrw_out_col(int t, int l) { return 16 * t + (l & 15); }
// RAGGED k (k % 8 == 0): 32-k steps per batch element, the k values of step ks that exist, and whether lane l's group (k = 8 (l >> 4) ..
// + 7 of the step) lies below that limit. A group that does not issues no load and feeds zeros as A AND as B operand.
constexpr int nrw_steps(int k) { return (k + NRW_KSTEP - 1) / NRW_KSTEP; }
constexpr int nrw_step_klim(int k, int ks) { return k - ks * NRW_KSTEP < NRW_KSTEP ? k - ks * NRW_KSTEP : NRW_KSTEP; }
constexpr bool nrw_group_kept(int l, int klim) { return 8 * (l >> 4) < klim; }
// THE DEAL: S = br * nrw_steps(k) steps, numbered batch element by batch element, over W = min(NRW_WMAX, S) waves in contiguous runs - the
// first S % W waves take one step more. W depends on br and k alone.
constexpr int nrw_waves(long long steps) { return steps < NRW_WMAX ? (int)steps : NRW_WMAX; }
constexpr int nrw_wave_count(int w, int W, int S) { return S / W + (w < S % W ? 1 : 0); }
constexpr int nrw_wave_first(int w, int W, int S) { return w * (S / W) + (w < S % W ? w : S % W); }
// what the launcher asks of the shape (the alignment rules: launch_bf16_narrow)
constexpr bool nrw_shape_ok(long long m, long long n, long long k, long long br) {
  return m >= NRW_M_MIN && m < NRW_ROWS_MAX && n >= 1 && n <= NRW_N_MAX && k >= 8 && k % 8 == 0 && k < NRW_EXTENT_MAX && br >= 1 &&
         br * nrw_steps((int)k) < NRW_EXTENT_MAX;
}
constexpr bool nrw_extents_ok(long long lda, long long ldb, long long ldc, long long stride_a, long long stride_b) {
  return lda < NRW_EXTENT_MAX && ldb < NRW_EXTENT_MAX && ldc < NRW_EXTENT_MAX && stride_a >= 0 && stride_a < NRW_EXTENT_MAX && stride_b >= 0 &&
         stride_b < NRW_EXTENT_MAX;
}

} // namespace tpp
