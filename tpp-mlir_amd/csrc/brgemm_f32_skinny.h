// brgemm_f32_skinny.h - the maps of the skinny-batch f32 kernel (brgemm_f32_skinny.hip, xsmm_hip_set_skinny_f32), written once as plain
// constexpr functions: which (k, column) of B a lane's load holds, which k the lane's piece of A holds, which of them MFMA (r, j) pairs,
// where an accumulator register lands in C, which lane groups the last 16-k step of a ragged k keeps, where a column block sits and what
// it stores, and how the stream of 16-k steps is dealt over the waves of a workgroup. The kernel, its launcher, the planner
// (gemm_plan.cpp) and a CPU test (tests/test_skinny_f32_cpu.py) all include this file. Nothing here needs a device: it compiles with any
// C++14 host compiler.
//
// One workgroup computes all m < 32 rows of one block of BN columns (BN = 16, 32, 64) on v_mfma_f32_16x16x4_f32: lane l supplies
// A[row l & 15][k-slot l >> 4] and B[k-slot l >> 4][column l & 15] and receives C[row 4 (l >> 4) + i][column l & 15], i = 0 .. 3. A step
// is 16 consecutive k of one batch element. Lane (g = l >> 4, c = l & 15) loads rows 4 g + r, r = 0 .. 3, of the step's slab of the flat
// B [k][ldb], C = BN / 16 consecutive floats each (columns C c .. C c + C - 1 of the block), and ONE piece of four floats of its row of
// A: k = 4 g .. 4 g + 3. MFMA (r, j) takes element j of the lane's B row r and element r of its A piece: k-slot g of that MFMA is the
// real k 4 g + r on BOTH sides - a permutation of k inside the step, free because the step is a sum - and its output column l & 15 is
// the block's column C c + j, so that a lane ends up with C CONSECUTIVE columns of four rows.
#pragma once

namespace tpp {

constexpr int SKF_KSTEP = 16; // k per step: 4 MFMAs of 4 k-slots per column of a lane
constexpr int SKF_WMAX = 8;   // most waves of a workgroup: the K split inside the workgroup (skf_waves)
constexpr int SKF_M_MAX = 31; // the rows the kernel takes: 1 .. 31 (MB = 16 for m <= 16, else two accumulator sets, MB = 32)

constexpr bool skf_bn_ok(int bn) { return bn == 16 || bn == 32 || bn == 64; }
constexpr int skf_mb(int m) { return m <= 16 ? 16 : 32; }
// C: the columns a lane holds (= floats of a row piece = MFMAs per accumulator set and B row)
constexpr int skf_cols(int bn) { return bn / 16; }
// LOAD MAP: element e (0 .. C - 1) of row r (0 .. 3) of lane l's step -> k within the step, column within the block
constexpr int skf_load_k(int l, int r) { return 4 * (l >> 4) + r; }
constexpr int skf_load_col(int bn, int l, int e) { return skf_cols(bn) * (l & 15) + e; }
// byte offset of the lane's row r from the start of the block's step slab (16 k values x the block's columns from its first column
// on); ldb in elements
constexpr long long skf_load_byte(int bn, int l, int r, long long ldb) { return 4LL * ((long long)(4 * (l >> 4) + r) * ldb + skf_cols(bn) * (l & 15)); }
// THE A PIECE: element e (0 .. 3) of the piece of set s of lane l -> row of A (before the clamp to m - 1), k within the step
constexpr int skf_a_row(int s, int l) { return 16 * s + (l & 15); }
constexpr int skf_a_k(int l, int e) { return 4 * (l >> 4) + e; }
// OPERAND SELECTION: MFMA (r, j) of a step takes element skf_mfma_b_elem of B row skf_mfma_b_row and element skf_mfma_a_elem of the A piece
constexpr int skf_mfma_b_row(int r, int j) { return r; }
constexpr int skf_mfma_b_elem(int r, int j) { return j; }
constexpr int skf_mfma_a_elem(int r, int j) { return r; }
// OUTPUT MAP: register i of the accumulator of column j, set s (rows 16 s ..), of lane l -> row of C, column within the block
constexpr int skf_out_row(int s, int l, int i) { return 16 * s + 4 * (l >> 4) + i; }
constexpr int skf_out_col(int bn, int l, int j) { return skf_cols(bn) * (l & 15) + j; }
// RAGGED k (k % 4 == 0): 16-k steps per batch element, the k values of step ks that exist, and whether lane l's group (k = 4 (l >> 4) ..
// + 3 of the step) lies below that limit. A group that does not issues no load and feeds +0.0 as A AND as B operand.
constexpr int skf_steps(int k) { return (k + SKF_KSTEP - 1) / SKF_KSTEP; }
constexpr int skf_step_klim(int k, int ks) { return k - ks * SKF_KSTEP < SKF_KSTEP ? k - ks * SKF_KSTEP : SKF_KSTEP; }
constexpr bool skf_group_kept(int l, int klim) { return 4 * (l >> 4) < klim; }
// COLUMN BLOCKS: ceil(n / BN) of them; every block but the last starts at BN b, the last one is shifted back to end at n (n >= BN, n % 4
// == 0: whole 16-byte pieces). A block computes all its BN columns and stores those from BN b on - in the block, the local columns from
// skf_skip on; a lane's C columns (C divides 4) are all stored or all skipped.
constexpr int skf_blocks(int n, int bn) { return (n + bn - 1) / bn; }
constexpr int skf_origin(int b, int n, int bn) { return b * bn < n - bn ? b * bn : n - bn; }
constexpr int skf_skip(int b, int n, int bn) { return b * bn - skf_origin(b, n, bn); }
constexpr bool skf_owns(int b, int n, int bn, int col) { return col >= b * bn && col < skf_origin(b, n, bn) + bn; }
// THE DEAL: S = br * skf_steps(k) steps, numbered batch element by batch element, over W = min(SKF_WMAX, S) waves in contiguous runs - the
// first S % W waves take one step more. W depends on br and k alone.
constexpr int skf_waves(long long steps) { return steps < SKF_WMAX ? (int)steps : SKF_WMAX; }
constexpr int skf_wave_count(int w, int W, int S) { return S / W + (w < S % W ? 1 : 0); }
constexpr int skf_wave_first(int w, int W, int S) { return w * (S / W) + (w < S % W ? w : S % W); }
// what the launcher asks of the shape (the alignment rules: launch_f32_skinny)
constexpr bool skf_shape_ok(long long m, long long n, long long k, long long br, int bn) {
  return skf_bn_ok(bn) && m >= 1 && m <= SKF_M_MAX && n >= bn && n % 4 == 0 && n < (1LL << 30) && k >= 4 && k % 4 == 0 && k < (1LL << 30) && br >= 1 &&
         br * skf_steps((int)k) < (1LL << 30);
}

} // namespace tpp
