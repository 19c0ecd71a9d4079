// brgemm_bf16_skinny.h - the maps of the skinny-batch bf16 kernel (brgemm_bf16_skinny.hip, xsmm_hip_set_skinny_bf16), written once as plain
// constexpr functions: which (k, column) of B a lane's load holds, which loaded halves make the operand of MFMA j, where an accumulator
// register lands in C, which lane groups the last 32-k step of a ragged k keeps, where a column block sits and what it stores, and how the
// stream of 32-k steps is dealt over the waves of a workgroup. The kernel, its launcher, the planner (gemm_plan.cpp) and a CPU test
// (tests/test_skinny_map.py) all include this file. Nothing here needs a device: it compiles with any C++14 host compiler.
//
// One workgroup computes all m < 32 rows of one block of BN columns (BN = 16, 32, 64) on v_mfma_f32_16x16x32_bf16: lane l supplies
// A[row l & 15][k = 8 (l >> 4) + e] and B[k = 8 (l >> 4) + e][column l & 15], e = 0 .. 7, and receives C[row 4 (l >> 4) + i][column l & 15],
// i = 0 .. 3. A block is c = BN / 16 MFMAs wide: MFMA j (j = 0 .. c - 1) computes the block's columns c (l & 15) + j, so that a
// lane ends up with c CONSECUTIVE columns of four rows. B goes from global memory straight into the operand registers: per step a lane
// loads skn_rows(image) rows of its image, skn_dwords(image, BN) dwords each, and the operand of MFMA j is a selection of their halves.
// B images are coded as everywhere (GemmLaunch::b_kind): 0 VNNI-2 [k/2][ldb][2], 2 flat [k][ldb], 4 VNNI-4 [k/4][ldb][4].
#pragma once

namespace tpp {

constexpr int SKN_KSTEP = 32; // k per MFMA step
constexpr int SKN_WMAX = 8;   // most waves of a workgroup: the K split inside the workgroup (skn_waves)
constexpr int SKN_M_MAX = 31; // the rows the kernel takes: 1 .. 31 (MB = 16 for m <= 16, else two accumulator sets, MB = 32)

constexpr bool skn_image_ok(int img) { return img == 0 || img == 2 || img == 4; }
constexpr bool skn_bn_ok(int bn) { return bn == 16 || bn == 32 || bn == 64; }
// a flat B with BN = 16 would need 2-byte loads (one column of one k-row per lane): there is no such instance
constexpr bool skn_instance_exists(int img, int bn) { return skn_image_ok(img) && skn_bn_ok(bn) && !(img == 2 && bn == 16); }
constexpr int skn_mb(int m) { return m <= 16 ? 16 : 32; }
// k values a row of the image holds per column (its blocking factor)
constexpr int skn_vfac(int img) { return img == 0 ? 2 : img == 4 ? 4 : 1; }
// c: the columns a lane holds (= MFMAs per accumulator set and step)
constexpr int skn_cols(int bn) { return bn / 16; }
// per step a lane loads R image rows (its 8 k values) of P dwords (its c columns): R * P = 4 c dwords
constexpr int skn_rows(int img) { return 8 / skn_vfac(img); }
constexpr int skn_dwords(int img, int bn) { return skn_cols(bn) * skn_vfac(img) / 2; }
// LOAD MAP: half h (0 / 1) of dword p of image row r of lane l's step -> k within the step, column within the block. Element e = 2 p + h of
// the lane's row piece is k value e % vfac of column e / vfac.
constexpr int skn_load_k(int img, int l, int r, int p, int h) { return 8 * (l >> 4) + r * skn_vfac(img) + (2 * p + h) % skn_vfac(img); }
constexpr int skn_load_col(int img, int bn, int l, int p, int h) { return skn_cols(bn) * (l & 15) + (2 * p + h) / skn_vfac(img); }
// byte offset of the lane's row r from the start of the block's step slab (the slab: 32 k values x the block's columns from its first
// column on); ldb in elements. Row pitch 2 vfac ldb bytes, column pitch 2 vfac bytes.
constexpr long long skn_load_byte(int img, int bn, int l, int r, long long ldb) {
  return 2LL * skn_vfac(img) * ((long long)(skn_rows(img) * (l >> 4) + r) * ldb + skn_cols(bn) * (l & 15));
}
// FRAGMENT SELECTION: element e (k = 8 (l >> 4) + e) of the B operand of MFMA j is half `half` of dword `dword` of the lane's row `row`
struct SknSrc {
  int row, dword, half;
};
constexpr SknSrc skn_frag_src(int img, int j, int e) {
  return SknSrc{e / skn_vfac(img), (j * skn_vfac(img) + e % skn_vfac(img)) / 2, (j * skn_vfac(img) + e % skn_vfac(img)) % 2};
}
// OUTPUT MAP: register i of the accumulator of MFMA j, set s (rows 16 s ..), of lane l -> row of C, column within the block
constexpr int skn_out_row(int s, int l, int i) { return 16 * s + 4 * (l >> 4) + i; }
constexpr int skn_out_col(int bn, int l, int j) { return skn_cols(bn) * (l & 15) + j; }
// RAGGED k (k % 8 == 0): 32-k steps per batch element, the k values of step ks that exist, and whether lane l's group (k = 8 (l >> 4) ..
// + 7 of the step) lies below that limit. A group that does not issues no load and feeds zeros as A AND as B operand.
constexpr int skn_steps(int k) { return (k + SKN_KSTEP - 1) / SKN_KSTEP; }
constexpr int skn_step_klim(int k, int ks) { return k - ks * SKN_KSTEP < SKN_KSTEP ? k - ks * SKN_KSTEP : SKN_KSTEP; }
constexpr bool skn_group_kept(int l, int klim) { return 8 * (l >> 4) < klim; }
// COLUMN BLOCKS: ceil(n / BN) of them; every block but the last starts at BN b, the last one is shifted back to end at n (n >= BN, n % 8
// == 0: whole 16-byte pieces of every image). A block computes all its BN columns and stores those from BN b on - in the block, the local
// columns from skn_skip on; a lane's c columns (c divides 8) are all stored or all skipped.
constexpr int skn_blocks(int n, int bn) { return (n + bn - 1) / bn; }
constexpr int skn_origin(int b, int n, int bn) { return b * bn < n - bn ? b * bn : n - bn; }
constexpr int skn_skip(int b, int n, int bn) { return b * bn - skn_origin(b, n, bn); }
constexpr bool skn_owns(int b, int n, int bn, int col) { return col >= b * bn && col < skn_origin(b, n, bn) + bn; }
// THE DEAL: S = br * skn_steps(k) steps, numbered batch element by batch element, over W = min(SKN_WMAX, S) waves in contiguous runs - the
// first S % W waves take one step more. W depends on br and k alone.
constexpr int skn_waves(long long steps) { return steps < SKN_WMAX ? (int)steps : SKN_WMAX; }
constexpr int skn_wave_count(int w, int W, int S) { return S / W + (w < S % W ? 1 : 0); }
constexpr int skn_wave_first(int w, int W, int S) { return w * (S / W) + (w < S % W ? w : S % W); }
// what the launcher asks of the shape (the alignment rules: launch_bf16_skinny)
constexpr bool skn_shape_ok(long long m, long long n, long long k, long long br, int bn) {
  return m >= 1 && m <= SKN_M_MAX && n >= bn && n % 8 == 0 && k >= 8 && k % 8 == 0 && br >= 1 && br * skn_steps((int)k) < (1LL << 30);
}

} // namespace tpp
