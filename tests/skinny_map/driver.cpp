// Walks the maps of the skinny-batch bf16 kernel (tpp-mlir_amd/csrc/brgemm_bf16_skinny.h) on a CPU, for one instance: B image (0 VNNI-2,
// 2 flat, 4 VNNI-4) and column-block width BN. Prints facts; tests/test_skinny_map.py asserts them.
//   driver <image> <bn>
// The image's own address function is restated here (elem_index), independent of the header.
#include "brgemm_bf16_skinny.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace tpp;

// element index of B[k][col] in an image with leading dimension ldb
static long long elem_index(int img, long long k, long long col, long long ldb) {
  if (img == 0) return ((k / 2) * ldb + col) * 2 + k % 2;
  if (img == 4) return ((k / 4) * ldb + col) * 4 + k % 4;
  return k * ldb + col;
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  const int img = atoi(argv[1]), bn = atoi(argv[2]);
  if (!skn_instance_exists(img, bn)) return 3;
  const int c = skn_cols(bn), R = skn_rows(img), P = skn_dwords(img, bn);
  printf("instance image %d bn %d c %d rows %d dwords %d\n", img, bn, c, R, P);

  // 1. the load map: every (k, column) of a step's 32 x BN slab exactly once; the byte offsets are the image's addresses
  {
    std::vector<int> seen(32 * bn, 0);
    long outside = 0, byte_mismatch = 0;
    const long long ldb = 1000;
    for (int l = 0; l < 64; ++l)
      for (int r = 0; r < R; ++r)
        for (int p = 0; p < P; ++p)
          for (int h = 0; h < 2; ++h) {
            const int k = skn_load_k(img, l, r, p, h), col = skn_load_col(img, bn, l, p, h);
            if (k < 0 || k >= 32 || col < 0 || col >= bn) { ++outside; continue; }
            ++seen[k * bn + col];
            if (skn_load_byte(img, bn, l, r, ldb) + 4 * p + 2 * h != 2 * elem_index(img, k, col, ldb)) ++byte_mismatch;
          }
    long once = 0, never = 0, more = 0;
    for (int v : seen) once += v == 1, never += v == 0, more += v > 1;
    printf("slab once %ld never %ld more %ld outside %ld byte_mismatch %ld\n", once, never, more, outside, byte_mismatch);
  }
  // 2. the fragment selection: element e of MFMA j's operand of lane l is k = 8 (l >> 4) + e of column c (l & 15) + j - and with the
  // selection of ANOTHER image it is not (the control)
  for (int sel = 0; sel <= 4; sel += 2) {
    long wrong = 0, off_lane = 0;
    for (int l = 0; l < 64; ++l)
      for (int j = 0; j < c; ++j)
        for (int e = 0; e < 8; ++e) {
          const SknSrc s = skn_frag_src(sel, j, e);
          if (s.row < 0 || s.row >= R || s.dword < 0 || s.dword >= P) { ++off_lane; continue; }
          if (skn_load_k(img, l, s.row, s.dword, s.half) != 8 * (l >> 4) + e || skn_load_col(img, bn, l, s.dword, s.half) != c * (l & 15) + j) ++wrong;
        }
    printf("frag selection_of %d wrong %ld off_lane %ld\n", sel, wrong, off_lane);
  }
  // 3. the output map and the column blocks: every (row < m, column < n) stored exactly once; every block's loads inside the operand;
  // the kernel's form of the predicate (a lane's first local column at or behind the skip) is skn_owns; without it: stored twice
  static const int ms[] = {1, 7, 16, 17, 31}, ns[] = {16, 24, 72, 200, 1000};
  for (int m : ms)
    for (int n : ns) {
      if (n < bn) continue;
      const int sets = skn_mb(m) / 16, blocks = skn_blocks(n, bn);
      std::vector<int> stored((size_t)m * n, 0), unpred((size_t)m * n, 0);
      long outside = 0, origin_off8 = 0, pred_mismatch = 0, split_lane = 0;
      for (int b = 0; b < blocks; ++b) {
        const int n0 = skn_origin(b, n, bn), skip = skn_skip(b, n, bn);
        if (n0 < 0 || n0 + bn > n) ++outside;
        if (n0 % 8) ++origin_off8;
        for (int l = 0; l < 64; ++l) {
          const bool lane_stores = skn_out_col(bn, l, 0) >= skip;
          for (int j = 0; j < c; ++j) {
            const int col = n0 + skn_out_col(bn, l, j);
            if (col < 0 || col >= n) { ++outside; continue; }
            if (skn_owns(b, n, bn, col) != lane_stores) ++pred_mismatch; // (also: a lane's c columns are all stored or all skipped)
            if ((skn_out_col(bn, l, j) >= skip) != lane_stores) ++split_lane;
            for (int s = 0; s < sets; ++s)
              for (int i = 0; i < 4; ++i) {
                const int row = skn_out_row(s, l, i);
                if (row >= m) continue;
                ++unpred[(size_t)row * n + col];
                if (lane_stores) ++stored[(size_t)row * n + col];
              }
          }
        }
      }
      long once = 0, never = 0, more = 0, twice = 0, unever = 0;
      for (size_t i = 0; i < stored.size(); ++i) {
        once += stored[i] == 1, never += stored[i] == 0, more += stored[i] > 1;
        twice += unpred[i] > 1, unever += unpred[i] == 0;
      }
      printf("store m %d n %d blocks %d once %ld never %ld more %ld outside %ld origin_off8 %ld pred_mismatch %ld split_lane %ld unpredicated_twice %ld unpredicated_never %ld\n",
             m, n, blocks, once, never, more, outside, origin_off8, pred_mismatch, split_lane, twice, unever);
    }
  // 4. ragged k: the groups kept in the last step hold exactly the k values below the limit
  for (int kmod = 0; kmod < 32; kmod += 8) {
    const int k = 64 + kmod, steps = skn_steps(k);
    long kept_below = 0, kept_beyond = 0, dropped_below = 0, full_steps_masked = 0;
    for (int ks = 0; ks < steps; ++ks) {
      const int klim = skn_step_klim(k, ks);
      for (int l = 0; l < 64; l += 16) // one lane per group
        for (int e = 0; e < 8; ++e) {
          const int kk = ks * SKN_KSTEP + 8 * (l >> 4) + e;
          const bool kept = skn_group_kept(l, klim);
          if (ks < steps - 1 && !kept) ++full_steps_masked;
          if (ks == steps - 1) kept_below += kept && kk < k, kept_beyond += kept && kk >= k, dropped_below += !kept && kk < k;
        }
    }
    printf("mask kmod %d steps %d last_klim %d kept_below %ld kept_beyond %ld dropped_below %ld full_steps_masked %ld\n", kmod, steps,
           skn_step_klim(k, steps - 1), kept_below, kept_beyond, dropped_below, full_steps_masked);
  }
  // 5. the deal: every step belongs to exactly one wave, in contiguous ascending runs
  static const int Ss[] = {1, 2, 3, SKN_WMAX - 1, SKN_WMAX, SKN_WMAX + 1, 5 * SKN_WMAX + 3};
  for (int S : Ss) {
    const int W = skn_waves(S);
    std::vector<int> owner(S, 0);
    long out_of_order = 0, idle = 0;
    int next = 0;
    for (int w = 0; w < W; ++w) {
      const int first = skn_wave_first(w, W, S), cnt = skn_wave_count(w, W, S);
      if (first != next) ++out_of_order;
      if (cnt < 1) ++idle;
      for (int t = first; t < first + cnt; ++t)
        if (t >= 0 && t < S) ++owner[t];
        else ++out_of_order;
      next = first + cnt;
    }
    long once = 0;
    for (int v : owner) once += v == 1;
    printf("deal steps %d waves %d once %ld out_of_order %ld idle %ld end %d\n", S, W, once, out_of_order, idle, next);
  }
  return 0;
}
