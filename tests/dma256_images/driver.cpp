// Walks the B image maps of the 256x256 bf16 tile (tpp-mlir_amd/csrc/brgemm_bf16_dma256_images.h) on a CPU: the 16 LDS-DMA instructions of a
// chunk are carried out on a model of global memory whose every element names its own (k, column), then every fragment read of the MFMA
// waves is simulated on the resulting B slot. Prints facts; tests/test_dma256_images.py asserts them.
#include "brgemm_bf16_dma256_images.h"
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

using namespace tpp;

static const int LDB = 520, KTOT = 96, K0 = 32, N0 = 256; // the second chunk of the second column tile of a [96][520] operand

// element index of (k, column) in the operand of image img
static long long elem_at(int img, int k, int c) {
  const int rk = d256_b_row_k(img);
  return (long long)(k / rk) * rk * LDB + (long long)rk * c + k % rk;
}

static int run(int img, bool swz) {
  std::vector<unsigned> g((size_t)KTOT * LDB, 0xffffffffu); // (k << 16 | column), one per bf16 element
  for (int k = 0; k < KTOT; ++k)
    for (int c = 0; c < LDB; ++c) g[elem_at(img, k, c)] = (unsigned)k << 16 | (unsigned)c;
  std::vector<unsigned> lds(D256_B_SLOT / 2, 0xffffffffu);
  std::vector<int> hits(D256_B_SLOT, 0);
  int kmin = 1 << 30, kmax = -1, cmin = 1 << 30, cmax = -1, misaligned = 0;
  // the chunk's first row and the tile's first column, as the kernel forms its B pointer
  const long long base = (K0 / D256_BK) * d256_b_chunk_elems(LDB) + d256_b_col_elems(img, N0);
  for (int v = 0; v < D256_B_INSTR; ++v)
    for (int lane = 0; lane < 64; ++lane) {
      long long src_b = 2 * base + (long long)d256_b_dma_row(img, v, lane) * d256_b_row_bytes(img, LDB) + d256_b_dma_src(img, v, lane, swz);
      if (swz && (unsigned)(src_b - 2 * base) != d256_b_dma_voff(img, v, lane, LDB)) ++misaligned;
      if (src_b % 16) ++misaligned;
      const int dst = d256_b_dma_lds(v, lane);
      for (int e = 0; e < 8; ++e) {
        const unsigned val = g[src_b / 2 + e];
        lds[dst / 2 + e] = val;
        hits[dst + 2 * e]++, hits[dst + 2 * e + 1]++;
        const int k = (int)(val >> 16), c = (int)(val & 0xffff);
        if (k < kmin) kmin = k;
        if (k > kmax) kmax = k;
        if (c < cmin) cmin = c;
        if (c > cmax) cmax = c;
      }
    }
  int hmin = 1 << 30, hmax = -1;
  for (int b = 0; b < D256_B_SLOT; ++b) {
    if (hits[b] < hmin) hmin = hits[b];
    if (hits[b] > hmax) hmax = hits[b];
  }
  printf("cover %d %d bytes %d min %d max %d misaligned %d\n", img, (int)swz, D256_B_SLOT, hmin, hmax, misaligned);
  printf("src %d %d k %d %d c %d %d\n", img, (int)swz, kmin, kmax, cmin, cmax);

  // the reader
  long long reads = 0, wrong = 0, oob = 0, unaligned = 0;
  int worst = 0;
  for (int wn = 0; wn < 2; ++wn)
    for (int j = 0; j < 4; ++j)
      for (int ks = 0; ks < 2; ++ks)
        for (int h = 0; h < 2; ++h) {
          for (int lane = 0; lane < 64; ++lane) {
            unsigned got[4];
            const int a = d256_b_frag_lds(img, wn, j, ks, lane, h, swz);
            if (a < 0 || a + (img == 0 ? 1024 + 4 : 8) > D256_B_SLOT) { ++oob; continue; }
            if (a % (img == 0 ? 4 : 8)) ++unaligned;
            if (img == 0) { // two dwords one pair-row apart
              got[0] = lds[a / 2], got[1] = lds[a / 2 + 1], got[2] = lds[(a + 1024) / 2], got[3] = lds[(a + 1024) / 2 + 1];
            } else if (img == 2) { // ds_read_b64_tr_b16: element q comes from the 8 bytes another lane of the 16-lane group names
              for (int q = 0; q < 4; ++q) got[q] = lds[d256_b_frag_lds(img, wn, j, ks, d256_tr16_lane(lane, q), h, swz) / 2 + d256_tr16_elem(lane)];
            } else {
              for (int q = 0; q < 4; ++q) got[q] = lds[a / 2 + q];
            }
            for (int q = 0; q < 4; ++q) {
              const unsigned want = (unsigned)(K0 + d256_b_frag_k(ks, lane, h) + q) << 16 | (unsigned)(N0 + d256_b_frag_col(wn, j, lane));
              ++reads;
              if (got[q] != want) ++wrong;
            }
          }
          if (img != 0) // bank (a / 4) mod 64, per 32-lane half, equal addresses broadcast: the ways of the busiest bank
            for (int half = 0; half < 2; ++half) {
              std::set<int> per_bank[64];
              for (int lane = 32 * half; lane < 32 * half + 32; ++lane) {
                const int a = d256_b_frag_lds(img, wn, j, ks, lane, h, swz);
                per_bank[(a / 4) % 64].insert(a / 4), per_bank[(a / 4 + 1) % 64].insert(a / 4 + 1);
              }
              for (int b = 0; b < 64; ++b)
                if ((int)per_bank[b].size() > worst) worst = (int)per_bank[b].size();
            }
        }
  printf("frag %d %d reads %lld wrong %lld oob %lld unaligned %lld\n", img, (int)swz, reads, wrong, oob, unaligned);
  if (img != 0) printf("ways %d %d %d\n", img, (int)swz, worst);
  return 0;
}

int main() {
  run(0, true);
  run(2, true);
  run(4, true);
  run(2, false); // the flat image without its swizzle: writer and reader still agree, the reads conflict
  printf("steps %d %d slots %d %d ok %d %d %d %d\n", D256_KS_STEP, D256_H_STEP, D256_A_SLOT, D256_B_SLOT, (int)d256_image_ok(0), (int)d256_image_ok(2),
         (int)d256_image_ok(4), (int)d256_image_ok(1));
  printf("ldb %d %d %d %d %d %d\n", (int)d256_b_ldb_ok(2, 520), (int)d256_b_ldb_ok(2, 516), (int)d256_b_ldb_ok(4, 258), (int)d256_b_ldb_ok(4, 257),
         (int)d256_b_ldb_ok(2, 1ll << 25), (int)d256_b_ldb_ok(2, 248));
  return 0;
}
