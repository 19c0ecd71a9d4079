// driver.cpp - TEST INFRASTRUCTURE for tests/test_edge_k8_bf16_schedule.py, never part of the product library.
//
// Walks the half-step ragged-k schedule of tpp-mlir_amd/csrc/brgemm_bf16_lw_kedge.h (bkedge8_*) the way the kernel's two sides do and prints
// what each does:
//   <k> <br> <WK> <batch element> <chunk> L<loader position> S<chunk start> s<skipped half steps> <steps of K group 0>,<group 1>
// The loader position is walked as blw_loader walks it with GRP = 6: + bkedge_step inside a batch element, the batch wrap (stride -
// bkedge_chunk_start(last)) behind its last chunk, with a stride of k + 40. A K group's steps are the k-steps of its share (wk * 4 / WK ..)
// that bkedge8_step_part does not answer with "not run", in the order of the chunk loop: the digit of a whole step, the digit followed
// by 'u' for a step that multiplies its upper eight k-values only. Plain host C++: no device, no library.
#include "brgemm_bf16_lw_kedge.h"
#include <initializer_list>
#include <stdio.h>

using namespace tpp;

int main() {
  for (int k = 72; k <= 648; k += 16) {
    if (!bkedge8_k_ok(k)) continue;
    for (int br = 1; br <= 3; ++br)
      for (int WK : {1, 2}) {
        const int stride = k + 40, chunks = bkedge_chunks(k), KS = BKEDGE_STEPS / WK;
        long pos = 0;
        for (int b = 0; b < br; ++b)
          for (int c = 0; c < chunks; ++c) {
            const int skip = bkedge8_skip_halves(k, c);
            printf("%d %d %d %d %d L%ld S%d s%d ", k, br, WK, b, c, pos, bkedge_chunk_start(k, c), skip);
            for (int wk = 0; wk < WK; ++wk) {
              for (int q = 0; q < KS; ++q) {
                const int part = bkedge8_step_part(wk * KS + q, skip);
                if (part == BKEDGE8_WHOLE) printf("%d", wk * KS + q);
                if (part == BKEDGE8_UPPER) printf("%du", wk * KS + q);
              }
              printf(wk + 1 < WK ? "," : "\n");
            }
            pos += c + 1 < chunks ? bkedge_step(k, c) : stride - bkedge_chunk_start(k, chunks - 1);
          }
      }
  }
  for (int k : {0, 8, 56, 64, 76, 80, 128, 784, 72, 200, 1000}) printf("ok %d %d\n", k, (int)bkedge8_k_ok(k));
  for (int k : {72, 88, 104, 120, 168, 200, 296, 568, 1000}) printf("facts %d %d %d\n", k, bkedge_chunks(k), bkedge_overlap(k));
  return 0;
}
