// driver.cpp - TEST INFRASTRUCTURE for tests/test_edge_k_bf16_schedule.py, never part of the product library.
//
// Walks the ragged-k schedule of tpp-mlir_amd/csrc/brgemm_bf16_lw_kedge.h the way the kernel's two sides do and prints what each does:
//   <k> <br> <WK> <batch element> <chunk> L<loader position> S<chunk start> s<skipped steps> <kept steps of K group 0>,<group 1>
// The loader position is walked as blw_loader walks it with GRP = 4: + bkedge_step inside a batch element, the batch wrap (stride -
// bkedge_chunk_start(last)) behind its last chunk, with a stride of k + 40. A K group's kept steps are the k-steps of its share (wk * 4 /
// WK ..) for which bkedge_step_runs says yes, in the order of the chunk loop, as digits. Plain host C++: no device, no library.
#include "brgemm_bf16_lw_kedge.h"
#include <initializer_list>
#include <stdio.h>

using namespace tpp;

int main() {
  for (int k = 64; k <= 640; k += 16) {
    if (!bkedge_k_ok(k)) continue;
    for (int br = 1; br <= 3; ++br)
      for (int WK : {1, 2}) {
        const int stride = k + 40, chunks = bkedge_chunks(k), KS = BKEDGE_STEPS / WK;
        long pos = 0;
        for (int b = 0; b < br; ++b)
          for (int c = 0; c < chunks; ++c) {
            const int skip = bkedge_skip_steps(k, c);
            printf("%d %d %d %d %d L%ld S%d s%d ", k, br, WK, b, c, pos, bkedge_chunk_start(k, c), skip);
            for (int wk = 0; wk < WK; ++wk) {
              for (int q = 0; q < KS; ++q)
                if (bkedge_step_runs(wk * KS + q, skip)) printf("%d", wk * KS + q);
              printf(wk + 1 < WK ? "," : "\n");
            }
            pos += c + 1 < chunks ? bkedge_step(k, c) : stride - bkedge_chunk_start(k, chunks - 1);
          }
      }
  }
  for (int k : {0, 16, 48, 64, 72, 100, 128, 136, 200, 632, 640, 1000}) printf("ok %d %d\n", k, (int)bkedge_k_ok(k));
  for (int k : {80, 96, 112, 160, 272, 560, 784}) printf("facts %d %d %d %d\n", k, bkedge_chunks(k), bkedge_overlap(k), bkedge_skip_steps(k, bkedge_chunks(k) - 1));
  return 0;
}
