// driver.cpp - TEST INFRASTRUCTURE for tests/test_edge_k_schedule.py, never part of the product library.
//
// Walks the ragged-k schedule of tpp-mlir_amd/csrc/brgemm_f32_lw_kedge.h the way the kernel's two sides do and prints what each does:
//   <k> <br> <WK> <batch element> <chunk> L<loader position> S<chunk start> s<skipped blocks> <kept blocks of K group 0>,<group 1>,...
// The loader position is walked as Loader::issue_ragged walks it: + kedge_step inside a batch element, the batch wrap (stride -
// kedge_chunk_start(last)) behind its last chunk, with a stride of k + 24. A K group's kept blocks are the k-blocks of its share (wk * 8 /
// WK ..) for which kedge_block_runs says yes, in the order of the chunk loop, as digits. Plain host C++: no device, no library.
#include "brgemm_f32_lw_kedge.h"
#include <initializer_list>
#include <stdio.h>

using namespace tpp;

int main() {
  for (int k = 64; k <= 640; k += 8) {
    if (!kedge_k_ok(k)) continue;
    for (int br = 1; br <= 3; ++br)
      for (int WK : {1, 2, 4}) {
        const int stride = k + 24, chunks = kedge_chunks(k);
        long pos = 0;
        for (int b = 0; b < br; ++b)
          for (int c = 0; c < chunks; ++c) {
            const int skip = kedge_skip_blocks(k, c);
            printf("%d %d %d %d %d L%ld S%d s%d ", k, br, WK, b, c, pos, kedge_chunk_start(k, c), skip);
            for (int wk = 0; wk < WK; ++wk) {
              for (int q = 0; q < 8 / WK; ++q)
                if (kedge_block_runs(wk * (8 / WK) + q, skip)) printf("%d", wk * (8 / WK) + q);
              printf(wk + 1 < WK ? "," : "\n");
            }
            pos += c + 1 < chunks ? kedge_step(k, c) : stride - kedge_chunk_start(k, chunks - 1);
          }
      }
  }
  for (int k : {0, 8, 56, 64, 100, 128, 132, 636, 640}) printf("ok %d %d\n", k, (int)kedge_k_ok(k));
  return 0;
}
