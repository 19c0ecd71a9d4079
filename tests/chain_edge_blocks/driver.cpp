// driver.cpp - TEST INFRASTRUCTURE for tests/test_chain_edge_blocks.py, never part of the product library.
//
// Walks tpp-mlir_amd/csrc/brgemm_bf16_lw_chain_edge.h - the header the chain kernel on edge row tiles includes - as plain host C++: for
// every BM in {32, 64, 128} and every m in [BM, 4 BM + 7] one line per row block
//   <BM> <m> <tiles_m> <tm> r<first row loaded> o<first row stored, block-relative> s<store begin>:<store end> w<first block>:<last block>
#include "brgemm_bf16_lw_chain_edge.h"
#include <initializer_list>
#include <stdio.h>

using namespace tpp;

static_assert(chain_edge_first_block(2, 3, 189, 64) == 1 && chain_edge_last_block(2, 3, 189, 64) == 2, "3 BM - 3 rows: the last block waits for blocks 1 and 2");
static_assert(chain_edge_row0(1, 2, 72, 64) == 8 && chain_edge_own_row(1, 2, 72, 64) == 56, "BM + 8 rows: the last block owns 8 rows");

int main() {
  for (int bm : {32, 64, 128})
    for (int m = bm; m <= 4 * bm + 7; ++m) {
      const int tiles_m = chain_edge_tiles_m(m, bm);
      for (int tm = 0; tm < tiles_m; ++tm)
        printf("%d %d %d %d r%d o%d s%d:%d w%d:%d\n", bm, m, tiles_m, tm, chain_edge_row0(tm, tiles_m, m, bm), chain_edge_own_row(tm, tiles_m, m, bm),
               chain_edge_store_begin(tm, tiles_m, m, bm), chain_edge_store_end(tm, tiles_m, m, bm), chain_edge_first_block(tm, tiles_m, m, bm),
               chain_edge_last_block(tm, tiles_m, m, bm));
    }
  return 0;
}
