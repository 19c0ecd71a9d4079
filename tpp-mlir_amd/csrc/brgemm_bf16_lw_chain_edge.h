// brgemm_bf16_lw_chain_edge.h - which row blocks a row block of a RAGGED-m layer chain depends on (brgemm_bf16_lw.hip GRP = 5, opt-in:
// xsmm_hip_set_chain_edge), written once as plain functions: the kernel, its launcher, the planner (gemm_plan.cpp) and a CPU test
// (tests/test_chain_edge_blocks.py) all include this file. Nothing here needs a device: it compiles with any C++14 host compiler.
//
// m rows - m >= BM, any m - run on tiles_m = ceil(m / BM) row blocks of BM rows. Block tm < tiles_m - 1 starts at row tm * BM. The LAST
// block is SHIFTED BACK to start at m - BM: it ends exactly at m, so no load or store leaves [0, m). Every block STORES its own rows only:
// the rows from tm * BM on, i.e. the last block skips its first tiles_m * BM - m rows - those are block tiles_m - 2's. In a chain, layer
// l + 1 of a block READS the rows [row0, row0 + BM) of layer l's output: the rows of the blocks first_block .. last_block. For every
// block but a shifted last one that is the block itself; a shifted last block reads rows of block tiles_m - 2 as well and must see BOTH
// blocks' layer-l tiles stored before it streams them.
#pragma once

namespace tpp {

// row blocks of m rows on tiles of bm rows
constexpr int chain_edge_tiles_m(int m, int bm) { return (m + bm - 1) / bm; }
// first row block tm loads (and computes)
constexpr int chain_edge_row0(int tm, int tiles_m, int m, int bm) { return tm + 1 == tiles_m && tiles_m * bm > m ? m - bm : tm * bm; }
// first row block tm stores, relative to chain_edge_row0: 0 for every block but a shifted last one
constexpr int chain_edge_own_row(int tm, int tiles_m, int m, int bm) { return tm * bm - chain_edge_row0(tm, tiles_m, m, bm); }
// rows block tm stores: [chain_edge_store_begin, chain_edge_store_end)
constexpr int chain_edge_store_begin(int tm, int /*tiles_m*/, int /*m*/, int bm) { return tm * bm; }
constexpr int chain_edge_store_end(int tm, int tiles_m, int m, int bm) { return tm + 1 == tiles_m ? m : (tm + 1) * bm; }
// the producers of the rows block tm reads from the layer before: the row blocks first_block .. last_block (one or two blocks)
constexpr int chain_edge_first_block(int tm, int tiles_m, int m, int bm) { return chain_edge_row0(tm, tiles_m, m, bm) / bm; }
constexpr int chain_edge_last_block(int tm, int /*tiles_m*/, int /*m*/, int /*bm*/) { return tm; }

} // namespace tpp
