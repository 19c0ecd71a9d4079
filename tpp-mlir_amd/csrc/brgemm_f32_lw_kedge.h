// brgemm_f32_lw_kedge.h - the schedule of a RAGGED-k batch element on the f32 loader-wave tiles (brgemm_f32_lw.hip brgemm_f32_lw_kedge,
// opt-in: xsmm_hip_set_edge_k), written once as plain functions: the kernel, its launcher, the planner (gemm_plan.cpp) and a CPU test
// (tests/test_edge_k_schedule.py) all include this file. Nothing here needs a device: it compiles with any C++14 host compiler.
//
// A batch element of length k - k >= 64, k % 8 == 0, k % 64 != 0 - is read as ceil(k / 64) chunks of 64 k-values. Chunk c < last starts
// at 64 c. The LAST chunk is SHIFTED BACK to start at k - 64: it ends exactly at k, so no load leaves [0, k), and it holds again the
// o = 64 - k % 64 k-values that the chunk before it already multiplied. The MFMA waves SKIP those: a k-block is 8 k-values (one
// ds_read_b128 of A, four B values per lane, four v_mfma_f32_32x32x2_f32), o is a multiple of 8, so exactly the first o / 8 k-blocks
// of the last chunk are not multiplied - skipped, not multiplied by zero: an Inf in the overlap counts once, as data.
#pragma once

namespace tpp {

constexpr int KEDGE_BK = 64; // k per chunk (= LW_BK)
constexpr int KEDGE_KB = 8;  // k per k-block

// the lengths the schedule takes
constexpr bool kedge_k_ok(long long k) { return k >= KEDGE_BK && k % KEDGE_KB == 0 && k % KEDGE_BK != 0; }
// chunks per batch element
constexpr int kedge_chunks(int k) { return (k + KEDGE_BK - 1) / KEDGE_BK; }
// o: the k-values at the head of the last chunk that the chunk before it has already multiplied
constexpr int kedge_overlap(int k) { return KEDGE_BK - k % KEDGE_BK; }
// first k of chunk c (0 <= c < kedge_chunks(k))
constexpr int kedge_chunk_start(int k, int c) { return c + 1 < kedge_chunks(k) ? KEDGE_BK * c : k - KEDGE_BK; }
// k-blocks at the head of chunk c that are not multiplied
constexpr int kedge_skip_blocks(int k, int c) { return c + 1 < kedge_chunks(k) ? 0 : kedge_overlap(k) / KEDGE_KB; }
// does k-block kb (0 .. 7) of a chunk with `skip` skipped blocks run? K group wk of WK owns blocks wk * (8 / WK) .. of every chunk and
// asks per block, so what a group keeps of its share is a suffix of it - possibly nothing (it still takes the chunk's barrier)
constexpr bool kedge_block_runs(int kb, int skip) { return kb >= skip; }
// the loader's advance from chunk c to chunk c + 1 of the same batch element (c + 1 < kedge_chunks(k)), in k-values: 64, and k % 64
// into the last chunk; behind the last chunk comes the batch wrap: the element's stride less kedge_chunk_start(k, last)
constexpr int kedge_step(int k, int c) { return kedge_chunk_start(k, c + 1) - kedge_chunk_start(k, c); }

} // namespace tpp
