// brgemm_bf16_lw_kedge.h - the schedule of a RAGGED-k batch element on the bf16 loader-wave tiles (brgemm_bf16_lw.hip GRP = 4, opt-in:
// xsmm_hip_set_edge_k_bf16), written once as plain functions: the kernel, its launcher, the planner (gemm_plan.cpp) and a CPU test
// (tests/test_edge_k_bf16_schedule.py) all include this file. Nothing here needs a device: it compiles with any C++14 host compiler.
//
// A batch element of length k - k >= 64, k % 16 == 0, k % 64 != 0 - is read as ceil(k / 64) chunks of 64 k-values. Chunk c < last starts
// at 64 c. The LAST chunk is SHIFTED BACK to start at k - 64: it ends exactly at k, so no load leaves [0, k), and it holds again the
// o = 64 - k % 64 k-values (16, 32 or 48) that the chunk before it already multiplied. The MFMA waves SKIP those: a k-step is 16
// k-values (one v_mfma_f32_32x32x16_bf16 per accumulator), so exactly the first o / 16 k-steps of the last chunk are not multiplied -
// skipped, not multiplied by zero: an Inf in the overlap counts once, as data. (The f32 tiles' schedule, with its 8-k blocks, is
// brgemm_f32_lw_kedge.h.)
#pragma once

namespace tpp {

constexpr int BKEDGE_BK = 64; // k per chunk (= BLW_BK)
constexpr int BKEDGE_KS = 16; // k per k-step
constexpr int BKEDGE_STEPS = BKEDGE_BK / BKEDGE_KS; // k-steps per chunk

// the lengths the schedule takes
constexpr bool bkedge_k_ok(long long k) { return k >= BKEDGE_BK && k % BKEDGE_KS == 0 && k % BKEDGE_BK != 0; }
// chunks per batch element
constexpr int bkedge_chunks(int k) { return (k + BKEDGE_BK - 1) / BKEDGE_BK; }
// o: the k-values at the head of the last chunk that the chunk before it has already multiplied
constexpr int bkedge_overlap(int k) { return BKEDGE_BK - k % BKEDGE_BK; }
// first k of chunk c (0 <= c < bkedge_chunks(k))
constexpr int bkedge_chunk_start(int k, int c) { return c + 1 < bkedge_chunks(k) ? BKEDGE_BK * c : k - BKEDGE_BK; }
// k-steps at the head of chunk c that are not multiplied
constexpr int bkedge_skip_steps(int k, int c) { return c + 1 < bkedge_chunks(k) ? 0 : bkedge_overlap(k) / BKEDGE_KS; }
// does k-step s (0 .. 3) of a chunk with `skip` skipped steps run? K group wk of WK owns steps wk * (4 / WK) .. of every chunk and asks
// per step, so what a group keeps of its share is a suffix of it - possibly nothing (it still takes the chunk's barrier)
constexpr bool bkedge_step_runs(int s, int skip) { return s >= skip; }
// the loader's advance from chunk c to chunk c + 1 of the same batch element (c + 1 < bkedge_chunks(k)), in k-values: 64, and k % 64
// into the last chunk; behind the last chunk comes the batch wrap: the element's stride less bkedge_chunk_start(k, last)
constexpr int bkedge_step(int k, int c) { return bkedge_chunk_start(k, c + 1) - bkedge_chunk_start(k, c); }

// HALF STEPS (brgemm_bf16_lw.hip GRP = 6, opt-in: xsmm_hip_set_edge_k8_bf16; tests/test_edge_k8_bf16_schedule.py): k >= 64, k % 8 == 0,
// k % 16 != 0 (1000, 200, 72). Chunk count, chunk start, overlap and the loader's steps are the functions above (a shifted start k - 64 is
// still 16 bytes into an A row and a whole number of pair-rows / VNNI-4 group rows / flat rows of B). The overlap o is now an ODD multiple
// of 8 (8, 24, 40, 56): o / 16 whole k-steps of the last chunk plus the LOWER half of one more are multiplied already. In every operand
// fragment lanes 0 .. 31 hold k-values 0 .. 7 of a k-step and lanes 32 .. 63 hold 8 .. 15, so in that one step the MFMA's operands are
// zero in lanes 0 .. 31, on BOTH sides: the half contributes +0.0 products, and an Inf or NaN in it counts once, as data.
constexpr int BKEDGE8_KH = 8; // k per half step
constexpr bool bkedge8_k_ok(long long k) { return k >= BKEDGE_BK && k % BKEDGE8_KH == 0 && k % BKEDGE_KS != 0; }
// half steps at the head of chunk c that are not multiplied (odd on a last chunk: 1, 3, 5 or 7)
constexpr int bkedge8_skip_halves(int k, int c) { return c + 1 < bkedge_chunks(k) ? 0 : bkedge_overlap(k) / BKEDGE8_KH; }
// what k-step s (0 .. 3) of a chunk with `skip_halves` skipped half steps does: BKEDGE8_NONE not run, BKEDGE8_UPPER its upper eight
// k-values only (lanes 32 .. 63), BKEDGE8_WHOLE all sixteen
constexpr int BKEDGE8_NONE = 0, BKEDGE8_UPPER = 1, BKEDGE8_WHOLE = 2;
constexpr int bkedge8_step_part(int s, int skip_halves) {
  return 2 * s + 2 <= skip_halves ? BKEDGE8_NONE : 2 * s + 1 == skip_halves ? BKEDGE8_UPPER : BKEDGE8_WHOLE;
}

} // namespace tpp
