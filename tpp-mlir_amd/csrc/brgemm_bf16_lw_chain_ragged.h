// brgemm_bf16_lw_chain_ragged.h - the per-layer schedule of a RAGGED-WIDTH layer chain on the bf16 loader-wave tiles (brgemm_bf16_lw.hip
// GRP = 8, opt-in: xsmm_hip_set_chain_ragged), written once as plain functions: the loader, the MFMA loop, the launcher
// (brgemm_bf16_lw_chain_ragged.hip), the planner (gemm_plan.cpp plan_chain_ragged) and a CPU test (tests/test_chain_ragged_schedule.py) all
// include this file. Nothing here needs a device: it compiles with any C++14 host compiler.
//
// A chain of L layers on ceil(m / BM) x ceil(n / BN) co-resident workgroups. Rows: brgemm_bf16_lw_chain_edge.h (the last row block shifted
// back, two counters at a seam). Columns: the last column tile shifted back to start at n - BN, storing its own columns only. k, per layer:
// k >= 64 and k % 8 == 0 - whole (k % 64 == 0), in whole k-steps (k % 16 == 0) or in half steps (k % 16 == 8). A batch element is
// bkedge_chunks(k) chunks of 64 k-values, the last one shifted back to start at k - 64 (brgemm_bf16_lw_kedge.h); the MFMA waves skip the
// half steps (8 k-values) at its head that the chunk before it multiplied: none for a whole k, an even count for k % 16 == 0, an odd one for
// k % 16 == 8. Layer l is T(l) = br(l) * bkedge_chunks(k(l)) chunks, chunk c of it batch element c / chunks, chunk c % chunks of that
// element. THE RING is carried through the layers: chunk c of layer l lies in slot (s0(l) + c) % NSLOT, s0(0) = 0 and
// s0(l + 1) = (s0(l) + T(l)) % NSLOT - a layer may start at ANY slot. The B loader does not run ahead across a seam in this mode: every
// layer's first request goes to s0(l), from both loaders.
#pragma once
#include "brgemm_bf16_lw_kedge.h"

namespace tpp {

// the lengths a layer of a ragged-width chain takes
constexpr bool chain_ragged_k_ok(long long k) { return k >= BKEDGE_BK && k % BKEDGE8_KH == 0; }
// chunks per batch element / per layer
constexpr int chain_ragged_chunks(int k) { return bkedge_chunks(k); }
constexpr int chain_ragged_layer_chunks(int k, int br) { return br * bkedge_chunks(k); }
// chunk c of a layer (0 <= c < chain_ragged_layer_chunks): its batch element, its index in that element, its first k
constexpr int chain_ragged_batch(int k, int c) { return c / bkedge_chunks(k); }
constexpr int chain_ragged_chunk_in_batch(int k, int c) { return c % bkedge_chunks(k); }
constexpr int chain_ragged_chunk_k0(int k, int c) { return bkedge_chunk_start(k, c % bkedge_chunks(k)); }
// half steps at the head of a batch element's LAST chunk that are not multiplied: 0 for a whole k (bkedge_overlap would say 64: there is
// no overlap), 2, 4, 6 for k % 16 == 0, 1, 3, 5, 7 for k % 16 == 8
constexpr int chain_ragged_layer_skip(int k) { return k % BKEDGE_BK == 0 ? 0 : bkedge_overlap(k) / BKEDGE8_KH; }
// ... of chunk c of a layer: the layer's skip on a last chunk, 0 on every other
constexpr int chain_ragged_skip_halves(int k, int c) { return c % bkedge_chunks(k) + 1 == bkedge_chunks(k) ? chain_ragged_layer_skip(k) : 0; }
// The K loop counts chunks up to the next one it must TEST (a last chunk with skipped halves) and runs the chunks in between through the
// plain chain's untested bodies: every bkedge_chunks(k) chunks in a ragged layer - and never in a whole-k layer of T chunks, whose last
// chunks skip nothing (measured on 1024 rows x [1024, 1000, 1000], layer 0 sixteen one-chunk batch elements: 17.64 us per step with every
// chunk through the tested bodies, 14.87 this way)
constexpr int chain_ragged_test_period(int k, int T) { return chain_ragged_layer_skip(k) == 0 ? T + 1 : bkedge_chunks(k); }
// what k-step s (0 .. 3) of chunk c does: bkedge8_step_part (BKEDGE8_NONE / _UPPER / _WHOLE) - with 0 skipped halves WHOLE for every step
constexpr int chain_ragged_step_part(int k, int c, int s) { return bkedge8_step_part(s, chain_ragged_skip_halves(k, c)); }
// the ring: slot of the chunk after the one in `slot`; slot of the next layer's chunk 0; slot of chunk c of a layer that starts at s0
constexpr int chain_ragged_next_slot(int slot, int nslot) { return slot + 1 == nslot ? 0 : slot + 1; }
constexpr int chain_ragged_next_s0(int s0, int k, int br, int nslot) { return (s0 + chain_ragged_layer_chunks(k, br)) % nslot; }
constexpr int chain_ragged_slot(int s0, int c, int nslot) { return (s0 + c) % nslot; }
// s0 of layer l given the layers before it
constexpr int chain_ragged_s0(int l, const int *k, const int *br, int nslot) {
  int s0 = 0;
  for (int i = 0; i < l; ++i) s0 = chain_ragged_next_s0(s0, k[i], br[i], nslot);
  return s0;
}
// column tiles of n columns on tiles of bn columns; first column of tile tn (the last one shifted back); first column tile tn stores,
// relative to that
constexpr int chain_ragged_tiles_n(int n, int bn) { return (n + bn - 1) / bn; }
constexpr int chain_ragged_col0(int tn, int n, int bn) { return (tn + 1) * bn > n ? n - bn : tn * bn; }
constexpr int chain_ragged_own_col(int tn, int n, int bn) { return tn * bn - chain_ragged_col0(tn, n, bn); }

} // namespace tpp
