// brgemm_bf16_skinny_chain.h - the schedule of a skinny-batch bf16 LAYER CHAIN in one launch (brgemm_bf16_skinny_chain.hip, opt-in:
// xsmm_hip_set_chain_skinny), on top of brgemm_bf16_skinny.h: which column blocks of which layer a workgroup owns, when it arrives at a
// seam and what a consumer waits for, which waves of the launch take steps in a layer, and what the launcher refuses. The kernel, its
// launcher, the planner (gemm_plan.cpp plan_chain_skinny) and a CPU test (tests/test_chain_skinny_map.py) all include this file. Nothing
// here needs a device: it compiles with any C++14 host compiler.
//
// G resident workgroups run every layer of the chain, layer by layer. In layer l, with n_l columns in skn_blocks(n_l, BN) column blocks,
// workgroup w owns the blocks b = w, w + G, .. - none where w is at or beyond the block count. A block is the unsplit kernel's: skn_origin
// / skn_skip place it and say what it stores, and the layer's S_l = br_l * skn_steps(k_l) steps are dealt over W_l = skn_waves(S_l) waves
// by skn_wave_first / skn_wave_count - an element's chain of additions is the single call's. The launch has the waves of its deepest
// layer; waves at or beyond W_l take no step in layer l.
// THE SEAM between layer l and l + 1 is ONE counter, cnt[l]: every workgroup adds 1 to it exactly once per launch - behind the stores of
// its last block of layer l, at once if it owns none - so a launch adds exactly G, and a consumer of epoch e waits for e * G.
#pragma once
#include "brgemm_bf16_skinny.h"

namespace tpp {

constexpr int SKC_MAXL = 8;    // layers per launch (= CH_MAXL, chain_args.h: the launcher asserts it)
constexpr int SKC_GMAX = 512;  // most resident workgroups a mode can force (xsmm_hip_set_chain_skinny: 1000 * G + BN)

// OWNERSHIP: blocks of layer l that workgroup w of G owns, the i-th of them, and the owner of block b
constexpr int skc_owned(int w, int G, int blocks) { return w < blocks ? (blocks - 1 - w) / G + 1 : 0; }
constexpr int skc_block(int w, int G, int i) { return w + i * G; }
constexpr int skc_owner(int b, int G) { return b % G; }
// G by rule: a workgroup per block of the widest layer, at most the compute units (every workgroup must be resident)
constexpr int skc_groups(int max_blocks, long long cus) { return max_blocks < cus ? max_blocks : (int)cus; }
// ARRIVALS: workgroup w signals seam l (0 <= l < nlayers - 1) once, behind block index skc_owned - 1 of its walk (-1: at the layer's start)
constexpr bool skc_signals(int l, int nlayers) { return l + 1 < nlayers; }
constexpr int skc_arrive_after(int w, int G, int blocks) { return skc_owned(w, G, blocks) - 1; }
constexpr unsigned skc_arrivals(int G) { return (unsigned)G; }                              // what one launch adds to every seam counter
constexpr unsigned skc_target(unsigned epoch, int G) { return epoch * (unsigned)G; }        // what the consumers of launch `epoch` wait for
// a workgroup WAITS in front of layer l > 0 only if it owns a block there (it then reads the layer's A, every column of it)
constexpr bool skc_waits(int w, int G, int l, int blocks) { return l > 0 && skc_owned(w, G, blocks) > 0; }
// WAVES: of a layer, and of the launch (the deepest layer's)
constexpr int skc_layer_waves(long long br, int k) { return skn_waves(br * skn_steps(k)); }
constexpr int skc_wave_count(int wave, long long br, int k) {
  return wave < skc_layer_waves(br, k) ? skn_wave_count(wave, skc_layer_waves(br, k), (int)(br * skn_steps(k))) : 0;
}
constexpr int skc_wave_first(int wave, long long br, int k) {
  return wave < skc_layer_waves(br, k) ? skn_wave_first(wave, skc_layer_waves(br, k), (int)(br * skn_steps(k))) : 0;
}
// THE COUNTER BLOCK (rt_chain.h chain_block): keyed (stream, row blocks = 1, column tiles = G, layers) - the key of a plain chain with one
// row block and G column tiles, which adds the same G to the same nlayers - 1 counters per launch: the two forms share the block, and
// the epoch order under the block's mutex is their stream order (tests/test_chain_skinny_dispatch.py interleaves them).
constexpr int skc_key_tiles_m() { return 1; }
constexpr int skc_key_tiles_n(int G) { return G; }

// what the launcher refuses of one layer besides skn_shape_ok and the pointers: leading dimensions that do not cover the layer, or are no
// multiples of 8 elements, and offsets a 32-bit buffer offset cannot hold - the handed-off A and every C are addressed through buffer
// resources: 2 * (31 * ld + n) bytes must stay below 2^31
constexpr bool skc_ld_ok(long long lda, long long ldb, long long ldc, long long stride_a, long long stride_b, long long n, long long k) {
  return lda >= k && ldb >= n && ldc >= n && !((lda | ldb | ldc | stride_a | stride_b) & 7) && stride_a >= 0 && stride_b >= 0 && lda < (1LL << 24) &&
         ldc < (1LL << 24);
}
constexpr bool skc_launch_shape_ok(int nlayers, int G) { return nlayers >= 2 && nlayers <= SKC_MAXL && G >= 1; }

} // namespace tpp
