// brgemm_f32_skinny_chain.h - the schedule of a skinny-batch f32 LAYER CHAIN in one launch (brgemm_f32_skinny_chain.hip, opt-in:
// xsmm_hip_set_chain_skinny_f32), on top of brgemm_f32_skinny.h. Ownership (workgroup w of G owns the column blocks w, w + G, .. of
// skf_blocks(n_l, BN)), arrivals (one counter per seam, a launch adds exactly G), targets (epoch * G) and the counter-block key
// ((stream, 1, G, nlayers)) do not depend on the data type: they are the skc_* functions of brgemm_bf16_skinny_chain.h, used as they are.
// f32's own: which waves of the launch take steps in a layer - the single call's deal, skf_waves / skf_wave_first / skf_wave_count - and
// what the launcher refuses of a layer's leading dimensions. The kernel, its launcher, the planner (gemm_plan.cpp plan_chain_skinny_f32)
// and a CPU test (tests/test_chain_skinny_f32_cpu.py) include this file. Nothing here needs a device: it compiles with any C++14 host
// compiler.
#pragma once
#include "brgemm_bf16_skinny_chain.h"
#include "brgemm_f32_skinny.h"

namespace tpp {

// WAVES: of a layer (W_l, the single call's), and a wave's run in it - nothing for a wave at or beyond W_l. The launch has the waves of
// its deepest layer.
constexpr int skfc_layer_waves(long long br, int k) { return skf_waves(br * skf_steps(k)); }
constexpr int skfc_wave_count(int wave, long long br, int k) {
  return wave < skfc_layer_waves(br, k) ? skf_wave_count(wave, skfc_layer_waves(br, k), (int)(br * skf_steps(k))) : 0;
}
constexpr int skfc_wave_first(int wave, long long br, int k) {
  return wave < skfc_layer_waves(br, k) ? skf_wave_first(wave, skfc_layer_waves(br, k), (int)(br * skf_steps(k))) : 0;
}

// What the launcher refuses of one layer besides skf_shape_ok and the pointers: leading dimensions that do not cover the layer, a leading
// dimension or stride that is negative or no multiple of 4 elements, and offsets a 32-bit buffer offset cannot hold. The handed-off A and
// every C are addressed through buffer resources of 2^31 - 1 bytes; the largest byte offset formed is 4 * (31 * ld + n) - row 30 at most,
// the piece's last byte included, and for A the batch elements stay inside the row (the launcher's check), so n stands for k <= ld there.
// THE BOUND: with n <= ld that is at most 4 * 32 * ld = 128 ld, below 2^31 exactly when ld < 2^24.
constexpr long long SKFC_LD_MAX = 1LL << 24;
constexpr bool skfc_ld_ok(long long lda, long long ldb, long long ldc, long long stride_a, long long stride_b, long long n, long long k) {
  return lda >= k && ldb >= n && ldc >= n && !((lda | ldb | ldc | stride_a | stride_b) & 3) && stride_a >= 0 && stride_b >= 0 && ldb >= 0 && lda < SKFC_LD_MAX &&
         ldc < SKFC_LD_MAX;
}
static_assert(4 * (31 * (SKFC_LD_MAX - 4) + (SKFC_LD_MAX - 4)) < (1LL << 31), "the largest admitted leading dimension keeps every buffer offset below 2^31");

} // namespace tpp
