// brgemm_bf16_skinny_chain.hip - a CHAIN of skinny-batch bf16 layers (1 .. 31 rows) in ONE launch (opt-in: xsmm_hip_set_chain_skinny): the
// unsplit skinny kernel (brgemm_bf16_skinny.hip) with a layer loop and a block loop around its body. G resident workgroups; in layer l
// workgroup w takes the column blocks w, w + G, .. of that layer's n_l columns (the schedule: brgemm_bf16_skinny_chain.h, walked on a CPU by
// tests/test_chain_skinny_map.py). A block is the single call's: the same load maps, ragged-k mask, ring of SKN_DEPTH steps, deal of the
// layer's steps over W_l = skn_waves(br_l * skn_steps(k_l)) waves, LDS combine into wave 0 in wave order, bias, relu and ONE rounding - bit
// for bit the call under xsmm_hip_set_skinny_bf16(BN). The launch has the waves of its deepest layer; a wave at or beyond W_l takes no step
// in layer l but meets every barrier.
// The K loop and the epilogue (brgemm_bf16_skinny_chain_body.h) and the combine below are the chain's own text of what brgemm_bf16_skinny_tile.h
// holds for the unsplit and the split kernel. Built from that tile (sc1 loads of A and the seam wait as a hook in its K loop, sc1 stores in its epilogue) every result
// bit was the same, but a forced BN 64 launch measured 2 .. 4 % slower than this text (profiles/skinny_tile_refactor_ab.txt, part 4), and
// the cause was not found. Until it is, a change to the tile's K loop, combine or epilogue has to be made here too: the GPU tests compare
// the chain with the calls bit for bit (tests/test_chain_skinny_gpu.py).
//
// THE SEAM between layer l and l + 1 is the project's chain protocol (brgemm_bf16_lw.hip's header; guide: Guideline 16, recipe R1) on ONE
// counter per seam, cnt[l]. No memset, no reset: counters only grow, a launch adds exactly G to each, the host passes target = epoch * G.
//   producer: EVERY store of C is write-through - raw buffer stores of 2 / 4 / 8 bytes with aux 16 (sc1); the last layer's too, it has no
//             other store path -. Only wave 0 stores, so no other wave's drain is owed: wave 0 executes s_waitcnt vmcnt(0) behind the
//             stores of the workgroup's LAST block of the layer, then its lane 0 adds 1 to cnt[l] (relaxed, agent scope). A workgroup
//             that owns no block of the layer arrives at once.
//   consumer: in front of the first block of a layer l > 0, wave 0 polls cnt[l - 1] (relaxed agent-scope load, s_sleep) until it reaches
//             the target; the spin is bounded by CHAIN_TIMEOUT_TICKS of s_memrealtime and on a timeout writes 1 + l to *err and carries
//             on (wrong numbers, never a hung GPU). Then a workgroup barrier. EVERY load of a handed-off activation - A of a layer
//             l > 0 - is an sc1 buffer load to registers (aux 16: the CU's L1 is bypassed), so the recipe's agent-scope acquire is
//             DROPPED (checked in the .s along every path: profiles/chain_skinny_isa.txt). A of layer 0, B and the bias are plain loads
//             of bytes nobody writes in the launch.
//   weights ahead of the wait: the B loads of a wave's first SKN_DEPTH ring slots are issued BEFORE the poll, the A loads of those slots
//             behind the barrier - weights do not depend on activations. It changes no bit and costs no register.
// LDS: part[] is written by waves 1 .. W_l - 1 in front of the block's first barrier and read by wave 0 behind it; a second barrier
// behind wave 0's reads frees it for the next block, whose K loop the other waves may already have finished.
// PROGRESS: G is at most the stream's compute units (the caller's guarantee, gemm_plan.cpp plan_chain_skinny) and a workgroup of at
// most 512 threads with less than 64 KiB of LDS fits one to a compute unit, so all G workgroups are resident at once. A workgroup waits
// only for arrivals at the seam of an EARLIER layer, and every workgroup makes each of its arrivals unconditionally after work that
// itself waits only for still earlier seams: by induction over the layers no wait is cyclic. Every spin is bounded.
#include "brgemm_bf16_skinny_chain_body.h"

namespace tpp {

static_assert(SKC_MAXL == CH_MAXL, "the schedule's layer count is the launch's");

// SknStep, skc_seam_wait, skc_k_loop, skc_epilogue and skc_args_again: brgemm_bf16_skinny_chain_body.h (shared with brgemm_bf16_skinny_chain_split.hip)

template <int IMG, int BN, int MB> __global__ __launch_bounds__(64 * SKN_WMAX) void brgemm_bf16_skinny_chain(ChainArgs p_by_value) {
  skc_kernarg_t *const pp = (skc_kernarg_t *)__builtin_amdgcn_kernarg_segment_ptr(); // = &p_by_value (the only explicit argument)
  constexpr int C = skn_cols(BN), SETS = MB / 16;
  constexpr int NACC = SETS * C * 4;
  __shared__ float part[(SKN_WMAX - 1) * NACC * 64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int w = (int)blockIdx.x;

  for (int l = 0; l < pp->nlayers; ++l) {
    // this workgroup's blocks of the layer: w, w + G, .. (skc_block) - none if w is at or beyond the layer's blocks (skc_owned)
    if (w >= skn_blocks(pp->L[l].pad, BN)) { // the layer is sat out: arrive at once (nothing of this workgroup's is owed)
      if (skc_signals(l, pp->nlayers) && threadIdx.x == 0)
        __hip_atomic_fetch_add((skc_gu32 *)(pp->cnt + (size_t)l * CHAIN_CNT_STRIDE), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      continue;
    }
    for (int blk = w;;) {
      f32x4 acc[SETS][C];
      {
        skc_kernarg_t &p = *skc_args_again(pp);
        SkcLayer a;
        a.A = l == 0 ? p.A : p.L[l - 1].C;
        a.lda = l == 0 ? p.lda : p.L[l - 1].ldc;
        a.B = p.L[l].B, a.D = nullptr, a.C = nullptr;
        a.ldb = p.L[l].ldb, a.ldc = 0, a.stride_a = p.L[l].stride_a, a.stride_b = p.L[l].stride_b;
        a.m = p.m, a.n = p.L[l].pad, a.k = p.L[l].k, a.br = p.L[l].br, a.ep = 0;
        const int cnt = skc_wave_count(wave, a.br, a.k), t0 = skc_wave_first(wave, a.br, a.k);
        const int n0 = skn_origin(blk, a.n, BN);
        const unsigned *const seam = p.cnt + (size_t)(l > 0 ? l - 1 : 0) * CHAIN_CNT_STRIDE;
        if (l == 0) skc_k_loop<IMG, BN, MB, false>(a, lane, wave, n0, t0, cnt, false, seam, p.target, p.err, l, acc);
        else skc_k_loop<IMG, BN, MB, true>(a, lane, wave, n0, t0, cnt, blk == w, seam, p.target, p.err, l, acc);
      }
      skc_kernarg_t &p = *skc_args_again(pp);
      const int W = skc_layer_waves(p.L[l].br, p.L[l].k);
      // the partial accumulators through LDS, added by wave 0 in wave order
      if (wave > 0 && wave < W) {
#pragma unroll
        for (int s = 0; s < SETS; ++s)
#pragma unroll
          for (int j = 0; j < C; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) part[((wave - 1) * NACC + (s * C + j) * 4 + r) * 64 + lane] = acc[s][j][r];
      }
      __syncthreads();
      if (wave == 0)
        for (int ww = 1; ww < W; ++ww)
#pragma unroll
          for (int s = 0; s < SETS; ++s)
#pragma unroll
            for (int j = 0; j < C; ++j)
#pragma unroll
              for (int r = 0; r < 4; ++r) acc[s][j][r] += part[((ww - 1) * NACC + (s * C + j) * 4 + r) * 64 + lane];
      __syncthreads(); // part[] is free again: the other waves may be a whole K loop ahead
      const int next = blk + p.groups, blocks = skn_blocks(p.L[l].pad, BN);
      if (wave == 0) {
        SkcLayer a{};
        a.D = p.L[l].D, a.C = p.L[l].C, a.ldc = p.L[l].ldc;
        a.m = p.m, a.n = p.L[l].pad, a.ep = p.L[l].ep;
        skc_epilogue<BN, MB>(a, lane, blk, skn_origin(blk, a.n, BN), acc);
        if (skc_signals(l, p.nlayers) && next >= blocks) { // the producer's side of the seam, behind the LAST block: only this wave stored
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          if (lane == 0) __hip_atomic_fetch_add((skc_gu32 *)(p.cnt + (size_t)l * CHAIN_CNT_STRIDE), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      if (next >= blocks) break;
      blk = next;
    }
  }
}

template <int IMG, int BN> static hipError_t launch_bf16_skinny_chain_t(const ChainArgs &a, int waves, hipStream_t s) {
  const dim3 grid(a.groups), block(64 * waves);
  if (skn_mb(a.m) == 16) hipLaunchKernelGGL((brgemm_bf16_skinny_chain<IMG, BN, 16>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((brgemm_bf16_skinny_chain<IMG, BN, 32>), grid, block, 0, s, a);
  return hipGetLastError();
}

// A chain of a.nlayers skinny-batch layers on a.groups = G resident workgroups, G at most the stream's compute units - the caller's
// guarantee; layer l has a.L[l].pad columns. Refuses with hipErrorInvalidValue, launching nothing, everything the kernel does not assume:
// per layer what launch_bf16_skinny refuses of the same call (an instance; skn_shape_ok; leading dimensions that cover the layer; leading
// dimensions and strides in multiples of 8 elements; A, B and C 16-byte and the bias row 8-byte aligned; no VNNI C), a beta 1, a leading
// dimension of A or C of 2^24 elements or more (buffer offsets), a later layer whose batch elements leave the rows of its input, fewer than
// 2 or more than CH_MAXL layers, G < 1, no counters or no error word.
// (the list as a function: launch_bf16_skinny_chain_split, brgemm_bf16_skinny_chain_split.hip, refuses the same)
bool bf16_skinny_chain_args_ok(int b_kind, int bn, const ChainArgs &a) {
  if (!skn_instance_exists(b_kind, bn) || !skc_launch_shape_ok(a.nlayers, a.groups) || !a.cnt || !a.err || !a.A || ((uintptr_t)a.A & 15)) return false;
  for (int l = 0; l < a.nlayers; ++l) {
    const ChainLayer &L = a.L[l];
    const int64_t lda = l == 0 ? a.lda : a.L[l - 1].ldc;
    if (!skn_shape_ok(a.m, L.pad, L.k, L.br, bn) || !skc_ld_ok(lda, L.ldb, L.ldc, L.stride_a, L.stride_b, L.pad, L.k)) return false;
    if (!(L.ep & EP_BETA0) || (L.ep & EP_VNNI_C) || !L.B || !L.C || (((uintptr_t)L.B | (uintptr_t)L.C) & 15)) return false;
    if ((L.ep & EP_BIAS) && (!L.D || ((uintptr_t)L.D & 7))) return false;
    if (l > 0 && (int64_t)(L.br - 1) * L.stride_a + L.k > lda) return false;
  }
  return true;
}
hipError_t launch_bf16_skinny_chain(int b_kind, int bn, const ChainArgs &a, hipStream_t s) {
  if (!bf16_skinny_chain_args_ok(b_kind, bn, a)) return hipErrorInvalidValue;
  int waves = 1;
  for (int l = 0; l < a.nlayers; ++l) waves = std::max(waves, skc_layer_waves(a.L[l].br, a.L[l].k));
  switch (b_kind * 100 + bn) {
  case 16: return launch_bf16_skinny_chain_t<0, 16>(a, waves, s);
  case 32: return launch_bf16_skinny_chain_t<0, 32>(a, waves, s);
  case 64: return launch_bf16_skinny_chain_t<0, 64>(a, waves, s);
  case 232: return launch_bf16_skinny_chain_t<2, 32>(a, waves, s);
  case 264: return launch_bf16_skinny_chain_t<2, 64>(a, waves, s);
  case 416: return launch_bf16_skinny_chain_t<4, 16>(a, waves, s);
  case 432: return launch_bf16_skinny_chain_t<4, 32>(a, waves, s);
  case 464: return launch_bf16_skinny_chain_t<4, 64>(a, waves, s);
  }
  return hipErrorInvalidValue;
}

} // namespace tpp
