// brgemm_f32_skinny_chain.hip - a CHAIN of skinny-batch f32 layers (1 .. 31 rows) in ONE launch (opt-in: xsmm_hip_set_chain_skinny_f32): the
// unsplit f32 skinny kernel (brgemm_f32_skinny.hip) with a layer loop and a block loop around its body. G resident workgroups; in layer l
// workgroup w takes the column blocks w, w + G, .. of that layer's n_l columns (the schedule: brgemm_f32_skinny_chain.h on top of
// brgemm_bf16_skinny_chain.h, walked on a CPU by tests/test_chain_skinny_f32_cpu.py). A block is the single call's, and it is the single
// call's TEXT: skf_k_loop, skf_park, skf_gather and skf_epilogue of brgemm_f32_skinny_tile.h - the load maps, the flat B from global memory
// straight into the operands of v_mfma_f32_16x16x4_f32, the ring of SKF_DEPTH steps, the ragged-k mask, the deal of the layer's steps over
// W_l = skf_waves(br_l * skf_steps(k_l)) waves in contiguous runs, the LDS combine into wave 0 in wave order, bias, relu, the store - with
// the tile's chain parameters set (HANDED, the seam wait, SC1). Every layer is bit for bit the call under xsmm_hip_set_skinny_f32(BN) with
// the split off. The launch has the waves of its deepest layer; a wave at or beyond W_l takes no step in layer l but meets every barrier.
//
// THE SEAM between layer l and l + 1 is the project's chain protocol exactly as brgemm_bf16_skinny_chain.hip's header writes it down, on ONE
// counter per seam, cnt[l]. No memset, no reset: counters only grow, a launch adds exactly G to each, the host passes target = epoch * G.
//   producer: EVERY store of C is a write-through raw buffer store of 4 / 8 / 16 bytes with aux 16 (sc1), the last layer's too. Only wave 0
//             stores: it executes s_waitcnt vmcnt(0) behind the stores of the workgroup's LAST block of the layer, then its lane 0 adds 1
//             to cnt[l] (relaxed, agent scope). A workgroup that owns no block of the layer arrives at once.
//   consumer: in front of the first block of a layer l > 0, wave 0 polls cnt[l - 1] (relaxed agent-scope load, s_sleep) until it reaches
//             the target; the spin is bounded by CHAIN_TIMEOUT_TICKS of s_memrealtime and on a timeout writes 1 + l to *err and carries
//             on (wrong numbers, never a hung GPU). Then a workgroup barrier. EVERY load of a handed-off activation - A of a layer
//             l > 0 - is an sc1 raw buffer load of 16 bytes to registers (the CU's L1 is bypassed), so no acquire fence instruction
//             stands between the poll and those loads (checked in the .s: profiles/chain_skinny_f32_isa.txt). A of layer 0, B and the
//             bias are plain loads of bytes nobody writes in the launch.
//   weights ahead of the wait: the B loads of a wave's first SKF_DEPTH ring slots are issued BEFORE the poll, the A loads of those slots
//             behind the barrier.
// LDS: part[] is written by waves 1 .. in front of the block's first barrier (skf_park) and read by wave 0 behind it (skf_gather); a
// second barrier behind wave 0's reads frees it for the next block, whose K loop the other waves may already have finished.
// PROGRESS: G is at most the stream's compute units (the caller's guarantee, gemm_plan.cpp plan_chain_skinny_f32) and a workgroup of at
// most 512 threads with at most 56 KiB of static LDS fits one to a compute unit, so all G workgroups are resident at once. A workgroup
// waits only for arrivals at the seam of an EARLIER layer, and makes each of its arrivals unconditionally after work that itself waits
// only for still earlier seams: by induction over the layers no wait is cyclic. Every spin is bounded.
#include "brgemm_f32_skinny_seam.h"
#include "brgemm_f32_skinny_chain.h"

namespace tpp {

static_assert(SKC_MAXL == CH_MAXL, "the schedule's layer count is the launch's");

// SkfcSeam, the consumer's side of the seam, and skfc_args_again: brgemm_f32_skinny_seam.h (shared with brgemm_f32_skinny_chain_split.hip)

template <int BN, int MB> __global__ __launch_bounds__(64 * SKF_WMAX) void brgemm_f32_skinny_chain(ChainArgs p_by_value) {
  skfc_kernarg_t *const pp = (skfc_kernarg_t *)__builtin_amdgcn_kernarg_segment_ptr(); // = &p_by_value (the only explicit argument)
  constexpr int C = skf_cols(BN), SETS = MB / 16;
  constexpr int NACC = SETS * C * 4;
  __shared__ float part[(SKF_WMAX - 1) * NACC * 64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int w = (int)blockIdx.x;

  for (int l = 0; l < pp->nlayers; ++l) {
    // this workgroup's blocks of the layer: w, w + G, .. (skc_block) - none if w is at or beyond the layer's blocks (skc_owned)
    if (w >= skf_blocks(pp->L[l].pad, BN)) { // the layer is sat out: arrive at once (nothing of this workgroup's is owed)
      if (skc_signals(l, pp->nlayers) && threadIdx.x == 0)
        __hip_atomic_fetch_add((skfc_gu32 *)(pp->cnt + (size_t)l * CHAIN_CNT_STRIDE), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      continue;
    }
    for (int blk = w;;) {
      SkfAcc<BN, MB> acc;
      {
        skfc_kernarg_t &p = *skfc_args_again(pp);
        GemmArgs a{};
        a.A = l == 0 ? p.A : p.L[l - 1].C;
        a.lda = l == 0 ? p.lda : p.L[l - 1].ldc;
        a.B = p.L[l].B, a.ldb = p.L[l].ldb, a.stride_a = p.L[l].stride_a, a.stride_b = p.L[l].stride_b;
        a.m = p.m, a.n = p.L[l].pad, a.k = p.L[l].k, a.br = p.L[l].br;
        const int cnt = skfc_wave_count(wave, a.br, a.k), t0 = skfc_wave_first(wave, a.br, a.k);
        const int n0 = skf_origin(blk, a.n, BN);
        if (l == 0) {
          skf_k_loop<BN, MB>(a, lane, n0, t0, cnt, acc);
        } else {
          const SkfcSeam seam{p.cnt + (size_t)(l - 1) * CHAIN_CNT_STRIDE, p.err, p.target, l, wave, lane, blk == w};
          skf_k_loop<BN, MB, true, SkfcSeam>(a, lane, n0, t0, cnt, acc, seam);
        }
      }
      skf_park<BN, MB>(part, lane, wave, acc); // a wave without a step parks zeros nobody reads; ONE barrier
      skfc_kernarg_t &p = *skfc_args_again(pp);
      if (wave == 0) skf_gather<BN, MB>(part, lane, skfc_layer_waves(p.L[l].br, p.L[l].k), acc); // a fixed order of additions
      __syncthreads(); // part[] is free again: the other waves may be a whole K loop ahead
      const int next = blk + p.groups, blocks = skf_blocks(p.L[l].pad, BN);
      if (wave == 0) {
        GemmArgs a{};
        a.D = p.L[l].D, a.C = p.L[l].C, a.ldc = p.L[l].ldc;
        a.m = p.m, a.n = p.L[l].pad, a.ep = p.L[l].ep | EP_BETA0;
        skf_epilogue<BN, MB, true>(a, lane, blk, skf_origin(blk, a.n, BN), acc);
        if (skc_signals(l, p.nlayers) && next >= blocks) { // the producer's side of the seam, behind the LAST block: only this wave stored
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          if (lane == 0) __hip_atomic_fetch_add((skfc_gu32 *)(p.cnt + (size_t)l * CHAIN_CNT_STRIDE), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      if (next >= blocks) break;
      blk = next;
    }
  }
}

template <int BN> static hipError_t launch_f32_skinny_chain_t(const ChainArgs &a, int waves, hipStream_t s) {
  const dim3 grid(a.groups), block(64 * waves);
  if (skf_mb(a.m) == 16) hipLaunchKernelGGL((brgemm_f32_skinny_chain<BN, 16>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((brgemm_f32_skinny_chain<BN, 32>), grid, block, 0, s, a);
  return hipGetLastError();
}

// A chain of a.nlayers skinny-batch f32 layers on a.groups = G resident workgroups, G at most the stream's compute units - the caller's
// guarantee; layer l has a.L[l].pad columns. Refuses with hipErrorInvalidValue, launching nothing, everything the kernel does not assume:
// per layer what launch_f32_skinny refuses of the same call (skf_shape_ok; A, B, C and the bias row 16-byte aligned) and skfc_ld_ok
// (leading dimensions that cover the layer, leading dimensions and strides in multiples of 4 elements and not negative, a leading
// dimension of A or C of 2^24 elements or more), a beta 1 or a VNNI flag, a later layer whose batch elements leave the rows of its input,
// fewer than 2 or more than CH_MAXL layers, G < 1, no counters or no error word.
// (the list as a function: launch_f32_skinny_chain_split, brgemm_f32_skinny_chain_split.hip, refuses the same)
bool f32_skinny_chain_args_ok(int bn, const ChainArgs &a) {
  if (!skf_bn_ok(bn) || !skc_launch_shape_ok(a.nlayers, a.groups) || !a.cnt || !a.err || !a.A || ((uintptr_t)a.A & 15)) return false;
  for (int l = 0; l < a.nlayers; ++l) {
    const ChainLayer &L = a.L[l];
    const int64_t lda = l == 0 ? a.lda : a.L[l - 1].ldc;
    if (!skf_shape_ok(a.m, L.pad, L.k, L.br, bn) || !skfc_ld_ok(lda, L.ldb, L.ldc, L.stride_a, L.stride_b, L.pad, L.k)) return false;
    if (!(L.ep & EP_BETA0) || (L.ep & EP_VNNI_C) || !L.B || !L.C || (((uintptr_t)L.B | (uintptr_t)L.C) & 15)) return false;
    if ((L.ep & EP_BIAS) && (!L.D || ((uintptr_t)L.D & 15))) return false;
    if (l > 0 && (int64_t)(L.br - 1) * L.stride_a + L.k > lda) return false;
  }
  return true;
}
hipError_t launch_f32_skinny_chain(int bn, const ChainArgs &a, hipStream_t s) {
  if (!f32_skinny_chain_args_ok(bn, a)) return hipErrorInvalidValue;
  int waves = 1;
  for (int l = 0; l < a.nlayers; ++l) waves = std::max(waves, skfc_layer_waves(a.L[l].br, a.L[l].k));
  return bn == 16 ? launch_f32_skinny_chain_t<16>(a, waves, s) : bn == 32 ? launch_f32_skinny_chain_t<32>(a, waves, s) : launch_f32_skinny_chain_t<64>(a, waves, s);
}

} // namespace tpp
