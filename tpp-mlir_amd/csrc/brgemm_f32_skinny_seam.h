// brgemm_f32_skinny_seam.h - the consumer's side of a seam of a skinny-batch f32 layer chain, and how its kernels read their argument block:
// moved here as they stood from brgemm_f32_skinny_chain.hip, which shares them with brgemm_f32_skinny_chain_split.hip. Device code only.
#pragma once
#include "brgemm_f32_skinny_tile.h"
#include "chain_args.h"

namespace tpp {

typedef __attribute__((address_space(1))) unsigned int skfc_gu32;
// the argument block, read where it lies (kernarg segment): the layer table is indexed at run time
typedef const __attribute__((address_space(4))) ChainArgs skfc_kernarg_t;

// the consumer's side of the seam, as the tile's K loop calls it between the B and the A loads of its first ring slots: wave 0 polls,
// everybody meets the barrier (brgemm_f32_skinny_chain.hip's header). wait = false: a later block of the layer - the seam is open already,
// no barrier
struct SkfcSeam {
  const unsigned *cnt;
  unsigned *err;
  unsigned target;
  int layer, wave, lane;
  bool wait;
  __device__ __forceinline__ void operator()() const {
    if (!wait) return;
    if (wave == 0) {
      skfc_gu32 *c = (skfc_gu32 *)cnt;
      const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
      for (;;) {
        const unsigned v = __hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((int)(v - target) >= 0) break;
        if (__builtin_amdgcn_s_memrealtime() - t0 > CHAIN_TIMEOUT_TICKS) { // never hang the GPU: flag it and go on
          if (lane == 0) __hip_atomic_store((skfc_gu32 *)err, 1u + (unsigned)layer, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          break;
        }
        __builtin_amdgcn_s_sleep(1);
      }
    }
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); // (no instruction: the A loads behind it stay behind the poll)
  }
};

// the argument block's address, opaque to the compiler from here on: what is read through the result is loaded HERE, not ahead of the K
// loop in front - the layer's facts would otherwise all stay in scalar registers across it (brgemm_bf16_skinny_chain.hip skc_args_again)
template <class Args> __device__ __forceinline__ Args *skfc_args_again(Args *pp) {
  asm volatile("" : "+s"(pp));
  return pp;
}

} // namespace tpp
