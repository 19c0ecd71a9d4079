// brgemm_bf16_dma256_chain.hip - a CHAIN of whole-layer fused bf16 BRGEMMs in ONE launch on the 256 x 256 LDS-DMA tile (opt-in:
// xsmm_hip_set_chain_dma256): the large-shape counterpart of the chain mode of brgemm_bf16_lw.hip, for the batches whose calls run on this
// tile - 16384 rows x 1024 columns are exactly 256 tiles. The tile's text is brgemm_bf16_dma256_tile.h (CHAIN = true: one call of the body
// is one layer step); the workgroup map and the step walk are brgemm_bf16_dma256_chain.h / brgemm_bf16_lw_chain_rounds.h, walked on the CPU
// by tests/test_chain_dma256_schedule.py.
//
// Grid: G x tiles_n workgroups of 256 threads, all resident (one per CU by LDS: 128 KiB); G = tiles_m in a chain of one round, fewer row
// groups walk several row blocks each (the launcher's a.groups). Workgroup (g, tn) computes tile (tm, tn) of EVERY layer for its row blocks
// tm = g, g + G, .., layer-major; layer l > 0 reads L[l-1].C as its A with lda = L[l-1].ldc. The layer table is read where it lies, in the
// kernarg segment: a copy in registers does not fit beside 256 accumulators, one in scratch is what this kernel must not have.
//
// The seam between layer l and l + 1 is the chain protocol of brgemm_bf16_lw.hip (its head comment), on a kernel without loader waves:
//   producer: the tile is stored write-through (sc1 16-byte stores: the tile's C_STORE_AUX), EVERY wave drains s_waitcnt vmcnt(0), a
//             workgroup barrier - it also retires the epilogue's staging tiles, which lie in the ring slots the next prologue fills -,
//             one lane adds 1 to cnt[l][tm] (relaxed, agent scope, global address space).
//   consumer: one wave polls cnt[l-1][tm] (relaxed agent-scope load, s_sleep) until it has reached target = epoch * tiles_n - counters
//             only grow, nothing is reset between launches -, bounded by CHAIN_TIMEOUT_TICKS of s_memrealtime: on a timeout *err = 1 + l
//             and the step carries on (wrong numbers, never a hang; the host looks at *err at its synchronisation points). A workgroup
//             barrier, then the layer's whole prologue: no run-ahead across a seam. Every LDS-DMA load of an A panel carries sc1.
//   After a non-final step of the LAST layer there is nothing to publish: only the rendezvous barrier that retires the staging tiles.
// Results are bit for bit those of the same layers launched one by one on this tile (same tile, same k order, same rounding).
#include "brgemm_bf16_dma256_tile.h"
#include "brgemm_bf16_dma256_chain.h"
#include "chain_args.h"

namespace tpp {

static_assert(D256C_BM == D256_BM && D256C_BN == D256_BN && D256C_BK == D256_BK, "brgemm_bf16_dma256_chain.h counts tiles and chunks as the tile does");
typedef const __attribute__((address_space(4))) ChainArgs d256c_kernarg_t; // the argument block where it lies (chain_kernarg_t of brgemm_bf16_lw.hip)
typedef __attribute__((address_space(1))) unsigned int d256c_g_u32;

// the argument block through a pointer the compiler cannot see through: what is loaded behind it is loaded THERE, not in front of the K
// loop - whose scalar registers (addresses, wrap deltas, buffer descriptors) leave no room for values that are needed once per seam
__device__ __forceinline__ d256c_kernarg_t &d256c_args_here() {
  d256c_kernarg_t *pp = (d256c_kernarg_t *)__builtin_amdgcn_kernarg_segment_ptr(); // = &p_by_value (the only explicit argument)
  asm volatile("" : "+s"(pp));
  return *pp;
}

// (a scalar value likewise: a comparison written once in front of the layer loop is kept across it - as a vector register, which was spilled)
__device__ __forceinline__ int d256c_here(int v) {
  asm volatile("" : "+s"(v));
  return v;
}

template <int IMG> __device__ __forceinline__ void brgemm_bf16_dma256_chain_body() {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  int tn, tm, l = 0; // the walk: chain_rounds_next
  {
    d256c_kernarg_t &p = d256c_args_here();
    tn = d256c_col((int)blockIdx.x, p.groups, p.tiles_n);
    tm = d256c_group((int)blockIdx.x, p.groups, p.tiles_n);
  }
  for (;;) {
    {
      d256c_kernarg_t &p = d256c_args_here();
      const int lp = l > 0 ? l - 1 : 0;
      if (l > 0) {
        // every producer tile of the rows [256 tm, + 256) of layer l - 1 has been stored write-through and drained
        if (d256c_here(wave) == 0) {
          d256c_g_u32 *c = (d256c_g_u32 *)(p.cnt + d256c_counter(lp, tm, p.tiles_m, CHAIN_CNT_STRIDE));
          const unsigned target = p.target;
          const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
          for (;;) {
            const unsigned v = __hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((int)(v - target) >= 0) break;
            if (__builtin_amdgcn_s_memrealtime() - t0 > CHAIN_TIMEOUT_TICKS) { // never hang the GPU: flag it and go on
              if (d256_fresh_lane() == 0) __hip_atomic_store((d256c_g_u32 *)p.err, 1u + (unsigned)l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              break;
            }
            __builtin_amdgcn_s_sleep(1);
          }
        }
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_barrier(); // the polling wave has seen the producers arrive
        __builtin_amdgcn_sched_barrier(0);
      }
      GemmArgs a{}; // (C, D, ldc and the epilogue bits: the body reads them behind its K loop)
      a.A = l > 0 ? (const void *)p.L[lp].C : p.A;
      a.lda = l > 0 ? p.L[lp].ldc : p.lda;
      a.B = p.L[l].B;
      a.ldb = p.L[l].ldb;
      a.stride_a = p.L[l].stride_a;
      a.stride_b = p.L[l].stride_b;
      a.k = p.L[l].k;
      a.br = p.L[l].br;
      a.ep = EP_BETA0;
      brgemm_bf16_dma256_body<IMG, false, true>(a, tm, tn, wave, l);
    }
    d256c_kernarg_t &p = d256c_args_here();
    const int L = p.nlayers, G = p.groups, tiles_m = p.tiles_m;
    const bool last = l + 1 == L;
    if (last && !chain_rounds_more(tm, G, tiles_m)) break;
    if (last) {
      // a further row block of the LAST layer follows: nothing to publish and no store to wait for - only the rendezvous behind every
      // wave's epilogue (its staging tile in the ring has been read back) before the next step's prologue fills the ring
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    } else {
      // ---- seam: publish this tile to the row block's consumers
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // EVERY storing wave drains its write-through stores
      __builtin_amdgcn_s_barrier();
      if (d256c_here(wave) == 0 && d256_fresh_lane() == 0)
        __hip_atomic_fetch_add((d256c_g_u32 *)(p.cnt + d256c_counter(l, tm, tiles_m, CHAIN_CNT_STRIDE)), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __builtin_amdgcn_sched_barrier(0);
    chain_rounds_next(tm, l, G, tiles_m);
  }
}

// (the argument is read through the kernarg segment pointer: see the body)
__global__ __launch_bounds__(256) void brgemm_bf16_dma256_chain(ChainArgs) { brgemm_bf16_dma256_chain_body<0>(); }
__global__ __launch_bounds__(256) void brgemm_bf16_dma256_chain_flatb(ChainArgs) { brgemm_bf16_dma256_chain_body<2>(); }
__global__ __launch_bounds__(256) void brgemm_bf16_dma256_chain_vnni4(ChainArgs) { brgemm_bf16_dma256_chain_body<4>(); }

template <int IMG> static hipError_t launch_bf16_dma256_chain_t(const ChainArgs &a, hipStream_t s) {
  constexpr size_t lds = 4 * 32768;
  static std::atomic<unsigned long long> lds_set{0};
  void (*const kern)(ChainArgs) = IMG == 0 ? brgemm_bf16_dma256_chain : IMG == 2 ? brgemm_bf16_dma256_chain_flatb : brgemm_bf16_dma256_chain_vnni4;
  if (hipError_t e = ensure_dynamic_lds((const void *)kern, (int)lds, lds_set); e != hipSuccess) return e;
  ChainArgs args = a;
  args.tiles_m = a.m / D256C_BM;
  args.tiles_n = a.n / D256C_BN;
  args.groups = a.groups > 0 ? a.groups : args.tiles_m; // one round: every row block its own group
  args.xm = 0;
  args.items = nullptr;
  args.item_subs = 0;
  args.pad_items = 0;
  hipLaunchKernelGGL(kern, dim3((unsigned)d256c_grid(args.groups, args.tiles_n)), dim3(256), lds, s, args);
  return hipGetLastError();
}

// A chain of a.nlayers layers of m x n on the 256x256 tile with B image b_kind (0 VNNI-2, 2 flat, 4 VNNI-4; every layer the same) on
// a.groups row groups (0: one round, tiles_m groups); the caller guarantees groups * n / 256 <= the stream's compute units and the
// counters / target / error word of a chain launch. Refuses - hipErrorInvalidValue, nothing launched - whatever the kernel cannot run:
// m or n not in whole tiles, fewer than 2 or more than CH_MAXL layers, a k not in 32-k chunks or an empty batch, a layer that is not
// beta 0 or stores a VNNI C, no 16-byte pieces at a DMA lane's source or a row of C, an 8-byte bias read off its grid, a lane offset
// beyond 31 bits, a later layer whose batch elements leave its predecessor's rows, more groups than row blocks, no counters.
hipError_t launch_bf16_dma256_chain(int b_kind, const ChainArgs &a, hipStream_t s) {
  if (!d256_image_ok(b_kind) || a.groups < 0 || !d256c_shape_ok(a.m, a.n, a.nlayers, CH_MAXL, a.groups > 0 ? a.groups : a.m / D256C_BM)) return hipErrorInvalidValue;
  if (!a.A || !a.cnt || !a.err || ((uintptr_t)a.A & 15) || (a.lda & 7) || a.lda >= (1 << 22)) return hipErrorInvalidValue;
  for (int l = 0; l < a.nlayers; ++l) {
    const ChainLayer &y = a.L[l];
    const int64_t lda = l > 0 ? a.L[l - 1].ldc : a.lda;
    if (!d256c_k_ok(y.k, y.br) || !(y.ep & EP_BETA0) || (y.ep & EP_VNNI_C)) return hipErrorInvalidValue;
    if (!d256_b_ldb_ok(b_kind, y.ldb) || lda < y.k || y.ldc < a.n || ((y.ldc | y.stride_a | y.stride_b) & 7) || y.ldc >= (1 << 22)) return hipErrorInvalidValue;
    if (!y.B || !y.C || (((uintptr_t)y.B | (uintptr_t)y.C) & 15) || ((y.ep & EP_BIAS) && (!y.D || ((uintptr_t)y.D & 7)))) return hipErrorInvalidValue;
    if (l > 0 && (int64_t)(y.br - 1) * y.stride_a + y.k > lda) return hipErrorInvalidValue; // (the hand-off is per row block)
  }
  return b_kind == 0 ? launch_bf16_dma256_chain_t<0>(a, s) : b_kind == 2 ? launch_bf16_dma256_chain_t<2>(a, s) : launch_bf16_dma256_chain_t<4>(a, s);
}

} // namespace tpp
