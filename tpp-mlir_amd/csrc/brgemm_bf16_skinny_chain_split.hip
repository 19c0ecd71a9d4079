// brgemm_bf16_skinny_chain_split.hip - a CHAIN of skinny-batch bf16 layers (1 .. 31 rows) in ONE launch whose layers are K-SPLIT over workgroups
// (opt-in: xsmm_hip_set_chain_skinny_split, a refinement of xsmm_hip_set_chain_skinny). The unsplit chain (brgemm_bf16_skinny_chain.hip) has
// min(column blocks of the widest layer, CUs) resident workgroups, each streaming the whole K range of its blocks alone, while the separate
// calls run split on P times as many. Here the resident-workgroup loop of the chain walks UNITS - a (part, column block) of
// brgemm_bf16_skinny_split.hip - instead of blocks, and a block's parts meet through that kernel's hand-off, in which nobody waits. The
// schedule: brgemm_bf16_skinny_chain_split.h, walked on a CPU by tests/test_chain_skinny_split_cpu.py.
// THE TEXT of the K loop and the epilogue is the unsplit chain's (brgemm_bf16_skinny_chain_body.h: sc1 loads of handed-off A, the seam wait
// between the B and the A loads of the first ring slots, sc1 stores), not brgemm_bf16_skinny_tile.h's: that tile has neither the sc1 paths
// nor the hook, and the unsplit chain built from a tile that had them measured slower (its header). The bit-for-bit GPU test against the
// calls under xsmm_hip_set_skinny_bf16(BN) + xsmm_hip_set_skinny_split(P), which run the tile, keeps the two in step.
//
// UNITS. Layer l has blocks_l column blocks, S_l = br_l * skn_steps(k_l) steps and P_l = min(P, S_l) parts per block: blocks_l * P_l units,
// part-major (unit u = part * blocks_l + block: workgroups that start together share a k range, A's bytes). Workgroup w of G takes the
// units w, w + G, ..; none if w is at or beyond the unit count.
// ONE UNIT is what one workgroup of brgemm_bf16_skinny_split runs: the part's run of steps dealt over waves by sks_wave_first /
//   sks_wave_count (ring of SKN_DEPTH steps, the ragged-k mask on the last step of a batch element), the LDS combine into wave 0 in wave
//   order, the part's f32 sum parked at [block][part][register][lane] of the stream's scratch block with 16-byte write-through stores,
//   s_waitcnt vmcnt(0), one relaxed agent-scope fetch_add on the block's arrival counter. The LAST ARRIVER - whichever workgroup it is; one
//   that owns several parts of a block is simply its own - resets the counter, loads ALL P_l parts past the caches, adds them in part order
//   0 .. P_l - 1 and runs the chain's epilogue (bias, relu, ONE rounding to bf16, write-through stores). Nobody waits for a part. A layer
//   with P_l = 1 (one step) skips the hand-off: its unit is the unsplit chain's block. Every layer is so bit for bit the call under
//   xsmm_hip_set_skinny_bf16(BN) + xsmm_hip_set_skinny_split(P).
// THE SEAM stays ONE counter per seam, cnt[l], target epoch * G (brgemm_bf16_skinny_chain.hip's header has the protocol; the consumer's side
//   is its skc_seam_wait, in front of the workgroup's FIRST unit of a layer l > 0, between the B and the A loads of the first ring slots:
//   weights ahead of the wait). Every workgroup adds 1 exactly once per layer: wave 0, behind the workgroup's LAST unit of the layer - or
//   thread 0 at once where it has none - after s_waitcnt vmcnt(0). Only wave 0 stores to global memory, so that wait covers every epilogue
//   store this workgroup made as a last arriver in the layer, its resets of arrival counters and its parked parts.
//   WHY A SEAM AT ITS TARGET MEANS THE LAYER IS STORED: every block of layer l has exactly one last arriver (the fetch_add hands out
//   0 .. P_l - 1 once each), a workgroup that runs the block's epilogue as part of one of ITS units; its seam arrival comes behind its last
//   unit and the vmcnt(0) wait, hence behind those stores. The counter reaches epoch * G only when all G workgroups have arrived, the last
//   arrivers of all blocks among them.
// THE SCRATCH ACROSS LAYERS. One region of partial sums and one set of arrival counters serve every layer of the launch, laid out per
//   layer ([blocks_l][P_l] slots of MB * BN floats): a slot of layer l + 1 may overlap any slot of layer l. The order of events makes it
//   safe: a unit of layer l + 1 parks its part only behind the consumer's wait at seam l - a workgroup waits there in front of its first
//   unit of layer l + 1 (every wave calls the K loop's wait, with steps or without), and a workgroup that sits layer l + 1 out parks
//   nothing; seam l reaches its target only after EVERY workgroup has arrived, each behind its last unit of layer l, the last arrivers'
//   reads of all parts and their counter resets (vmcnt(0)) included. So every read of layer l's parts and every reset is complete before
//   the first write of a part or the first arrival of layer l + 1. Inside a layer no slot is written twice and a counter runs 0 .. P_l - 1
//   once. Layer 0 follows the previous launch of the stream, whose block it is (split_scratch.h), in stream order.
// WAVES: the launch has the waves of its deepest part (sks_block_waves, the most over the layers); a wave beyond a unit's count takes no
//   step but meets every barrier. LDS is the unsplit chain's (part[], two barriers per unit), PROGRESS its argument: G <= CUs workgroups,
//   all resident; the only wait is the bounded poll of an EARLIER layer's seam, and every arrival is unconditional.
#include "brgemm_bf16_skinny_chain_body.h"
#include "brgemm_bf16_skinny_chain_split.h"
#include "split_scratch.h"

namespace tpp {

static_assert(SKC_MAXL == CH_MAXL, "the schedule's layer count is the launch's");
static_assert(SKS_PMAX == SPLIT_MAX && SKCS_MAX_TILES == SPLIT_MAX_TILES && SKCS_MAX_FLOATS == (long long)SPLIT_SCRATCH_FLOATS,
              "the planner's most parts, column blocks and partial floats are the scratch block's");

// the argument block (chain_args.h: ChainArgs, then the scratch block and the parts), read where it lies
typedef const __attribute__((address_space(4))) ChainSplitArgs skcs_kernarg_t;

// a layer's schedule facts, from the argument block as it is read at this point (skc_args_again): derived anew on each side of the K loop,
// a few scalar instructions, instead of living in scalar registers across it
struct SkcsLayer {
  int blocks, S_all, P_l, units;
  __device__ __forceinline__ SkcsLayer(skcs_kernarg_t &p, const int l, const int bn)
      : blocks(skn_blocks(p.L[l].pad, bn)), S_all(skcs_steps(p.L[l].br, p.L[l].k)), P_l(sks_parts(p.split, S_all)), units(blocks * P_l) {}
};

template <int IMG, int BN, int MB> __global__ __launch_bounds__(64 * SKN_WMAX) void brgemm_bf16_skinny_chain_split(ChainSplitArgs p_by_value) {
  skcs_kernarg_t *const pp = (skcs_kernarg_t *)__builtin_amdgcn_kernarg_segment_ptr(); // = &p_by_value (the only explicit argument)
  constexpr int C = skn_cols(BN), SETS = MB / 16, REGS = SETS * C;
  constexpr int NACC = REGS * 4;
  __shared__ float part[(SKN_WMAX - 1) * NACC * 64];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int w = (int)blockIdx.x;

  for (int l = 0; l < pp->nlayers; ++l) {
    // this workgroup's units of the layer: w, w + G, .. (skcs_unit) - none if w is at or beyond the layer's units (skcs_owned)
    if (w >= SkcsLayer(*pp, l, BN).units) { // the layer is sat out: arrive at once (nothing of this workgroup's is owed, and it parks nothing)
      if (skc_signals(l, pp->nlayers) && threadIdx.x == 0)
        __hip_atomic_fetch_add((skc_gu32 *)(pp->cnt + (size_t)l * CHAIN_CNT_STRIDE), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      continue;
    }
    for (int u = w;;) {
      int prt; // (u and prt are what crosses the K loop)
      f32x4 acc[SETS][C];
      {
        skcs_kernarg_t &p = *skc_args_again(pp);
        const SkcsLayer f(p, l, BN);
        prt = skcs_unit_part(u, f.blocks);
        const int blk = u - prt * f.blocks;
        SkcLayer a;
        a.A = l == 0 ? p.A : p.L[l - 1].C;
        a.lda = l == 0 ? p.lda : p.L[l - 1].ldc;
        a.B = p.L[l].B, a.D = nullptr, a.C = nullptr;
        a.ldb = p.L[l].ldb, a.ldc = 0, a.stride_a = p.L[l].stride_a, a.stride_b = p.L[l].stride_b;
        a.m = p.m, a.n = p.L[l].pad, a.k = p.L[l].k, a.br = p.L[l].br, a.ep = 0;
        const int cnt = sks_wave_count(wave, prt, f.P_l, f.S_all), t0 = sks_wave_first(wave, prt, f.P_l, f.S_all);
        const int n0 = skn_origin(blk, a.n, BN);
        const unsigned *const seam = p.cnt + (size_t)(l > 0 ? l - 1 : 0) * CHAIN_CNT_STRIDE;
        if (l == 0) skc_k_loop<IMG, BN, MB, false>(a, lane, wave, n0, t0, cnt, false, seam, p.target, p.err, l, acc);
        else skc_k_loop<IMG, BN, MB, true>(a, lane, wave, n0, t0, cnt, u == w, seam, p.target, p.err, l, acc);
      }
      skcs_kernarg_t &p = *skc_args_again(pp);
      const SkcsLayer f(p, l, BN);
      const int P_l = f.P_l, units = f.units, blk = u - prt * f.blocks;
      const int W = skn_waves(sks_part_count(prt, P_l, f.S_all)); // the waves of this part that had steps
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
      const int next = u + p.groups;
      if (wave == 0) {
        bool last = true;
        if (P_l > 1) { // the hand-off of brgemm_bf16_skinny_split.hip: park the part's sum, arrive, and only the last arriver goes on
          // (the slot's last byte lies below blocks_l * P_l * MB * BN floats, which the launcher has fitted to the scratch block)
          const __amdgpu_buffer_rsrc_t rs =
              __builtin_amdgcn_make_buffer_rsrc((void *)(p.split_scratch + (size_t)blk * P_l * (MB * BN)), 0, 0x7fffffff, 0x00020000);
          const unsigned vo = (unsigned)(lane * 16);
#pragma unroll
          for (int s = 0; s < SETS; ++s)
#pragma unroll
            for (int j = 0; j < C; ++j)
              __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[s][j]), rs, vo, (unsigned)((prt * REGS + s * C + j) * 1024), SKC_SC1);
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          unsigned arrived = 0;
          if (lane == 0) arrived = __hip_atomic_fetch_add((skc_gu32 *)(p.split_cnt + blk), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          arrived = __builtin_amdgcn_readfirstlane(arrived);
          last = arrived == (unsigned)(P_l - 1);
          if (last) {
            if (lane == 0) __hip_atomic_store((skc_gu32 *)(p.split_cnt + blk), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // ALL partials, this workgroup's own included, in part order: the bits do not depend on who arrived last
#pragma unroll
            for (int s = 0; s < SETS; ++s)
#pragma unroll
              for (int j = 0; j < C; ++j)
                acc[s][j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, vo, (unsigned)((s * C + j) * 1024), SKC_SC1));
            for (int q = 1; q < P_l; ++q)
#pragma unroll
              for (int s = 0; s < SETS; ++s)
#pragma unroll
                for (int j = 0; j < C; ++j)
                  acc[s][j] += __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, vo, (unsigned)((q * REGS + s * C + j) * 1024), SKC_SC1));
          }
        }
        if (last) {
          SkcLayer a{};
          a.D = p.L[l].D, a.C = p.L[l].C, a.ldc = p.L[l].ldc;
          a.m = p.m, a.n = p.L[l].pad, a.ep = p.L[l].ep;
          skc_epilogue<BN, MB>(a, lane, blk, skn_origin(blk, a.n, BN), acc);
        }
        if (skc_signals(l, p.nlayers) && next >= units) { // the producer's side of the seam, behind the LAST unit: only this wave stored
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          if (lane == 0) __hip_atomic_fetch_add((skc_gu32 *)(p.cnt + (size_t)l * CHAIN_CNT_STRIDE), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      if (next >= units) break;
      u = next;
    }
  }
}

template <int IMG, int BN> static hipError_t launch_bf16_skinny_chain_split_t(const ChainSplitArgs &a, int waves, hipStream_t s) {
  const dim3 grid(a.groups), block(64 * waves);
  if (skn_mb(a.m) == 16) hipLaunchKernelGGL((brgemm_bf16_skinny_chain_split<IMG, BN, 16>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((brgemm_bf16_skinny_chain_split<IMG, BN, 32>), grid, block, 0, s, a);
  return hipGetLastError();
}

bool bf16_skinny_chain_args_ok(int b_kind, int bn, const ChainArgs &a); // brgemm_bf16_skinny_chain.hip

// launch_bf16_skinny_chain's chain with every layer over min(parts, its steps) workgroups per column block, on a.groups = G resident
// workgroups, G at most the stream's compute units - the caller's guarantee. Refuses with hipErrorInvalidValue, launching nothing, what
// launch_bf16_skinny_chain refuses, parts outside 2 .. 16, a chain none of whose layers has two steps (nothing to split), and a launch the
// stream's scratch block cannot hold: a split layer with more column blocks than arrival counters (SPLIT_MAX_TILES) or more partial
// floats than a block has, or no block at all (no memory, a 17th stream, a stream being captured) - the caller then runs
// launch_bf16_skinny_chain with the same arguments.
hipError_t launch_bf16_skinny_chain_split(int b_kind, int bn, int parts, const ChainArgs &a, hipStream_t s) {
  if (!skcs_parts_ok(parts) || !bf16_skinny_chain_args_ok(b_kind, bn, a)) return hipErrorInvalidValue;
  const int mb = skn_mb(a.m);
  long long floats = 0, counters = 0;
  int waves = 1;
  for (int l = 0; l < a.nlayers; ++l) {
    const ChainLayer &L = a.L[l];
    if (!skcs_layer_fits(L.pad, bn, mb, parts, L.br, L.k, SPLIT_MAX_TILES, SPLIT_MAX, (long long)SPLIT_SCRATCH_FLOATS)) return hipErrorInvalidValue;
    floats = std::max(floats, skcs_layer_floats(L.pad, bn, mb, parts, L.br, L.k));
    counters = std::max(counters, skcs_layer_counters(L.pad, bn, parts, L.br, L.k));
    waves = std::max(waves, skcs_layer_waves(parts, L.br, L.k));
  }
  if (counters == 0) return hipErrorInvalidValue;
  const SplitScratch *sc = split_scratch_for(s, counters, floats);
  if (!sc) return hipErrorInvalidValue;
  ChainSplitArgs args;
  static_cast<ChainArgs &>(args) = a;
  args.split = parts;
  args.split_scratch = sc->partial;
  args.split_cnt = sc->cnt;
  switch (b_kind * 100 + bn) {
  case 16: return launch_bf16_skinny_chain_split_t<0, 16>(args, waves, s);
  case 32: return launch_bf16_skinny_chain_split_t<0, 32>(args, waves, s);
  case 64: return launch_bf16_skinny_chain_split_t<0, 64>(args, waves, s);
  case 232: return launch_bf16_skinny_chain_split_t<2, 32>(args, waves, s);
  case 264: return launch_bf16_skinny_chain_split_t<2, 64>(args, waves, s);
  case 416: return launch_bf16_skinny_chain_split_t<4, 16>(args, waves, s);
  case 432: return launch_bf16_skinny_chain_split_t<4, 32>(args, waves, s);
  case 464: return launch_bf16_skinny_chain_split_t<4, 64>(args, waves, s);
  }
  return hipErrorInvalidValue;
}

} // namespace tpp
