// brgemm_bf16_skinny_chain.hip - a CHAIN of skinny-batch bf16 layers (1 .. 31 rows) in ONE launch (opt-in: xsmm_hip_set_chain_skinny): the
// unsplit skinny kernel (brgemm_bf16_skinny.hip) with a layer loop and a block loop around its body. G resident workgroups; in layer l
// workgroup w takes the column blocks w, w + G, .. of that layer's n_l columns (the schedule: brgemm_bf16_skinny_chain.h, walked on a CPU by
// tests/test_chain_skinny_map.py). A block is the single call's: the same load maps, ragged-k mask, ring of SKN_DEPTH steps, deal of the
// layer's steps over W_l = skn_waves(br_l * skn_steps(k_l)) waves, LDS combine into wave 0 in wave order, bias, relu and ONE rounding - bit
// for bit the call under xsmm_hip_set_skinny_bf16(BN). The launch has the waves of its deepest layer; a wave at or beyond W_l takes no step
// in layer l but meets every barrier.
// The K loop, the combine and the epilogue below are this file's own text of what brgemm_bf16_skinny_tile.h holds for the unsplit and the
// split kernel. Built from that tile (sc1 loads of A and the seam wait as a hook in its K loop, sc1 stores in its epilogue) every result
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
#include "gemm_common.h"
#include "chain_args.h"
#include "brgemm_bf16_skinny_chain.h"

namespace tpp {

static_assert(SKC_MAXL == CH_MAXL, "the schedule's layer count is the launch's");

typedef __bf16 skn_bf16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(1))) const char skn_gchar;
typedef unsigned int skn_u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) unsigned int skc_gu32;
// the argument block, read where it lies (kernarg segment): the layer table is indexed at run time (brgemm_bf16_lw.hip chain_kernarg_t)
typedef const __attribute__((address_space(4))) ChainArgs skc_kernarg_t;
constexpr int SKN_DEPTH = 4; // steps of loads in flight per wave
constexpr int SKC_SC1 = 16;  // aux of a raw buffer access: sc1

template <int P> __device__ __forceinline__ void skn_load_row(uint32_t (&d)[P], skn_gchar *p) {
  if constexpr (P == 1) {
    d[0] = *(__attribute__((address_space(1))) const uint32_t *)p;
  } else if constexpr (P == 2) {
    const skn_u32x2 v = *(__attribute__((address_space(1))) const skn_u32x2 *)p;
    d[0] = v.x, d[1] = v.y;
  } else {
#pragma unroll
    for (int q = 0; q < P / 4; ++q) {
      const u32x4 v = ((__attribute__((address_space(1))) const u32x4 *)p)[q];
      d[4 * q] = v.x, d[4 * q + 1] = v.y, d[4 * q + 2] = v.z, d[4 * q + 3] = v.w;
    }
  }
}

// one step of one lane: its R x P dwords of B and its 8 k values of one row of A per accumulator set
template <int IMG, int BN, int MB> struct SknStep {
  uint32_t b[skn_rows(IMG)][skn_dwords(IMG, BN)];
  u32x4 a[MB / 16];
};

// one layer's operands and shape, as the single call's GemmArgs has them
struct SkcLayer {
  const void *A, *B, *D;
  void *C;
  int64_t lda, ldb, ldc, stride_a, stride_b;
  int m, n, k, br, ep;
};

// the seam wait of a consumer: wave 0 polls, everybody meets the barrier (the file's header)
__device__ __forceinline__ void skc_seam_wait(const unsigned *cnt, unsigned target, unsigned *err, int layer, int wave, int lane) {
  if (wave == 0) {
    skc_gu32 *c = (skc_gu32 *)cnt;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    for (;;) {
      const unsigned v = __hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((int)(v - target) >= 0) break;
      if (__builtin_amdgcn_s_memrealtime() - t0 > CHAIN_TIMEOUT_TICKS) { // never hang the GPU: flag it and go on
        if (lane == 0) __hip_atomic_store((skc_gu32 *)err, 1u + (unsigned)layer, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
  }
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); // (no instruction: the A loads below stay behind the poll)
}

// steps t0 .. t0 + cnt - 1 of the layer's stream (numbered batch element by batch element) of the column block at n0, into acc (zeroed
// here). HANDED: A is a predecessor's output of this launch - sc1 buffer loads -, and with `wait` the seam wait stands between the B loads
// and the A loads of the first ring slots. Every wave of the workgroup calls this, one with cnt = 0 included (the barrier of the wait).
template <int IMG, int BN, int MB, bool HANDED>
__device__ __forceinline__ void skc_k_loop(const SkcLayer &p, const int lane, const int wave, const int n0, const int t0, const int cnt, const bool wait,
                                           const unsigned *seam, const unsigned target, unsigned *err, const int layer,
                                           f32x4 (&acc)[MB / 16][BN / 16]) {
  constexpr int C = skn_cols(BN), R = skn_rows(IMG), P = skn_dwords(IMG, BN), SETS = MB / 16, VF = skn_vfac(IMG);
  const int g = lane >> 4, l15 = lane & 15;
  const int spb = skn_steps(p.k);
  const int klast = skn_step_klim(p.k, spb - 1); // k values of the last step of a batch element: 8 .. 32
  const bool tail_masked = !skn_group_kept(lane, klast);

  const int64_t row_pitch = 2 * VF * p.ldb, step_pitch = 2 * (int64_t)SKN_KSTEP * p.ldb; // bytes: an image row, 32 k values of any image
  skn_gchar *const Bl = (skn_gchar *)p.B + skn_load_byte(IMG, BN, lane, 0, p.ldb) + 2 * VF * (int64_t)n0;
  skn_gchar *Al[SETS];
  unsigned Ao[SETS]; // HANDED: the lane's byte offset into the buffer of A (below 2^30: skc_ld_ok)
#pragma unroll
  for (int s = 0; s < SETS; ++s) {
    const int row = 16 * s + l15 < p.m ? 16 * s + l15 : p.m - 1; // a row at or beyond m: read from the last row, never stored
    Al[s] = (skn_gchar *)p.A + 2 * ((int64_t)row * p.lda + 8 * g);
    Ao[s] = (unsigned)(2 * (row * (int)p.lda + 8 * g));
  }
  const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void *)p.A, 0, 0x7fffffff, 0x00020000);

  auto load_b = [&] __device__(SknStep<IMG, BN, MB> &f, const int cb, const int cks) {
    if (cks == spb - 1 && tail_masked) { // (never true for k % 32 == 0)
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int q = 0; q < P; ++q) f.b[r][q] = 0;
    } else {
      skn_gchar *pb = Bl + 2 * (int64_t)cb * p.stride_b + (int64_t)cks * step_pitch;
#pragma unroll
      for (int r = 0; r < R; ++r) skn_load_row<P>(f.b[r], pb + r * row_pitch);
    }
  };
  auto load_a = [&] __device__(SknStep<IMG, BN, MB> &f, const int cb, const int cks) {
    if (cks == spb - 1 && tail_masked) {
#pragma unroll
      for (int s = 0; s < SETS; ++s) f.a[s] = u32x4{0, 0, 0, 0};
    } else if constexpr (HANDED) {
      const unsigned so = (unsigned)(2 * (cb * (int)p.stride_a + cks * SKN_KSTEP)); // (inside the row: below 2 lda)
#pragma unroll
      for (int s = 0; s < SETS; ++s) f.a[s] = __builtin_amdgcn_raw_buffer_load_b128(rsA, Ao[s], so, SKC_SC1);
    } else {
#pragma unroll
      for (int s = 0; s < SETS; ++s)
        f.a[s] = *(__attribute__((address_space(1))) const u32x4 *)(Al[s] + 2 * ((int64_t)cb * p.stride_a + cks * SKN_KSTEP));
    }
  };
  // the load cursor: batch element, step within it
  int cb = t0 / spb, cks = t0 - cb * spb;
  auto advance = [&] __device__(int &b, int &ks) {
    if (++ks == spb) ks = 0, ++b;
  };

#pragma unroll
  for (int s = 0; s < SETS; ++s)
#pragma unroll
    for (int j = 0; j < C; ++j) acc[s][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto compute = [&] __device__(const SknStep<IMG, BN, MB> &f) {
#pragma unroll
    for (int j = 0; j < C; ++j) {
      u32x4 bj;
#pragma unroll
      for (int q = 0; q < 4; ++q) { // dword q of the operand: k = 8 g + 2 q (low half), + 1 (high half)
        const SknSrc lo = skn_frag_src(IMG, j, 2 * q), hi = skn_frag_src(IMG, j, 2 * q + 1);
        const uint32_t x = f.b[lo.row][lo.dword], y = f.b[hi.row][hi.dword];
        bj[q] = (lo.half ? x >> 16 : x & 0xffffu) | (hi.half ? y & 0xffff0000u : y << 16);
      }
#pragma unroll
      for (int s = 0; s < SETS; ++s)
        acc[s][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(skn_bf16x8, f.a[s]), __builtin_bit_cast(skn_bf16x8, bj), acc[s][j], 0, 0, 0);
    }
  };

  SknStep<IMG, BN, MB> ring[SKN_DEPTH];
  // the first ring slots: the weights, then - behind the seam wait, where there is one - the activations
  {
    int ab = cb, aks = cks;
#pragma unroll
    for (int d = 0; d < SKN_DEPTH; ++d)
      if (d < cnt) {
        load_b(ring[d], cb, cks);
        advance(cb, cks);
      }
    if constexpr (HANDED)
      if (wait) skc_seam_wait(seam, target, err, layer, wave, lane);
#pragma unroll
    for (int d = 0; d < SKN_DEPTH; ++d)
      if (d < cnt) {
        load_a(ring[d], ab, aks);
        advance(ab, aks);
      }
  }
  int i = 0;
  for (; i + 2 * SKN_DEPTH <= cnt; i += SKN_DEPTH) { // steady state: every slot is computed and refilled
#pragma unroll
    for (int d = 0; d < SKN_DEPTH; ++d) {
      compute(ring[d]);
      load_b(ring[d], cb, cks);
      load_a(ring[d], cb, cks);
      advance(cb, cks);
    }
  }
  for (; i < cnt; i += SKN_DEPTH) {
#pragma unroll
    for (int d = 0; d < SKN_DEPTH; ++d)
      if (i + d < cnt) {
        compute(ring[d]);
        if (i + d + SKN_DEPTH < cnt) {
          load_b(ring[d], cb, cks);
          load_a(ring[d], cb, cks);
          advance(cb, cks);
        }
      }
  }
}

// wave 0, with the sum of the layer's steps in acc: a lane holds columns n0 + C l15 .. + C - 1 of rows 16 s + 4 g + r - one piece of 2 C bytes
// per row. The ownership skip of a shifted last block, the bias, relu and ONE rounding to bf16 (beta 0: the launcher takes nothing else);
// every piece leaves through a write-through store.
template <int BN, int MB>
__device__ __forceinline__ void skc_epilogue(const SkcLayer &p, const int lane, const int blk, const int n0, const f32x4 (&acc)[MB / 16][BN / 16]) {
  constexpr int C = skn_cols(BN), SETS = MB / 16;
  const int col = skn_out_col(BN, lane, 0);
  if (col < skn_skip(blk, p.n, BN)) return; // the block in front owns these columns
  float bias[C];
#pragma unroll
  for (int j = 0; j < C; ++j) bias[j] = 0.f;
  if (p.ep & EP_BIAS) {
    unsigned short h[C];
    const unsigned short *src = (const unsigned short *)p.D + n0 + col;
    if constexpr (C == 1) h[0] = *src;
    else if constexpr (C == 2) {
      const uint32_t v = *(const uint32_t *)src;
      h[0] = (unsigned short)v, h[1] = (unsigned short)(v >> 16);
    } else {
      const uint2 v = *(const uint2 *)src;
      h[0] = (unsigned short)v.x, h[1] = (unsigned short)(v.x >> 16), h[2] = (unsigned short)v.y, h[3] = (unsigned short)(v.y >> 16);
    }
#pragma unroll
    for (int j = 0; j < C; ++j) bias[j] = bf16_bits_to_f32(h[j]);
  }
  const __amdgpu_buffer_rsrc_t rsC = __builtin_amdgcn_make_buffer_rsrc(p.C, 0, 0x7fffffff, 0x00020000);
#pragma unroll
  for (int s = 0; s < SETS; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = skn_out_row(s, lane, r);
      if (row >= p.m) continue;
      const unsigned off = (unsigned)(2 * (row * (int)p.ldc + n0 + col)); // (below 2^30: skc_ld_ok)
      unsigned short h[C];
#pragma unroll
      for (int j = 0; j < C; ++j) {
        float v = acc[s][j][r];
        v += bias[j];
        if (p.ep & EP_RELU) v = v > 0.f ? v : 0.f;
        h[j] = f32_to_bf16_bits(v);
      }
      if constexpr (C == 1) __builtin_amdgcn_raw_buffer_store_b16(h[0], rsC, off, 0, SKC_SC1);
      else if constexpr (C == 2) __builtin_amdgcn_raw_buffer_store_b32((uint32_t)h[0] | ((uint32_t)h[1] << 16), rsC, off, 0, SKC_SC1);
      else
        __builtin_amdgcn_raw_buffer_store_b64(skn_u32x2{(uint32_t)h[0] | ((uint32_t)h[1] << 16), (uint32_t)h[2] | ((uint32_t)h[3] << 16)}, rsC, off, 0,
                                              SKC_SC1);
    }
}

// the argument block's address, opaque to the compiler from here on: what is read through the result is loaded HERE, not ahead of the K
// loop in front - the layer's facts would otherwise all stay in scalar registers across it, more than there are
__device__ __forceinline__ skc_kernarg_t *skc_args_again(skc_kernarg_t *pp) {
  asm volatile("" : "+s"(pp));
  return pp;
}

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
hipError_t launch_bf16_skinny_chain(int b_kind, int bn, const ChainArgs &a, hipStream_t s) {
  if (!skn_instance_exists(b_kind, bn) || !skc_launch_shape_ok(a.nlayers, a.groups) || !a.cnt || !a.err || !a.A || ((uintptr_t)a.A & 15)) return hipErrorInvalidValue;
  int waves = 1;
  for (int l = 0; l < a.nlayers; ++l) {
    const ChainLayer &L = a.L[l];
    const int64_t lda = l == 0 ? a.lda : a.L[l - 1].ldc;
    if (!skn_shape_ok(a.m, L.pad, L.k, L.br, bn) || !skc_ld_ok(lda, L.ldb, L.ldc, L.stride_a, L.stride_b, L.pad, L.k)) return hipErrorInvalidValue;
    if (!(L.ep & EP_BETA0) || (L.ep & EP_VNNI_C) || !L.B || !L.C || (((uintptr_t)L.B | (uintptr_t)L.C) & 15)) return hipErrorInvalidValue;
    if ((L.ep & EP_BIAS) && (!L.D || ((uintptr_t)L.D & 7))) return hipErrorInvalidValue;
    if (l > 0 && (int64_t)(L.br - 1) * L.stride_a + L.k > lda) return hipErrorInvalidValue;
    const int W = skc_layer_waves(L.br, L.k);
    if (W > waves) waves = W;
  }
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
