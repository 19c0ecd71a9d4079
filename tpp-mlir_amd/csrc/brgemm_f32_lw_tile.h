// brgemm_f32_lw_tile.h - the f32 loader-wave tile, written once: brgemm_f32_lw (one layer) and brgemm_f32_lw_chain (the layers of a
// step in one launch) in brgemm_f32_lw.hip are built from these pieces, which is what makes the chain's results the separate
// launches' bits - the same LDS images, the same schedule, the same order of additions. brgemm_f32_lw16.hip shares the loader schedule.
// (The structure and why it is as it is: the head of brgemm_f32_lw.hip.)
#pragma once
#include "brgemm_f32_lw_kedge.h"
#include "gemm_common.h"
#include "xsmm_desc.h"
#include <type_traits>

namespace tpp {

constexpr int LW_BK = 64;   // k per chunk
constexpr int LW_NSLOT = 4; // LDS ring slots
constexpr int LW_C_AUX = C_STORE_AUX; // write-through C stores (gemm_common.h)
static_assert(KEDGE_BK == LW_BK, "the ragged-k schedule is written for this chunk");

typedef __attribute__((address_space(3))) void lds_void_lw;
// The ring = the launch's dynamic LDS; the K-group combine parks its partials in it. Named here and used by the pieces directly: handed
// to them as a pointer argument the compiler kept one address register per (slot, k-block) where it now folds the slot offsets into
// the ds_read immediates - 8 VGPRs more on the 64x64 tile (80 -> 88, one wave per SIMD less in the compiler's resource report).
extern __shared__ __attribute__((aligned(16))) float smem_lw[];

// The loader waves' schedule: issue(slot) requests the next chunk of the wave's panel into a ring slot, wait_left(n) returns when
// all but the n youngest chunks of the wave's own DMA have landed.
// Prologue: chunks 0 and 1 are requested, chunk 0 is PUBLISHED as soon as it has landed, chunk 2 follows behind the barrier.
// (Round 2 requested all three first: an LDS-DMA instruction takes ~25 ns to issue, a chunk is 16 of them per loader - the MFMA
// waves waited ~0.4 us for requests they would not need for two chunk times; a chunk is 0.92 us of MFMA here, so the loader has
// all the time it needs behind the barrier. Stamped on the bf16 twin of this kernel: profiles/r03_chain_anatomy.txt.)
// first(): the request of chunk 0 into slot 0, for a loader that finishes its own setup behind it (Loader::issue_first) - the same
// request in the same place of the schedule.
template <int NSLOT, class Issue, class Wait, class First>
__device__ __forceinline__ void lw_loader_schedule(int T, Issue &&issue, Wait &&wait_left, First &&first) {
  if (T > 0) first();
  if (T > 1) issue(1);
  wait_left(T > 1 ? 1 : 0);
  __builtin_amdgcn_s_barrier(); // chunk 0 published
  if (NSLOT > 3 && T > 2) issue(2); // (a 3-slot ring holds chunks t, t+1, t+2: nothing more before chunk 0 has been retired)
  for (int t = 0; t + 1 < T; ++t) {
    wait_left(NSLOT > 3 && t + 2 < T ? 1 : 0); // chunk t+1 has landed (4 slots: chunk t+2 may still fly)
    __builtin_amdgcn_s_barrier();               // = the MFMA waves' mid-chunk barrier of chunk t
    if (t + NSLOT - 1 < T) issue((t + NSLOT - 1) % NSLOT); // the slot of chunk t-1: every MFMA wave is past it
  }
}

template <int NSLOT, class Issue, class Wait> __device__ __forceinline__ void lw_loader_schedule(int T, Issue &&issue, Wait &&wait_left) {
  lw_loader_schedule<NSLOT>(T, issue, wait_left, [&]() __attribute__((always_inline)) { issue(0); });
}

// LDS byte address of a float of the ring, and back: the MFMA waves' setup (LwTile::mfma_setup, tail_setup) keeps addresses as plain
// 32-bit numbers, which an empty asm can pin in a VGPR.
typedef __attribute__((address_space(3))) float lds_float_lw;
typedef __attribute__((address_space(3))) f32x4 lds_f32x4_lw;
__device__ __forceinline__ unsigned lw_lds_addr(const float *p) { return (unsigned)(__SIZE_TYPE__)(const lds_float_lw *)p; }
__device__ __forceinline__ lds_float_lw *lw_lds_float(unsigned a) { return (lds_float_lw *)(__SIZE_TYPE__)a; }
__device__ __forceinline__ const lds_f32x4_lw *lw_lds_f32x4(unsigned a) { return (const lds_f32x4_lw *)(__SIZE_TYPE__)a; }

// The tile of WM x WN MFMA waves (each ONE 32x32 accumulator) x WK wave groups that split every 64-k chunk, on an NSLOT-deep ring.
// NSLOT: 4; 3 for the 128x64 tile, whose 48 KiB slots would not fit four times.
template <int WM, int WN, int WK, int NSLOT = LW_NSLOT> struct LwTile {
  static constexpr int NMW = WM * WN * WK; // MFMA waves
  static constexpr int BM = 32 * WM, BN = 32 * WN;
  static constexpr int A_STAGE = BM * LW_BK, B_STAGE = LW_BK * BN, SLOT = A_STAGE + B_STAGE; // floats
  static constexpr int NA = BM / 4;      // DMA instructions (1 KiB each) per chunk of A: 4 rows x 64 k
  static constexpr int RPI = 256 / BN;   // B rows per DMA instruction
  static constexpr int NB = LW_BK / RPI; // DMA instructions per chunk of B
  static constexpr int KB_PER_WAVE = 8 / WK, KB_HALF = KB_PER_WAVE / 2;
  static constexpr int IPG = WK > 1 ? 4 / WK : 1; // K-split tiles: 16-byte store instructions per lane per group
  static constexpr size_t LDS_BYTES = (size_t)NSLOT * SLOT * sizeof(float);
  static_assert(KB_HALF >= 1, "tile outside the schedule's limits");
  static_assert(NSLOT == 3 || NSLOT == 4, "ring depth");
  static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");

  // ---- loader waves: NL for the A panel, NLB for the B panel; wave `part` of a panel issues the instructions part, part + NL, ... ----
  template <int NL, int NLB> struct Loader {
    static_assert(NA % NL == 0 && NB % NLB == 0, "panel instructions divide over the loader waves");
    static_assert(NA / NL <= 31 && NB / NLB <= 31, "tile outside the schedule's limits (vmcnt is 6 bits)");
    bool isA;
    int part, kc, kchunks;
    unsigned voA[4], voA2[2], voB, stepA, stepB, pairB;
    const float *g; // panel base of the chunk being fetched
    int64_t d_in, d_batch, d_wrap;

    // lw: loader wave 0 .. NL + NLB - 1 (the A loaders first). pair: a 64-k chunk is the 32-k blocks of TWO consecutive batch
    // elements (brgemm_f32_lw, GROUPED). nvalid: columns of the tile that exist (a multiple of 4; >= BN: all).
    // The constructor computes what the FIRST request needs and nothing else - the panel base, the lane offsets and steps of the
    // wave's own panel: that request starts the longest latency of the launch, every instruction in front of it is on the critical
    // path of every workgroup. What only the advance to the next chunk needs (d_in, d_batch, d_wrap: 64-bit multiplies) is
    // finish_setup(), which issue_first() runs BEHIND the request.
    __device__ __forceinline__ Loader(int lw, int lane, const float *A, const float *B, int m0, int n0, int lda, int ldb, int64_t stride_a,
                                      int64_t stride_b, int kchunks_, bool pair, int nvalid)
        : isA(lw < NL), part(lw < NL ? lw : lw - NL), kc(0), kchunks(kchunks_) {
#pragma unroll
      for (int j = 0; j < 4; ++j) voA[j] = 0u;
      voA2[0] = voA2[1] = voB = stepA = stepB = pairB = 0u;
      if (isA) {
        g = A + (int64_t)m0 * lda;
        // per-lane source offsets, constant for the whole panel stream. A instruction v covers rows 4v .. 4v+3
        // (lane -> row 4v + lane/16, 16-byte piece lane%16, XOR-ed with row&15 = 4(v&3) + lane/16: the
        // fragment read applies the same XOR); the 16-row group v>>2 goes into the scalar offset.
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = 4 * j + (lane >> 4), pc = (lane & 15) ^ r; // 16-byte piece of the chunk's row: k 4 pc .. 4 pc + 3
          voA[j] = (unsigned)((r * lda + (pair ? (pc >> 3) * (int)stride_a + 4 * (pc & 7) : 4 * pc)) * 4);
        }
        // NL = 2: this wave's instructions have v & 3 = part and part + 2 (NL = 4: always part)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int r = 4 * (part + 2 * j) + (lane >> 4), pc = (lane & 15) ^ r;
          voA2[j] = (unsigned)((r * lda + (pair ? (pc >> 3) * (int)stride_a + 4 * (pc & 7) : 4 * pc)) * 4);
        }
        stepA = (unsigned)(16 * lda * 4);
      } else {
        g = B + n0;
        // (a ragged last tile: the 16-byte column pieces beyond n re-read the tile's last valid piece - in bounds, and the columns
        // they feed are never stored)
        const int pieceB = nvalid < BN ? (lane % (BN / 4) < nvalid / 4 ? lane % (BN / 4) : nvalid / 4 - 1) : lane % (BN / 4);
        voB = (unsigned)(((lane / (BN / 4)) * ldb + 4 * pieceB) * 4);
        stepB = (unsigned)(RPI * ldb * 4);
        pairB = pair ? (unsigned)(((int)stride_b - 32 * ldb) * 4) : 0u; // rows 32.. of a pair chunk: the second element
      }
      ldb_ = ldb, stride_a_ = stride_a, stride_b_ = stride_b, pair_ = pair;
    }
    int ldb_;
    int64_t stride_a_, stride_b_;
    bool pair_;
    // the rest of the setup: how the panel base advances. The empty asm makes kchunks a value that exists only from here on, so the
    // compiler cannot lift the multiplies back above the request that issue_first() has just made.
    __device__ __forceinline__ void finish_setup() {
      int kch = kchunks;
      asm volatile("" : "+s"(kch));
      d_in = isA ? (int64_t)LW_BK : (int64_t)LW_BK * ldb_;
      d_batch = (isA ? stride_a_ : stride_b_) * (pair_ ? 2 : 1);
      d_wrap = d_batch - (int64_t)(kch - 1) * d_in;
    }
    // start at chunk t_first: batch element t_first / kchunks (pair mode: the pair t_first), k block t_first % kchunks
    __device__ __forceinline__ void start_at(int t_first) {
      const int b0 = t_first / kchunks;
      kc = t_first - b0 * kchunks;
      g += (int64_t)b0 * d_batch + (int64_t)kc * d_in;
    }
    template <int AUX> __device__ __forceinline__ void load_a(float *base, __amdgpu_buffer_rsrc_t r) const {
#pragma unroll
      for (int i = 0; i < NA / NL; ++i) {
        const int v = part + NL * i; // (NL = 2: v & 3 is part or part + 2 - both live in voA2)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_void_lw *)(base + v * 256), 16, NL == 1 ? voA[i & 3] : NL == 2 ? voA2[i & 1] : voA2[0],
                                                 (unsigned)(v >> 2) * stepA, 0, AUX);
      }
    }
    // request the next chunk of this wave's panel into ring slot `slot`. sc1 (MAY_SC1 instances only): the A rows were written by
    // other workgroups of THIS launch, another XCD's L2 may hold them - the aux bits stay a compile-time constant of each load.
    template <bool MAY_SC1 = false> __device__ __forceinline__ void issue(int slot, bool sc1 = false) {
      request<MAY_SC1>(slot, sc1);
      advance();
    }
    // the first request of a fresh loader (chunk 0 into slot 0), the rest of the setup behind it
    template <bool MAY_SC1 = false> __device__ __forceinline__ void issue_first(bool sc1 = false) {
      request<MAY_SC1>(0, sc1);
      finish_setup();
      advance();
    }
    template <bool MAY_SC1> __device__ __forceinline__ void request(int slot, bool sc1) const {
      float *base = smem_lw + slot * SLOT + (isA ? 0 : A_STAGE);
      const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void *)g, 0, 0x7fffffff, 0x00020000);
      if (isA) {
        if (MAY_SC1 && sc1) load_a<16>(base, r);
        else load_a<0>(base, r);
      } else {
#pragma unroll
        for (int i = 0; i < NB / NLB; ++i) {
          const int v = part + NLB * i;
          __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_void_lw *)(base + v * 256), 16, voB, (unsigned)v * stepB + (v * RPI >= 32 ? pairB : 0u), 0, 0);
        }
      }
    }
    __device__ __forceinline__ void advance() {
      if (++kc == kchunks) {
        kc = 0;
        g += d_wrap;
      } else {
        g += d_in;
      }
    }
    // RAGGED k (brgemm_f32_lw_kedge; the schedule: brgemm_f32_lw_kedge.h): kchunks = kedge_chunks(k) >= 2, the last chunk of every batch
    // element starts at k - 64. ragged_k once behind finish_setup (issue_first_ragged), then issue_ragged for issue: the advance into an element's last
    // chunk is k % 64 instead of 64 (issue has added 64: d_fix takes the overlap back), the batch wrap starts from k - 64.
    int64_t d_fix;
    __device__ __forceinline__ void ragged_k(int k) {
      const int64_t unit = d_in / LW_BK; // elements per k: 1 in A, ldb in B
      d_fix = (int64_t)(kedge_step(k, kchunks - 2) - LW_BK) * unit;
      d_wrap = d_batch - (int64_t)kedge_chunk_start(k, kchunks - 1) * unit;
    }
    __device__ __forceinline__ void issue_ragged(int slot) {
      issue(slot);
      if (kc == kchunks - 1) g += d_fix; // the chunk now due is the element's last
    }
    // the first request of a fresh ragged-k loader: finish_setup and ragged_k behind it
    __device__ __forceinline__ void issue_first_ragged(int k) {
      request<false>(0, false);
      finish_setup();
      ragged_k(k);
      advance();
      if (kc == kchunks - 1) g += d_fix;
    }
    // s_waitcnt vmcnt(n chunks of this wave's DMA may still be in flight), n = 0 or 1
    __device__ __forceinline__ void wait_left(int chunks) const {
      if (chunks == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else if (isA) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NA / NL) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NB / NLB) : "memory");
    }
  };

  // ---- MFMA waves ----------------------------------------------------------------------------------------------------------
  struct Wave { // role index wave = 0 .. NMW-1 -> K group wk, 32x32 block (wm, wn) = wmn of the tile
    int wk, wmn, wm, wn, lane;
    __device__ __forceinline__ Wave(int wave, int lane_) : wk(wave / (WM * WN)), wmn(wave % (WM * WN)), wm(wmn / WN), wn(wmn % WN), lane(lane_) {}
  };

  // The T > 0 chunks of one tile, from the "chunk 0 published" barrier (the caller's) to the last MFMA: one loop body per ring slot
  // (slot offsets are immediates), ONE raw s_barrier per chunk in the middle of the chunk's MFMAs, no vector memory instruction.
  // The setup of the chunk loop - where this lane's fragments lie in the ring - depends on the wave and the lane only, not on chunk 0:
  // mfma_setup() runs ABOVE the "chunk 0 published" barrier, while the wave waits for the loaders anyway, and pins every address in a
  // register (an empty asm the compiler cannot look through: it would otherwise sink the arithmetic to the first use, below the
  // barrier, where every CU pays for it in every launch with the data already there). Below the barrier stay the fragment reads.
  // a[g][q]: LDS byte address of the lane's 16-byte A piece of k-block q of the wave's share, ring slot g * A_SPG - the A_SPG slots
  // that the 16-bit offset of a ds_read_b128 reaches from there are immediates; b[slot][q]: its first B value of that block (the
  // other three: rows + 1 .. 3, offsets of the ds_read2_b32) - the registers the compiler has always kept for the steady-state lap.
  // PIN = false: nothing is computed ahead, load() is the expression the tile has always had and the compiler places the arithmetic
  // as it always has - for the instances where holding every address costs a wave per SIMD in the compiler's resource report: the
  // WK = 1 tiles (8 k-blocks per wave: 48 and 40 addresses) and the ragged-k kernels (profiles/f32_lw_head_tail_isa.txt).
  static constexpr int A_SPG = (65535 - 15) / (SLOT * 4) + 1, A_GRP = (NSLOT + A_SPG - 1) / A_SPG;
  static constexpr bool PIN_DEFAULT = WK > 1;
  template <bool PIN> struct Frags {
    unsigned a[PIN ? A_GRP : 1][KB_PER_WAVE], b[PIN ? NSLOT : 1][KB_PER_WAVE]; // (PIN only)
    int kbw;                                                                    // first k-block of the wave's share of a chunk
    int li, lh, a_off, b_off;                                                   // (PIN = false only)
    __device__ __forceinline__ void load(f32x4 &fa, float (&fb)[4], int slot, int q) const { // q: k-block of the wave's share
      if constexpr (PIN) {
        fa = *lw_lds_f32x4(a[slot / A_SPG][q] + (unsigned)((slot % A_SPG) * SLOT * 4));
        const lds_float_lw *bs = lw_lds_float(b[slot][q]);
#pragma unroll
        for (int s = 0; s < 4; ++s) fb[s] = bs[s * BN];
      } else {
        const int kb = kbw + q;
        const float *as = smem_lw + slot * SLOT + a_off;
        const float *bs = smem_lw + slot * SLOT + A_STAGE + b_off;
        fa = *(const f32x4 *)(as + (((2 * kb + lh) ^ (li & 15)) << 2));
#pragma unroll
        for (int s = 0; s < 4; ++s) fb[s] = bs[(8 * kb + 4 * lh + s) * BN];
      }
    }
  };
  template <bool PIN = PIN_DEFAULT> static __device__ __forceinline__ Frags<PIN> mfma_setup(const Wave &w) {
    Frags<PIN> f = {};
    f.li = w.lane & 31, f.lh = w.lane >> 5;
    f.a_off = (w.wm * 32 + f.li) * LW_BK, f.b_off = w.wn * 32 + f.li;
    f.kbw = w.wk * KB_PER_WAVE;
    if constexpr (PIN) {
#pragma unroll
      for (int q = 0; q < KB_PER_WAVE; ++q) {
        const int kb = f.kbw + q;
#pragma unroll
        for (int g = 0; g < A_GRP; ++g) {
          f.a[g][q] = lw_lds_addr(smem_lw + g * A_SPG * SLOT + f.a_off + (((2 * kb + f.lh) ^ (f.li & 15)) << 2));
          asm volatile("" : "+v"(f.a[g][q]));
        }
#pragma unroll
        for (int slot = 0; slot < NSLOT; ++slot) {
          f.b[slot][q] = lw_lds_addr(smem_lw + slot * SLOT + A_STAGE + f.b_off + (8 * kb + 4 * f.lh) * BN);
          asm volatile("" : "+v"(f.b[slot][q]));
        }
      }
    }
    return f;
  }
  // the chunk count of a tile, pinned like the addresses: the lap tests that need only T are decided above the barrier
  template <bool PIN = PIN_DEFAULT> static __device__ __forceinline__ int pin_chunks(int T) {
    if constexpr (PIN) asm volatile("" : "+s"(T));
    return T;
  }

  template <bool PIN> static __device__ __forceinline__ void mfma_chunks(f32x16 &acc, int T, const Frags<PIN> &f) {
    // MFMA fragments of one k-block (8 k): 4 A values (one ds_read_b128) and 4 B values per lane;
    // double-buffered so block q+1 is read while block q multiplies (brgemm_f32.hip has the layout notes)
    f32x4 fa[2];
    float fb[2][4];
    auto frag_load = [&](int buf, int slot, int q) __attribute__((always_inline)) { f.load(fa[buf], fb[buf], slot, q); }; // q: block of the wave's share
    // hn_c: does another chunk follow (= does this chunk carry the barrier)? 1: yes, a compile-time fact - the steady-state lap below
    // is then ONE basic block (a conditional barrier or an exit test between two chunks is a block boundary: a branch, and a point
    // where the compiler waits for every LDS read in flight); 2: decided at run time (the last lap)
    auto chunk = [&](auto slot_c, auto hn_c, bool has_next_rt) __attribute__((always_inline)) {
      constexpr int S = decltype(slot_c)::value, NS = (S + 1) % NSLOT;
      const bool has_next = decltype(hn_c)::value == 1 ? true : has_next_rt;
#pragma unroll
      for (int q = 0; q < KB_PER_WAVE; ++q) {
        const int cur = q & 1, nxt = cur ^ 1;
        if (q + 1 < KB_PER_WAVE) frag_load(nxt, S, q + 1);
        else frag_load(nxt, NS, 0); // first block of chunk t+1 (published by this chunk's barrier; unused after the last chunk)
        __builtin_amdgcn_sched_barrier(0); // the reads of step q+1 stay above the MFMAs of step q
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[cur][s], fb[cur][s], acc, 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (q == KB_HALF - 1 && has_next) {
          __builtin_amdgcn_s_barrier(); // chunk t+1 published by the loaders; the slot of chunk t-1 retired
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      // the prefetched fragments of chunk t+1 are dead on the loop's exit path: without this the compiler sinks
      // their reads into the next chunk's head, where the first MFMA then waits for them (the wait this
      // implies sits behind the last step's four MFMAs: the reads are long back)
      // (not inside the steady-state laps: there the next chunk follows in the same basic block, the sched_barriers keep the order,
      // and the pin would only make the compiler wait for the prefetched fragments at the end of every chunk)
      constexpr int PF = KB_PER_WAVE & 1;
      if constexpr (decltype(hn_c)::value != 1)
        asm volatile("" : "+v"(fa[PF]), "+v"(fb[PF][0]), "+v"(fb[PF][1]), "+v"(fb[PF][2]), "+v"(fb[PF][3]));
    };
    using S0 = std::integral_constant<int, 0>;
    using S1 = std::integral_constant<int, 1>;
    using S2 = std::integral_constant<int, 2>;
    using S3 = std::integral_constant<int, 3>;
    using HY = std::integral_constant<int, 1>;
    using HR = std::integral_constant<int, 2>;

    frag_load(0, 0, 0);
    int t = 0;
    for (; t + NSLOT < T; t += NSLOT) { // whole laps of the ring that are followed by at least one more chunk
      chunk(S0{}, HY{}, true);
      chunk(S1{}, HY{}, true);
      chunk(S2{}, HY{}, true);
      if constexpr (NSLOT > 3) chunk(S3{}, HY{}, true);
    }
    for (;;) { // the last lap: 1 .. NSLOT chunks
      chunk(S0{}, HR{}, t + 1 < T);
      if (++t == T) break;
      chunk(S1{}, HR{}, t + 1 < T);
      if (++t == T) break;
      chunk(S2{}, HR{}, t + 1 < T);
      if (++t == T) break;
      if constexpr (NSLOT > 3) {
        chunk(S3{}, HR{}, t + 1 < T);
        if (++t == T) break;
      }
    }
  }

  // RAGGED k (brgemm_f32_lw_kedge): mfma_chunks for batch elements of kchunks >= 2 chunks whose LAST chunk was fetched shifted back
  // (Loader::issue_ragged) - the wave does not multiply k-block b of that chunk unless kedge_block_runs(b, skip), skip =
  // kedge_skip_blocks: a wave-uniform test per k-block of the wave's share, around the four MFMAs only; the fragment reads (the slot
  // holds valid data) and the chunk's barrier stay, also for a K group that skips its whole share. Laps of the ring that hold no last
  // chunk are mfma_chunks' steady-state laps, one basic block; a lap with a last chunk in it goes chunk by chunk with the test.
  template <bool PIN> static __device__ __forceinline__ void mfma_chunks_ragged(f32x16 &acc, int T, int kchunks, int skip, const Frags<PIN> &f) {
    f32x4 fa[2];
    float fb[2][4];
    auto frag_load = [&](int buf, int slot, int q) __attribute__((always_inline)) { f.load(fa[buf], fb[buf], slot, q); };
    const int kbw = f.kbw;
    // rag_c 0: a whole chunk that another follows (compile-time facts: mfma_chunks' HY chunk); 1: `first` blocks of the chunk are
    // skipped (0: none), whether another chunk follows is decided at run time
    auto chunk = [&](auto slot_c, auto rag_c, int first, bool has_next_rt) __attribute__((always_inline)) {
      constexpr int S = decltype(slot_c)::value, NS = (S + 1) % NSLOT;
      constexpr bool RAG = decltype(rag_c)::value != 0;
      const bool has_next = RAG ? has_next_rt : true;
#pragma unroll
      for (int q = 0; q < KB_PER_WAVE; ++q) {
        const int cur = q & 1, nxt = cur ^ 1;
        if (q + 1 < KB_PER_WAVE) frag_load(nxt, S, q + 1);
        else frag_load(nxt, NS, 0);
        __builtin_amdgcn_sched_barrier(0);
        if (!RAG || kedge_block_runs(kbw + q, first)) {
#pragma unroll
          for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[cur][s], fb[cur][s], acc, 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (q == KB_HALF - 1 && has_next) {
          __builtin_amdgcn_s_barrier();
          __builtin_amdgcn_sched_barrier(0);
        }
      }
      constexpr int PF = KB_PER_WAVE & 1; // (mfma_chunks: the prefetched fragments are dead on an exit path)
      if constexpr (RAG) asm volatile("" : "+v"(fa[PF]), "+v"(fb[PF][0]), "+v"(fb[PF][1]), "+v"(fb[PF][2]), "+v"(fb[PF][3]));
    };
    using S0 = std::integral_constant<int, 0>;
    using S1 = std::integral_constant<int, 1>;
    using S2 = std::integral_constant<int, 2>;
    using S3 = std::integral_constant<int, 3>;
    using R0 = std::integral_constant<int, 0>;
    using R1 = std::integral_constant<int, 1>;

    frag_load(0, 0, 0);
    int t = 0, c = 0; // chunk t of the tile = chunk c of its batch element; a lap starts on slot 0
    for (;;) {
      if (c + NSLOT < kchunks) { // chunks c .. c + NSLOT - 1 are whole and the element's last chunk is still to come
        chunk(S0{}, R0{}, 0, true);
        chunk(S1{}, R0{}, 0, true);
        chunk(S2{}, R0{}, 0, true);
        if constexpr (NSLOT > 3) chunk(S3{}, R0{}, 0, true);
        t += NSLOT, c += NSLOT;
        continue;
      }
      chunk(S0{}, R1{}, c + 1 == kchunks ? skip : 0, t + 1 < T);
      if (++t == T) break;
      if (++c == kchunks) c = 0;
      chunk(S1{}, R1{}, c + 1 == kchunks ? skip : 0, t + 1 < T);
      if (++t == T) break;
      if (++c == kchunks) c = 0;
      chunk(S2{}, R1{}, c + 1 == kchunks ? skip : 0, t + 1 < T);
      if (++t == T) break;
      if (++c == kchunks) c = 0;
      if constexpr (NSLOT > 3) {
        chunk(S3{}, R1{}, c + 1 == kchunks ? skip : 0, t + 1 < T);
        if (++t == T) break;
        if (++c == kchunks) c = 0;
      }
    }
  }

  // ---- K-split tiles (WK > 1): combine the K groups through LDS and finish ----------------------------------------------------
  // EVERY group parks its 32x32 partial, then group g finishes the accumulator registers [g * 16 / WK, (g + 1) * 16 / WK) of its
  // tile - sum in group order (group 0 carries C when beta = 1), bias, relu, store. (With group 0 finishing alone the other
  // groups' waves idled through 16 LDS reads + 16 stores per lane.) Two workgroup barriers: the ring is free, the partials are there.
  // Where the wave parks, what it sums and where it stores depends on the lane, the wave's role and ldc only: tail_setup() runs with
  // mfma_setup() above the "chunk 0 published" barrier and pins the addresses, so that between the last MFMA and the stores there
  // are the two barriers, the LDS traffic and the additions, and no multiply by ldc. A handful of registers held across the loop.
  // PIN = false (the ragged-k kernels, the split instances, the 64x64 chain instance): nothing ahead, the expressions the tile has
  // always had.
  template <bool PIN> struct Tail {
    unsigned park;     // LDS byte address of the lane's first parked value
    unsigned src[IPG]; // ... of piece j of K group 0's partial (group g: + g * WM*WN * 4096, an immediate)
    unsigned off[IPG]; // piece_off(w, j, ldc)
    Wave w;            // (PIN = false only)
    int ldc;
  };
  template <bool PIN = true> static __device__ __forceinline__ Tail<PIN> tail_setup(const Wave &w, int ldc) {
    Tail<PIN> t = {0u, {}, {}, w, ldc};
    if constexpr (PIN && WK > 1) { // (WK = 1: no combine, the epilogue stores from the accumulator registers)
      t.park = lw_lds_addr(smem_lw + (w.wk * (WM * WN) + w.wmn) * 1024 + w.lane); // WK * WM*WN * 1024 floats, fits in the ring
      asm volatile("" : "+v"(t.park));
#pragma unroll
      for (int j = 0; j < IPG; ++j) {
        const int q = piece_row(w, j); // row of the 32x32 tile: q = (r & 3) + 4 * lh + 8 * (r >> 2)
        const int r = (q & 3) + 4 * (q >> 3), lh2 = (q >> 2) & 1;
        t.src[j] = lw_lds_addr(smem_lw + w.wmn * 1024 + r * 64 + lh2 * 32 + 4 * (w.lane & 7));
        t.off[j] = piece_off(w, j, ldc);
        asm volatile("" : "+v"(t.src[j]), "+v"(t.off[j]));
      }
    }
    return t;
  }
  template <bool PIN> static __device__ __forceinline__ unsigned tail_off(const Tail<PIN> &t, int j) {
    if constexpr (PIN) return t.off[j];
    else return piece_off(t.w, j, t.ldc);
  }
  template <bool PIN> static __device__ __forceinline__ void park_partials(const f32x16 &acc, const Tail<PIN> &t) {
    __syncthreads();
    if constexpr (PIN) {
      lds_float_lw *dst = lw_lds_float(t.park);
#pragma unroll
      for (int r = 0; r < 16; ++r) dst[r * 64] = acc[r];
    } else {
      float *dst = smem_lw + (t.w.wk * (WM * WN) + t.w.wmn) * 1024 + t.w.lane;
#pragma unroll
      for (int r = 0; r < 16; ++r) dst[r * 64] = acc[r];
    }
    __syncthreads();
  }
  // The parked partials are [register r][lane = column li + 32 * lh]: four consecutive columns of one output row (r, lh) are
  // 16 contiguous bytes. A lane finishes float4 pieces - 8 lanes x 16 B = one 128-byte row of the tile, a wave instruction 8
  // rows - so a tile is 4 x 16-byte stores per lane split over the K groups, instead of 16 dword stores (round 2).
  // Piece j of a lane: 16-byte column piece lane & 7 of row piece_row of the wave's 32x32 block.
  static __device__ __forceinline__ int piece_row(const Wave &w, int j) { return 8 * (w.wk * IPG + j) + (w.lane >> 3); }
  static __device__ __forceinline__ unsigned piece_off(const Wave &w, int j, int ldc) { // bytes from the tile's first element of C
    return (unsigned)(((w.wm * 32 + piece_row(w, j)) * ldc + w.wn * 32 + 4 * (w.lane & 7)) * 4);
  }
  template <bool PIN> static __device__ __forceinline__ void sum_partials(f32x4 (&part)[IPG], const Tail<PIN> &t) {
#pragma unroll
    for (int j = 0; j < IPG; ++j) {
      if constexpr (PIN) {
        const lds_f32x4_lw *src = lw_lds_f32x4(t.src[j]);
        f32x4 v = *src;
#pragma unroll
        for (int g = 1; g < WK; ++g) v += src[g * (WM * WN) * 256];
        part[j] = v;
      } else {
        const int q = piece_row(t.w, j); // row of the 32x32 tile: q = (r & 3) + 4 * lh + 8 * (r >> 2)
        const int r = (q & 3) + 4 * (q >> 3), lh2 = (q >> 2) & 1;
        const float *src = smem_lw + t.w.wmn * 1024 + r * 64 + lh2 * 32 + 4 * (t.w.lane & 7);
        f32x4 v = *(const f32x4 *)src;
#pragma unroll
        for (int g = 1; g < WK; ++g) v += *(const f32x4 *)(src + g * (WM * WN) * 1024);
        part[j] = v;
      }
    }
  }
  // bias, relu, 16-byte write-through stores (ok: this lane's column piece exists)
  template <bool PIN>
  static __device__ __forceinline__ void finish(const f32x4 (&part)[IPG], f32x4 bias4, int ep, __amdgpu_buffer_rsrc_t rsrcC, bool ok, const Tail<PIN> &t) {
#pragma unroll
    for (int j = 0; j < IPG; ++j) {
      f32x4 v = part[j] + bias4;
      if (ep & EP_RELU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.0f ? v[e] : 0.0f;
      }
      if (ok) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rsrcC, tail_off(t, j), 0, LW_C_AUX);
    }
  }
  // EDGE tiles (brgemm_f32_lw_edge): does the tile own this lane's piece j - rows >= own_r and columns >= own_c of the tile (own_c a
  // multiple of 4: a 16-byte piece is owned whole or not at all)
  static __device__ __forceinline__ bool piece_owned(const Wave &w, int j, int own_r, int own_c) {
    return w.wm * 32 + piece_row(w, j) >= own_r && w.wn * 32 + 4 * (w.lane & 7) >= own_c;
  }
  // finish for an edge tile: the same values, stored only where the tile owns them
  template <bool PIN>
  static __device__ __forceinline__ void finish_owned(const f32x4 (&part)[IPG], f32x4 bias4, int ep, __amdgpu_buffer_rsrc_t rsrcC, int own_r, int own_c,
                                                      const Wave &w, const Tail<PIN> &t) {
#pragma unroll
    for (int j = 0; j < IPG; ++j) {
      f32x4 v = part[j] + bias4;
      if (ep & EP_RELU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.0f ? v[e] : 0.0f;
      }
      if (piece_owned(w, j, own_r, own_c)) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rsrcC, tail_off(t, j), 0, LW_C_AUX);
    }
  }
};

} // namespace tpp
