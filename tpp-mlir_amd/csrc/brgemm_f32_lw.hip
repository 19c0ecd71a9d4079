// brgemm_f32_lw.hip - f32 batch-reduce GEMM on v_mfma_f32_32x32x2_f32 with LOADER WAVES.
//
// Same arithmetic and LDS images as brgemm_f32_fast (brgemm_f32.hip: one workgroup per output tile,
// each MFMA wave one 32x32 accumulator = one k-ordered f32 fma chain per element, panels HBM -> LDS by
// LDS-DMA, A swizzled through the source address). What differs is WHO issues the DMA: measured on the
// 64x64 tile (profiles/r01_f32_c2_timeline_cycles.txt) a chunk costs 2302 cycles against 2048 of pure
// MFMA issue, and ~200 of the difference is the eight `buffer_load ... lds` instructions each MFMA wave
// issues per chunk: a wave is in-order, an LDS-DMA instruction takes 25-60 cycles to be accepted by
// the vector-memory path, and every such cycle delays the next MFMA of the SAME wave. A different wave on
// the same SIMD issues its VMEM instruction in parallel with that MFMA. So:
//   * WM*WN*WK MFMA waves: ds_read fragments + MFMA + ONE raw s_barrier per chunk. No vector memory
//     instruction in the loop at all.
//   * 2 loader waves (wave NMW streams A, wave NMW+1 streams B): all LDS-DMA of the workgroup, three
//     chunks ahead through a 4-slot ring; they wait for their own DMA (counted vmcnt) and meet the MFMA
//     waves at the per-chunk barrier, which publishes chunk t+1 and retires the slot of chunk t-1.
//   * one loop body per ring slot (slot offsets are immediates) and NO specialised tail bodies: the loop
//     is uniform, the end of the chunk stream only switches off a barrier (the first version's tail
//     variants each ran once per launch: instruction-cache cold misses in a 16-chunk kernel).
// The tile itself - the loader waves' offsets and schedule, the MFMA waves' chunk loop, the K-group combine and the finish - is
// brgemm_f32_lw_tile.h; the kernels below are their own logic around it.
#include "brgemm_f32_lw_tile.h"
#include "chain_args.h"
#include "split_scratch.h"
#include <type_traits>

namespace tpp {

typedef __attribute__((address_space(1))) unsigned int g_u32_lw;

// NSLOT: ring depth (4; 3 for the 128x64 tile, whose 48 KiB slots would not fit four times)
// NL loader waves for the A panel, NLB (default NL) for the B panel
// SPLIT (round 5): the batch-reduce dimension of ONE output tile is split over p.split workgroups - skinny outputs (the reference's
// M = 128 / 256 benchmark shapes: 32 .. 128 tiles on a 256-CU chip) otherwise leave most CUs idle. Workgroup (tile, s) owns the
// contiguous chunk range [T s / S, T (s + 1) / S), parks its partial tile in a scratch block (write-through stores), drains them
// and adds 1 to the tile's arrival counter; the workgroup whose add returns S - 1 (the last to arrive, whichever it is) sums the S
// partials IN SPLIT ORDER 0 .. S-1 - a fixed order of additions: results are bit-reproducible run to run, no float atomics -, adds
// C (beta = 1), bias, relu, stores, and resets the counter. No workgroup ever waits for another one (no co-residency assumption).
// GROUPED or SPLIT kernels also take n that is not a multiple of the tile width (the reference's --tiles=64,48,64 / 32,48,32):
// the B loader clamps the column pieces, the epilogue masks its loads and stores; the plain kernel (C2, C3) carries none of this.
// TAIL (opt-in, xsmm_hip_set_tail_split; gemm_plan.cpp choose_f32_tail_split): a whole-layer call of q CUs + r tiles in ONE launch whose
// first p.tail_body = q CUs workgroups each run one whole tile exactly as the plain kernel does (C joined at the start, all chunks,
// direct epilogue: the plain launch's bits) and whose last r S workgroups run the r tiles of the partial last round under the SPLIT
// protocol above, unchanged (chunk range [T s / S, T (s + 1) / S), park, count, the last arrival sums in split order: the bits of a
// SPLIT launch with that S). Body or tail is a run-time, workgroup-uniform test - which is why this is an instance of its own and not
// a mode of the plain kernel; it has the loader-wave counts of the plain instance of its tile, the body is most of the launch.
// The grid is linear and workgroups go to the XCDs round robin (XCD = workgroup id mod 8), so the mapping rebuilds the plain
// launcher's XCD blocks by hand: XCD x owns block x of the xm x xn blocks of tiles_m x tiles_n tiles the plain launcher would have
// chosen, and walks it in the plain grid's order (column fastest). The first tail_body / 8 tiles of EVERY block are body tiles, the
// rest of the block its tail tiles - each XCD's L2 keeps seeing one block of A rows and B columns through the whole launch, and the
// S workgroups of a tail tile run on the XCD whose L2 already holds that block's panels, in [s][tile] order like the SPLIT grid (the
// workgroups that start together share a k range). Shapes or CU counts that do not divide into 8 blocks: ONE block, the whole grid
// (p.tiles_m x p.tiles_n is then the whole tile grid: that is how the kernel tells the two).
template <int WM, int WN, int WK, bool GROUPED, int NL = 1, int NSLOT = LW_NSLOT, int NLB = NL, bool SPLIT = false, bool TAIL = false>
__global__ __launch_bounds__(64 * (WM * WN * WK + NL + NLB)) void brgemm_f32_lw(GemmArgs p, const WorkItem *__restrict__ items) {
  static_assert(!TAIL || (!GROUPED && !SPLIT), "the tail split is an instance of its own");
  constexpr bool MAYSPLIT = SPLIT || TAIL; // some workgroup of the launch shares its tile's batch-reduce range
  using Tile = LwTile<WM, WN, WK, NSLOT>;
  constexpr int NMW = Tile::NMW, BM = Tile::BM, BN = Tile::BN, IPG = Tile::IPG;

  const int tid = threadIdx.x, lane = tid & 63;
  // the two loader waves are the FIRST two hardware waves of the workgroup (waves start in order: the panels' first
  // chunks are requested before the MFMA waves have been launched); `wave` is the role index: MFMA waves 0 .. NMW-1, loaders NMW, NMW+1
  const int hw_wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave = hw_wave < NL + NLB ? NMW + hw_wave : hw_wave - (NL + NLB);
  // XCD-blocked (8, bn, bm) or plain (1, tiles_n, tiles_m) grid: see brgemm_f32.hip. GROUPED (tile queue): grid (items,
  // tiles_n, tiles_m), workgroup = one tile of one queued invoke, operands and batch count from its item. A template
  // parameter, not a run-time test: the plain kernel is the headline kernel and must not carry a second mode (measured: 0.6 %).
  static_assert(!SPLIT || WK > 1, "the split epilogue is the K-split tiles' float4 epilogue");
  constexpr bool RAGN = GROUPED || SPLIT; // n may end inside the tile's last 32-column block (a multiple of 4)
  WorkItem it{p.A, p.B, p.C, p.D, (int64_t)p.br};
  int tm, tn, sp = 0, tile_id = 0;
  bool is_tail = false; // TAIL: this workgroup shares a tail tile (else: it runs a whole body tile)
  if constexpr (TAIL) {
    const int per_block = p.tiles_m * p.tiles_n;                          // tiles of one block
    const int xshift = (p.m / BM) * (p.n / BN) == per_block ? 0 : 3;      // one block, or the 8 XCD blocks
    const int body_per = p.tail_body >> xshift, tail_per = per_block - body_per; // body and tail tiles of every block
    const int u = (int)blockIdx.x, x = u & ((1 << xshift) - 1); // (tail_body is a multiple of the block count: x is the XCD for both kinds)
    int lt = u >> xshift; // tile of block x, in the plain grid's order
    is_tail = u >= p.tail_body;
    if (is_tail) {
      const int j = (u - p.tail_body) >> xshift, t = j % tail_per;
      sp = j / tail_per;
      tile_id = x * tail_per + t; // scratch block and arrival counter: tail tiles only
      lt = body_per + t;
    }
    const int tz = lt / p.tiles_n;
    tm = (x >> p.xn_shift) * p.tiles_m + tz;
    tn = (x & ((1 << p.xn_shift) - 1)) * p.tiles_n + (lt - tz * p.tiles_n);
  } else if constexpr (SPLIT && GROUPED) {
    // grid (items * S, tiles_n, tiles_m): x = item * S + s (the two block rows of a layer that share a B panel then meet on one XCD)
    const int item = (int)blockIdx.x / p.split;
    sp = (int)blockIdx.x - item * p.split;
    if (items) it = items[item];
    tm = (int)blockIdx.z, tn = (int)blockIdx.y;
    tile_id = (item * (int)gridDim.y + tn) * (int)gridDim.z + tm;
  } else if constexpr (SPLIT) {
    // linear grid of S * tiles units in [s][tn][tm] order; XCD x (= workgroup id mod 8) takes the x-th eighth of the list, so that
    // one XCD's L2 sees ONE k range of A and B (every byte of the operands then comes out of HBM about once)
    const int tiles = p.tiles_m * p.tiles_n, total = tiles * p.split;
    int u = (int)blockIdx.x;
    if ((total & 7) == 0) u = (u & 7) * (total >> 3) + (u >> 3);
    sp = u / tiles;
    tile_id = u - sp * tiles;
    tn = tile_id / p.tiles_m;
    tm = tile_id - tn * p.tiles_m;
  } else {
    if constexpr (GROUPED) {
      if (items) it = items[blockIdx.x]; // (no list: a single invoke of the grouped kernel, operands in the arguments)
    }
    tm = GROUPED ? (int)blockIdx.z : (int)(blockIdx.x >> p.xn_shift) * p.tiles_m + (int)blockIdx.z;
    tn = GROUPED ? (int)blockIdx.y : (int)(blockIdx.x & ((1u << p.xn_shift) - 1)) * p.tiles_n + (int)blockIdx.y;
  }
  const int m0 = tm * BM, n0 = tn * BN;
  const int nvalid = RAGN ? p.n - n0 : BN; // columns of this tile that exist (>= BN everywhere but in a ragged last tile)
  // what the loader path reads of the arguments is fetched HERE, with the batch that the role test above needs - behind the branch
  // the loaders paid a second, dependent argument-fetch round trip in front of their first request (the empty asm: the values exist
  // from here on, the compiler cannot sink their loads into the branch)
  const float *A_ = (const float *)it.A, *B_ = (const float *)it.B;
  int lda = (int)p.lda, ldb = (int)p.ldb;
  int64_t stride_a = p.stride_a, stride_b = p.stride_b;
  asm volatile("" : "+s"(A_), "+s"(B_), "+s"(lda), "+s"(ldb), "+s"(stride_a), "+s"(stride_b));
  const float *__restrict__ A = A_;
  const float *__restrict__ B = B_;
  float *__restrict__ C = (float *)it.C;
  // GROUPED, k = 32 (the compiler's 32^3 tiles, mlir-gen --tiles=32,32,32): a 64-k chunk is the 32-k blocks of TWO consecutive
  // batch elements (even batch counts only: launch_gemm_grouped checks) - k 0..31 of the chunk image from element 2t, k 32..63
  // from element 2t+1. Only the loaders' source offsets know; the LDS images and the MFMA waves are the same.
  const bool pair = GROUPED && p.k == 32;
  const int kchunks = pair ? 1 : p.k / LW_BK;
  const int Tall = pair ? (int)it.br / 2 : (int)it.br * kchunks;
  // SPLIT: this workgroup's chunks [t_first, t_first + T) of the tile's Tall (TAIL: a body workgroup is the only one of its tile)
  const int nsplit = TAIL && !is_tail ? 1 : p.split;
  const int t_first = MAYSPLIT ? (int)(((long long)Tall * sp) / nsplit) : 0;
  const int T = MAYSPLIT ? (int)(((long long)Tall * (sp + 1)) / nsplit) - t_first : Tall;

  if (wave >= NMW) {
    // ---- loader waves --------------------------------------------------------------------
    typename Tile::template Loader<NL, NLB> ld(wave - NMW, lane, A, B, m0, n0, lda, ldb, stride_a, stride_b, kchunks, pair, nvalid);
    if constexpr (MAYSPLIT) { // (the first chunk of a shared tile is not chunk 0: the whole setup before the first request)
      ld.finish_setup();
      ld.start_at(t_first);
    }
    lw_loader_schedule<NSLOT>(T, [&](int slot) __attribute__((always_inline)) { ld.issue(slot); },
                              [&](int chunks) __attribute__((always_inline)) { ld.wait_left(chunks); },
                              [&]() __attribute__((always_inline)) {
                                if constexpr (MAYSPLIT) ld.issue(0);
                                else ld.issue_first();
                              });
    return; // ended waves do not take part in later barriers
  }

  // ---- MFMA waves --------------------------------------------------------------------------
  const typename Tile::Wave w(wave, lane);
  const int wk = w.wk, wm = w.wm, wn = w.wn;
  const int li = lane & 31, lh = lane >> 5;
  const int ccol = n0 + wn * 32 + li;
  const __amdgpu_buffer_rsrc_t rsrcC =
      __builtin_amdgcn_make_buffer_rsrc((void *)(C + (int64_t)m0 * p.ldc + n0), 0, 0x7fffffff, 0x00020000);
  const unsigned voffC = (unsigned)(((wm * 32 + 4 * lh) * (int)p.ldc + wn * 32 + li) * 4);
  const unsigned ldcb = (unsigned)((int)p.ldc * 4);
  // the accumulator chain of K group 0 starts from C (beta = 1), as in the reference; the bias is fetched
  // here so that its latency is not exposed in the epilogue
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  float bias = 0.0f;
  if constexpr (WK == 1) { // (the K-split tiles' epilogue works on float4 pieces: bias4 below)
    if ((p.ep & EP_BIAS) && (!RAGN || ccol < p.n)) bias = ((const float *)it.D)[ccol];
  }
  // ... and the K-split tiles' float4 epilogue: its four bias values per lane (16-byte column piece lane & 7). With ONE MFMA wave
  // per SIMD (32x32 + K4) they come in here as well - behind the combine's second barrier the load was an exposed round trip:
  // the batch-256 layer of the reference's MLP 7.05 -> 6.82 us per launch, its tile-queue iteration 19.47 -> 19.25 us (same box,
  // profiles/r04_c3_loaders_and_launch_knobs.txt (4)); with two MFMA waves per SIMD the other wave hides it and the early fetch
  // measured 0.02 us SLOWER on C3, so those tiles keep the load in the epilogue
  constexpr bool BIAS_EARLY = WK > 1 && WM * WN * WK <= 4;
  f32x4 bias4 = {0.0f, 0.0f, 0.0f, 0.0f};
  const bool piece_ok = !RAGN || wn * 32 + 4 * (lane & 7) < nvalid; // this lane's 16-byte column piece of the float4 epilogue exists
  if constexpr (BIAS_EARLY) {
    if ((p.ep & EP_BIAS) && piece_ok) bias4 = *(const f32x4 *)((const float *)it.D + n0 + wn * 32 + 4 * (lane & 7));
  }
  if (wk == 0 && !SPLIT && !(TAIL && is_tail)) { // (SPLIT: C joins the ordered sum of the partials in the last workgroup's epilogue)
    if (!(p.ep & EP_BETA0) && (!RAGN || ccol < p.n)) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        acc[r] = __builtin_bit_cast(
            float, __builtin_amdgcn_raw_buffer_load_b32(rsrcC, voffC, (unsigned)((r & 3) + 8 * (r >> 2)) * ldcb, 0));
    }
  }

  // the chunk loop's and the epilogue's address setup: above the barrier (brgemm_f32_lw_tile.h mfma_setup, tail_setup)
  const auto fr = Tile::mfma_setup(w);
  // (the SPLIT instances run at 99 .. 106 VGPRs: their epilogue keeps its addresses where they were)
  const auto tl = Tile::template tail_setup<!SPLIT>(w, (int)p.ldc);
  const int Tp = Tile::pin_chunks(T);

  __builtin_amdgcn_s_barrier(); // chunk 0 published
  __builtin_amdgcn_sched_barrier(0);
  if (Tp > 0) Tile::mfma_chunks(acc, Tp, fr);

  if constexpr (WK > 1) {
    Tile::park_partials(acc, tl);
    if constexpr (!BIAS_EARLY) {
      if ((p.ep & EP_BIAS) && piece_ok) bias4 = *(const f32x4 *)((const float *)it.D + n0 + wn * 32 + 4 * (lane & 7));
    }
    f32x4 part[IPG];
    Tile::sum_partials(part, tl);
    if (MAYSPLIT && (!TAIL || is_tail)) {
      // park the partial tile: block [tile][split][piece], piece = (j * NMW + MFMA wave) * 64 + lane - every wave instruction writes
      // 1 KiB contiguous; the last workgroup reads the S blocks with the same lane mapping
      constexpr int TILE = BM * BN; // floats per partial
      const int S = nsplit;
      float *scr = p.scratch + (size_t)tile_id * S * TILE;
      const __amdgpu_buffer_rsrc_t rsrcS = __builtin_amdgcn_make_buffer_rsrc((void *)scr, 0, 0x7fffffff, 0x00020000);
      const unsigned pvo = (unsigned)((wave * 64 + lane) * 16);
#pragma unroll
      for (int j = 0; j < IPG; ++j)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, part[j]), rsrcS, pvo, (unsigned)((sp * TILE + j * NMW * 256) * 4), 16);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the write-through stores of this wave have been acknowledged
      __syncthreads();                                  // ... and those of every MFMA wave (red is free again)
      unsigned *flag = (unsigned *)smem_lw;
      if (wave == 0 && lane == 0)
        *flag = __hip_atomic_fetch_add((g_u32_lw *)(p.split_cnt + tile_id), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __syncthreads();
      if (*flag != (unsigned)(S - 1)) return; // not the last to arrive: done
      if (wave == 0 && lane == 0) __hip_atomic_store((g_u32_lw *)(p.split_cnt + tile_id), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // for the next launch
      // the ordered sum: partial 0 + partial 1 + ... (sc1 loads: the blocks were written by workgroups behind other L2s)
#pragma unroll
      for (int j = 0; j < IPG; ++j) {
        f32x4 acc4 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrcS, pvo, (unsigned)((j * NMW * 256) * 4), 16));
        int s2 = 1;
        for (; s2 + 4 <= S; s2 += 4) { // four loads in flight, added in order
          f32x4 t[4];
#pragma unroll
          for (int e = 0; e < 4; ++e)
            t[e] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrcS, pvo, (unsigned)(((s2 + e) * TILE + j * NMW * 256) * 4), 16));
#pragma unroll
          for (int e = 0; e < 4; ++e) acc4 += t[e];
        }
        for (; s2 < S; ++s2)
          acc4 += __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrcS, pvo, (unsigned)((s2 * TILE + j * NMW * 256) * 4), 16));
        part[j] = acc4;
      }
#pragma unroll
      for (int j = 0; j < IPG; ++j) { // ... + C (beta = 1)
        if (!(p.ep & EP_BETA0) && piece_ok) part[j] += __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrcC, Tile::tail_off(tl, j), 0, 0));
      }
    }
    Tile::finish(part, bias4, p.ep, rsrcC, piece_ok, tl);
    return;
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float v = acc[r] + bias;
    if (p.ep & EP_RELU) v = v > 0.0f ? v : 0.0f;
    if (!RAGN || ccol < p.n)
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsrcC, voffC,
                                            (unsigned)((r & 3) + 8 * (r >> 2)) * ldcb, LW_C_AUX);
  }
}

// ---- a CHAIN of whole-layer f32 BRGEMMs in one launch ------------------------------------------------------------------------
// The reference's MLP benchmark (mlir-gen --batch=256 --layers=1024,1024,1024,1024, fp32, benchmarks/config/base/base.json:74-80)
// lowers to one whole-layer xsmm_fused_brgemm_invoke per layer; a layer of 256 x 1024 x 1024 is 3.4 us of MFMA work behind a
// 2.5 us launch. xsmm_hip_fused_brgemm_chain_invoke (runtime.cpp) runs the layers of such a step as ONE launch of this kernel: the
// same tile, the same loader-wave structure, the same order of additions as brgemm_f32_lw<WM, WN, WK> - both kernels are built from
// LwTile<WM, WN, WK>, brgemm_f32_lw_tile.h - (results bit-identical to the separate launches), one workgroup per output tile, all co-resident (tiles <= CUs), and between two layers the hand-off of
// the bf16 chain (brgemm_bf16_lw.hip): a tile is stored with 16-byte write-through stores, every storing wave drains them, the
// workgroup adds 1 to the arrival counter of its ROW BLOCK; the A loaders of the next layer wait until all tiles_n tiles of their
// row block have arrived and fetch the rows with sc1 loads (another XCD's L2 may hold them). Counters only grow (target = epoch x
// tiles_n, runtime.cpp); every spin is bounded (CHAIN_TIMEOUT_TICKS) and reports through p.err instead of hanging the GPU.
// The ring restarts at slot 0 with every layer (the K-group combine parks its partials in slot 0): the B loader of layer l+1
// requests its first chunks right behind the seam barrier, while the A loaders still poll.
//   barriers per layer, every wave: P (chunk 0 published), T - 1 mid-chunk barriers, R1 + R2 (combine), S1 (tile stored and
//   drained; not after the last layer)
typedef __attribute__((address_space(1))) unsigned int g_u32_f32c;
template <int WM, int WN, int WK, int NL>
__global__ __launch_bounds__(64 * (WM * WN * WK + 2 * NL)) void brgemm_f32_lw_chain(ChainArgs p) {
  static_assert(WK > 1, "the hand-off needs the 16-byte stores of the K-split tiles' epilogue");
  using Tile = LwTile<WM, WN, WK>;
  constexpr int NMW = Tile::NMW, BM = Tile::BM, BN = Tile::BN;

  const int tid = threadIdx.x, lane = tid & 63;
  const int hw_wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave = hw_wave < 2 * NL ? NMW + hw_wave : hw_wave - 2 * NL; // loaders first, as in brgemm_f32_lw
  const int tm = (int)blockIdx.x / p.tiles_n, tn = (int)blockIdx.x % p.tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;
  const int L = p.nlayers;

  if (wave >= NMW) {
    // ---- loader waves ------------------------------------------------------------------------------------------
    const bool isA = (wave - NMW) < NL;
    for (int l = 0; l < L; ++l) {
      const ChainLayer &Y = p.L[l];
      const int lda = (int)(l == 0 ? p.lda : p.L[l > 0 ? l - 1 : 0].ldc);
      const float *Asrc = (const float *)(l == 0 ? p.A : p.L[l > 0 ? l - 1 : 0].C);
      const int kchunks = Y.k / LW_BK;
      typename Tile::template Loader<NL, NL> ld(wave - NMW, lane, Asrc, (const float *)Y.B, m0, n0, lda, (int)Y.ldb, Y.stride_a, Y.stride_b, kchunks, false, BN);
      const bool sc1 = isA && l > 0; // rows written by other workgroups of THIS launch
      if (sc1) {
        // every producer tile of row block tm of layer l-1 has been stored (write-through) and drained
        g_u32_f32c *c = (g_u32_f32c *)(p.cnt + ((size_t)(l - 1) * p.tiles_m + tm) * CHAIN_CNT_STRIDE);
        const unsigned target = p.target;
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        for (;;) {
          const unsigned v = __hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if ((int)(v - target) >= 0) break;
          if (__builtin_amdgcn_s_memrealtime() - t0 > CHAIN_TIMEOUT_TICKS) { // never hang the GPU: flag it and go on
            if (lane == 0) __hip_atomic_store((g_u32_f32c *)p.err, 1u + (unsigned)l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
          }
          __builtin_amdgcn_s_sleep(1);
        }
        asm volatile("" ::: "memory");
      }
      lw_loader_schedule<LW_NSLOT>(Y.br * kchunks, [&](int slot) __attribute__((always_inline)) { ld.template issue<true>(slot, sc1); },
                                   [&](int chunks) __attribute__((always_inline)) { ld.wait_left(chunks); }, // P, T - 1 mid-chunk barriers
                                   [&]() __attribute__((always_inline)) { ld.template issue_first<true>(sc1); });
      __builtin_amdgcn_s_barrier(); // R1
      __builtin_amdgcn_s_barrier(); // R2
      if (l + 1 < L) __builtin_amdgcn_s_barrier(); // S1
    }
    return;
  }

  // ---- MFMA waves ------------------------------------------------------------------------------------------------
  const typename Tile::Wave w(wave, lane);
  // (the fragment addresses are the same for every layer: the ring restarts at slot 0. Held across the seams they cost the 64x64 + K2
  // instance a wave per SIMD in the compiler's resource report: that instance keeps the setup where it was)
  constexpr bool CHAIN_PIN = !(WM == 2 && WN == 2);
  const auto fr = Tile::template mfma_setup<CHAIN_PIN>(w);
  for (int l = 0; l < L; ++l) {
    const ChainLayer &Y = p.L[l];
    const int ldc = (int)Y.ldc;
    const __amdgpu_buffer_rsrc_t rsrcC = __builtin_amdgcn_make_buffer_rsrc((void *)((float *)Y.C + (int64_t)m0 * ldc + n0), 0, 0x7fffffff, 0x00020000);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const auto tl = Tile::template tail_setup<CHAIN_PIN>(w, ldc); // at every seam: above the barrier, as in brgemm_f32_lw
    const int T = Tile::template pin_chunks<CHAIN_PIN>(Y.br * (Y.k / LW_BK));
    __builtin_amdgcn_s_barrier(); // P
    __builtin_amdgcn_sched_barrier(0);
    Tile::mfma_chunks(acc, T, fr);
    // combine the K groups and store, exactly as brgemm_f32_lw does (group order; bias; relu; 16-byte write-through stores)
    Tile::park_partials(acc, tl); // R1, R2
    f32x4 bias4 = {0.0f, 0.0f, 0.0f, 0.0f}, part[Tile::IPG];
    if (Y.ep & EP_BIAS) bias4 = *(const f32x4 *)((const float *)Y.D + n0 + w.wn * 32 + 4 * (lane & 7));
    Tile::sum_partials(part, tl);
    Tile::finish(part, bias4, Y.ep, rsrcC, true, tl);
    if (l + 1 == L) break;
    // ---- seam: publish this tile to the row block's consumers ---------------------------------------------------
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); // every storing wave drains its write-through stores (and is done with the parked partials)
    __builtin_amdgcn_s_barrier();                                // S1
    if (wave == 0 && lane == 0)
      __hip_atomic_fetch_add((g_u32_f32c *)(p.cnt + ((size_t)l * p.tiles_m + tm) * CHAIN_CNT_STRIDE), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- EDGE TILES: a whole-layer call whose m or n is not a multiple of the tile (opt-in, xsmm_hip_set_edge_tiles) ----------------
// One workgroup per tile of the ceil(m / BM) x ceil(n / BN) grid, m >= BM, n >= BN, n a multiple of 4. A 32x32 MFMA accumulator computes
// each output element from its own row of A and column of B, in an order that does not depend on where the tile sits - so the last
// tile of a row or column of tiles is SHIFTED BACK inside the matrix: tile (tm, tn) computes the BM x BN block at m0 = min(tm BM, m -
// BM), n0 = min(tn BN, n - BN) (n0 stays a multiple of 4: the 16-byte pieces of B, of the bias row and of C keep their alignment) and
// OWNS rows >= tm BM - m0 and columns >= tn BN - n0 of it. Every load of the loader waves stays inside rows [0, m) of A and columns
// [0, n) of B without a clamp in their issue loop; the LDS images, the chunk loop and the K-group combine are the tile's, untouched. The
// epilogue joins C (beta = 1) and stores only what the tile owns: the rest of its block belongs to the neighbour, which may already have
// rewritten it. No scratch block, no counters, no waiting - legal on a captured stream and in strict mode.
// A kernel of its own around LwTile, like the chain kernel, and not a tenth template argument of brgemm_f32_lw: every instance of that
// kernel keeps its symbol and its code (tests/test_tail_split_host.py finds the tail instances by their mangled names).
template <int WM, int WN, int WK, int NL, int NSLOT, int NLB>
__global__ __launch_bounds__(64 * (WM * WN * WK + NL + NLB)) void brgemm_f32_lw_edge(GemmArgs p) {
  using Tile = LwTile<WM, WN, WK, NSLOT>;
  constexpr int NMW = Tile::NMW, BM = Tile::BM, BN = Tile::BN, IPG = Tile::IPG;

  const int tid = threadIdx.x, lane = tid & 63;
  const int hw_wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave = hw_wave < NL + NLB ? NMW + hw_wave : hw_wave - (NL + NLB); // loaders first, as in brgemm_f32_lw
  // XCD-blocked (8, bn, bm) or plain (1, tiles_n, tiles_m) grid over the ceil-divided tile counts, as brgemm_f32_lw's
  const int tm = (int)(blockIdx.x >> p.xn_shift) * p.tiles_m + (int)blockIdx.z;
  const int tn = (int)(blockIdx.x & ((1u << p.xn_shift) - 1)) * p.tiles_n + (int)blockIdx.y;
  const int m0 = tm * BM < p.m - BM ? tm * BM : p.m - BM, n0 = tn * BN < p.n - BN ? tn * BN : p.n - BN;
  const int own_r = tm * BM - m0, own_c = tn * BN - n0; // 0, 0 for every tile but the last of a ragged row / column of tiles
  // (the loader path's arguments in one batch above the role branch: brgemm_f32_lw)
  const float *A_ = (const float *)p.A, *B_ = (const float *)p.B;
  int lda = (int)p.lda, ldb = (int)p.ldb;
  int64_t stride_a = p.stride_a, stride_b = p.stride_b;
  asm volatile("" : "+s"(A_), "+s"(B_), "+s"(lda), "+s"(ldb), "+s"(stride_a), "+s"(stride_b));
  const float *__restrict__ A = A_;
  const float *__restrict__ B = B_;
  float *__restrict__ C = (float *)p.C;
  const int kchunks = p.k / LW_BK;
  const int T = p.br * kchunks;

  if (wave >= NMW) {
    typename Tile::template Loader<NL, NLB> ld(wave - NMW, lane, A, B, m0, n0, lda, ldb, stride_a, stride_b, kchunks, false, BN);
    lw_loader_schedule<NSLOT>(T, [&](int slot) __attribute__((always_inline)) { ld.issue(slot); },
                              [&](int chunks) __attribute__((always_inline)) { ld.wait_left(chunks); },
                              [&]() __attribute__((always_inline)) { ld.issue_first(); });
    return;
  }

  const typename Tile::Wave w(wave, lane);
  const int wk = w.wk, wm = w.wm, wn = w.wn;
  const int li = lane & 31, lh = lane >> 5;
  const __amdgpu_buffer_rsrc_t rsrcC =
      __builtin_amdgcn_make_buffer_rsrc((void *)(C + (int64_t)m0 * p.ldc + n0), 0, 0x7fffffff, 0x00020000);
  const unsigned voffC = (unsigned)(((wm * 32 + 4 * lh) * (int)p.ldc + wn * 32 + li) * 4);
  const unsigned ldcb = (unsigned)((int)p.ldc * 4);
  // accumulator register r of a lane: row wm 32 + 4 lh + (r & 3) + 8 (r >> 2), column wn 32 + li of the tile
  const bool col_owned = wn * 32 + li >= own_c;
  const int row_first = own_r - (wm * 32 + 4 * lh); // register r is owned if (r & 3) + 8 (r >> 2) >= row_first
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  float bias = 0.0f;
  if constexpr (WK == 1) {
    if (p.ep & EP_BIAS) bias = ((const float *)p.D)[n0 + wn * 32 + li];
  }
  constexpr bool BIAS_EARLY = WK > 1 && WM * WN * WK <= 4; // (brgemm_f32_lw)
  f32x4 bias4 = {0.0f, 0.0f, 0.0f, 0.0f};
  if constexpr (BIAS_EARLY) {
    if (p.ep & EP_BIAS) bias4 = *(const f32x4 *)((const float *)p.D + n0 + wn * 32 + 4 * (lane & 7));
  }
  // beta = 1: C joins the chain of K group 0 - only where the tile owns it; elsewhere the neighbour may already have stored
  if (wk == 0 && !(p.ep & EP_BETA0) && col_owned) {
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if ((r & 3) + 8 * (r >> 2) >= row_first)
        acc[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrcC, voffC, (unsigned)((r & 3) + 8 * (r >> 2)) * ldcb, 0));
  }

  const auto fr = Tile::mfma_setup(w); // (above the barrier: brgemm_f32_lw)
  const auto tl = Tile::tail_setup(w, (int)p.ldc);
  const int Tp = Tile::pin_chunks(T);

  __builtin_amdgcn_s_barrier(); // chunk 0 published
  __builtin_amdgcn_sched_barrier(0);
  if (Tp > 0) Tile::mfma_chunks(acc, Tp, fr);

  if constexpr (WK > 1) {
    Tile::park_partials(acc, tl);
    if constexpr (!BIAS_EARLY) {
      if (p.ep & EP_BIAS) bias4 = *(const f32x4 *)((const float *)p.D + n0 + wn * 32 + 4 * (lane & 7));
    }
    f32x4 part[IPG];
    Tile::sum_partials(part, tl);
    Tile::finish_owned(part, bias4, p.ep, rsrcC, own_r, own_c, w, tl);
    return;
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float v = acc[r] + bias;
    if (p.ep & EP_RELU) v = v > 0.0f ? v : 0.0f;
    if (col_owned && (r & 3) + 8 * (r >> 2) >= row_first)
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsrcC, voffC, (unsigned)((r & 3) + 8 * (r >> 2)) * ldcb, LW_C_AUX);
  }
}

// ---- RAGGED k: a whole-layer call whose k is not a multiple of 64 (opt-in, xsmm_hip_set_edge_k) ------------------------------------
// k >= 64, k % 8 == 0, k % 64 != 0, at least one batch element. Every batch element is ceil(k / 64) chunks; the last one is SHIFTED
// BACK to start at k - 64, so that it ends at k - no load leaves columns [0, k) of A or rows [0, k) of B, the start stays on 32
// bytes - and the MFMA waves SKIP the k-blocks at its head that the chunk before it has multiplied (brgemm_f32_lw_kedge.h: the
// schedule; Loader::issue_ragged, LwTile::mfma_chunks_ragged: the two places that know of it). Nothing is multiplied by zero: an Inf
// or NaN in the overlap counts once, as data. The workgroup is otherwise the edge tile's, shifted-back last tile row and column and
// ownership mask included (own_r = own_c = 0 when the tile divides m and n), so ONE kernel serves the ragged-k layer with divisible m
// and n and the layer ragged in all three. A kernel of its own, its body the edge kernel's line for line but for the three marked
// places: sharing the body as a function changed the code of the four edge instances, and no existing instance may change.
template <int WM, int WN, int WK, int NL, int NSLOT, int NLB>
__global__ __launch_bounds__(64 * (WM * WN * WK + NL + NLB)) void brgemm_f32_lw_kedge(GemmArgs p) {
  using Tile = LwTile<WM, WN, WK, NSLOT>;
  constexpr int NMW = Tile::NMW, BM = Tile::BM, BN = Tile::BN, IPG = Tile::IPG;

  const int tid = threadIdx.x, lane = tid & 63;
  const int hw_wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave = hw_wave < NL + NLB ? NMW + hw_wave : hw_wave - (NL + NLB); // loaders first, as in brgemm_f32_lw
  // the grid, the shifted-back last tile row / column and what the tile owns: brgemm_f32_lw_edge
  const int tm = (int)(blockIdx.x >> p.xn_shift) * p.tiles_m + (int)blockIdx.z;
  const int tn = (int)(blockIdx.x & ((1u << p.xn_shift) - 1)) * p.tiles_n + (int)blockIdx.y;
  const int m0 = tm * BM < p.m - BM ? tm * BM : p.m - BM, n0 = tn * BN < p.n - BN ? tn * BN : p.n - BN;
  const int own_r = tm * BM - m0, own_c = tn * BN - n0; // 0, 0 for every tile but the last of a ragged row / column of tiles
  // (the loader path's arguments in one batch above the role branch: brgemm_f32_lw)
  const float *A_ = (const float *)p.A, *B_ = (const float *)p.B;
  int lda = (int)p.lda, ldb = (int)p.ldb;
  int64_t stride_a = p.stride_a, stride_b = p.stride_b;
  asm volatile("" : "+s"(A_), "+s"(B_), "+s"(lda), "+s"(ldb), "+s"(stride_a), "+s"(stride_b));
  const float *__restrict__ A = A_;
  const float *__restrict__ B = B_;
  float *__restrict__ C = (float *)p.C;
  const int kchunks = kedge_chunks(p.k); // >= 2
  const int T = p.br * kchunks;

  if (wave >= NMW) {
    typename Tile::template Loader<NL, NLB> ld(wave - NMW, lane, A, B, m0, n0, lda, ldb, stride_a, stride_b, kchunks, false, BN);
    lw_loader_schedule<NSLOT>(T, [&](int slot) __attribute__((always_inline)) { ld.issue_ragged(slot); },
                              [&](int chunks) __attribute__((always_inline)) { ld.wait_left(chunks); },
                              [&]() __attribute__((always_inline)) { ld.issue_first_ragged(p.k); });
    return;
  }

  const typename Tile::Wave w(wave, lane);
  const int wk = w.wk, wm = w.wm, wn = w.wn;
  const int li = lane & 31, lh = lane >> 5;
  const __amdgpu_buffer_rsrc_t rsrcC =
      __builtin_amdgcn_make_buffer_rsrc((void *)(C + (int64_t)m0 * p.ldc + n0), 0, 0x7fffffff, 0x00020000);
  const unsigned voffC = (unsigned)(((wm * 32 + 4 * lh) * (int)p.ldc + wn * 32 + li) * 4);
  const unsigned ldcb = (unsigned)((int)p.ldc * 4);
  // accumulator register r of a lane: row wm 32 + 4 lh + (r & 3) + 8 (r >> 2), column wn 32 + li of the tile
  const bool col_owned = wn * 32 + li >= own_c;
  const int row_first = own_r - (wm * 32 + 4 * lh); // register r is owned if (r & 3) + 8 (r >> 2) >= row_first
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  float bias = 0.0f;
  if constexpr (WK == 1) {
    if (p.ep & EP_BIAS) bias = ((const float *)p.D)[n0 + wn * 32 + li];
  }
  constexpr bool BIAS_EARLY = WK > 1 && WM * WN * WK <= 4; // (brgemm_f32_lw)
  f32x4 bias4 = {0.0f, 0.0f, 0.0f, 0.0f};
  if constexpr (BIAS_EARLY) {
    if (p.ep & EP_BIAS) bias4 = *(const f32x4 *)((const float *)p.D + n0 + wn * 32 + 4 * (lane & 7));
  }
  // beta = 1: C joins the chain of K group 0 - only where the tile owns it; elsewhere the neighbour may already have stored
  if (wk == 0 && !(p.ep & EP_BETA0) && col_owned) {
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if ((r & 3) + 8 * (r >> 2) >= row_first)
        acc[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrcC, voffC, (unsigned)((r & 3) + 8 * (r >> 2)) * ldcb, 0));
  }

  // (not pinned above the barrier: the ragged laps need the registers - brgemm_f32_lw_tile.h mfma_setup)
  const auto fr = Tile::template mfma_setup<false>(w);
  const auto tl = Tile::template tail_setup<false>(w, (int)p.ldc);
  const int Tp = T;

  __builtin_amdgcn_s_barrier(); // chunk 0 published
  __builtin_amdgcn_sched_barrier(0);
  Tile::mfma_chunks_ragged(acc, Tp, kchunks, kedge_skip_blocks(p.k, kchunks - 1), fr);

  if constexpr (WK > 1) {
    Tile::park_partials(acc, tl);
    if constexpr (!BIAS_EARLY) {
      if (p.ep & EP_BIAS) bias4 = *(const f32x4 *)((const float *)p.D + n0 + wn * 32 + 4 * (lane & 7));
    }
    f32x4 part[IPG];
    Tile::sum_partials(part, tl);
    Tile::finish_owned(part, bias4, p.ep, rsrcC, own_r, own_c, w, tl);
    return;
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float v = acc[r] + bias;
    if (p.ep & EP_RELU) v = v > 0.0f ? v : 0.0f;
    if (col_owned && (r & 3) + 8 * (r >> 2) >= row_first)
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsrcC, voffC, (unsigned)((r & 3) + 8 * (r >> 2)) * ldcb, LW_C_AUX);
  }
}

// ---- launchers --------------------------------------------------------------------------------------------------------------
// The XCD blocks of a whole-layer grid: xm x xn = 8 blocks of tiles_m/xm x tiles_n/xn tiles, one per XCD. Each XCD's L2 then fetches
// m/xm rows of A and n/xn columns of B: the split that minimises m/xm + n/xn - 4 x 2 for square outputs (C2; ties keep it: rounds
// 1-3 had only this one), 2 x 4 for C3's 512 x 1024 and the batch-256 layers (-20 / -33 % of the L2 fill). Returns xm, 0 = the
// tile grid does not divide into 8 blocks.
static int lw_xcd_blocks(const GemmArgs &a, int tiles_m, int tiles_n) {
  int xm = 0;
  long long best = -1;
  for (int c : {4, 2, 8, 1}) {
    const int xn = 8 / c;
    if (tiles_m % c || tiles_n % xn || tiles_m / c > 65535 || tiles_n / xn > 65535) continue;
    const long long cost = (long long)a.m / c + (long long)a.n / xn;
    if (best < 0 || cost < best) {
      best = cost;
      xm = c;
    }
  }
  return xm;
}

// The grid of a whole-layer launch: fills args.tiles_m / tiles_n / xn_shift with the tiles of ONE XCD block and log2 of the blocks
// along N (blockIdx.x or workgroup id mod 8 = the XCD: workgroups go to XCDs round robin) and returns true, or - the tile grid does
// not divide into 8 blocks, or the caller does not allow them - with the whole tile grid as one block and returns false.
static bool lw_xcd_grid(GemmArgs &args, int tiles_m, int tiles_n, bool allow_blocks = true) {
  const int xm = allow_blocks ? lw_xcd_blocks(args, tiles_m, tiles_n) : 0, xn = xm ? 8 / xm : 1;
  args.tiles_m = xm ? tiles_m / xm : tiles_m;
  args.tiles_n = tiles_n / xn;
  args.xn_shift = xn == 8 ? 3 : xn == 4 ? 2 : xn == 2 ? 1 : 0;
  return xm != 0;
}

// SPLIT / TAIL launches: `tiles` partial-tile blocks of S x tile_floats and their arrival counters in the launch stream's scratch
// block (split_scratch.h). false: no scratch block - nothing is launched, the caller falls back to the unsplit launch.
static bool lw_split_scratch(GemmArgs &args, hipStream_t s, long long tiles, int S, int tile_floats) {
  const SplitScratch *sc = split_scratch_for(s, tiles, tiles * S * tile_floats);
  if (!sc) return false;
  args.split = S;
  args.scratch = sc->partial;
  args.split_cnt = sc->cnt;
  return true;
}

// One kernel instance, named ONCE: its workgroup size and LDS bytes follow from the same template arguments as the kernel itself,
// and lw_launch<I> keeps the per-instance (and per-device: ensure_dynamic_lds) record of the dynamic-LDS attribute.
template <int WM, int WN, int WK, bool GROUPED = false, int NL = 1, int NSLOT = LW_NSLOT, int NLB = NL, bool SPLIT = false, bool TAIL = false> struct LwLayer {
  using Tile = LwTile<WM, WN, WK, NSLOT>;
  static constexpr int NT = 64 * (Tile::NMW + NL + NLB);
  static constexpr auto kernel = brgemm_f32_lw<WM, WN, WK, GROUPED, NL, NSLOT, NLB, SPLIT, TAIL>;
};
template <int WM, int WN, int WK, int NL> struct LwChain {
  using Tile = LwTile<WM, WN, WK>;
  static constexpr int NT = 64 * (Tile::NMW + 2 * NL);
  static constexpr auto kernel = brgemm_f32_lw_chain<WM, WN, WK, NL>;
};
template <int WM, int WN, int WK, int NL, int NSLOT, int NLB> struct LwEdge {
  using Tile = LwTile<WM, WN, WK, NSLOT>;
  static constexpr int NT = 64 * (Tile::NMW + NL + NLB);
  static constexpr auto kernel = brgemm_f32_lw_edge<WM, WN, WK, NL, NSLOT, NLB>;
};
template <int WM, int WN, int WK, int NL, int NSLOT, int NLB> struct LwKEdge {
  using Tile = LwTile<WM, WN, WK, NSLOT>;
  static constexpr int NT = 64 * (Tile::NMW + NL + NLB);
  static constexpr auto kernel = brgemm_f32_lw_kedge<WM, WN, WK, NL, NSLOT, NLB>;
};
template <class I, class... Args> static hipError_t lw_launch(dim3 grid, hipStream_t s, const Args &...args) {
  static std::atomic<unsigned long long> lds_set{0};
  if (hipError_t e = ensure_dynamic_lds((const void *)I::kernel, (int)I::Tile::LDS_BYTES, lds_set); e != hipSuccess) return e;
  hipLaunchKernelGGL(I::kernel, grid, dim3(I::NT), I::Tile::LDS_BYTES, s, args...);
  return hipGetLastError();
}

template <int WM, int WN, int WK, int NL = 1, int NSLOT = LW_NSLOT, int NLB = NL> static hipError_t launch_lw_t(const GemmArgs &a, hipStream_t s) {
  using I = LwLayer<WM, WN, WK, false, NL, NSLOT, NLB>;
  GemmArgs args = a;
  // XCD-blocked grid (8, block's tiles_n, block's tiles_m), else (1, tiles_n, tiles_m)
  const bool blocks = lw_xcd_grid(args, a.m / I::Tile::BM, a.n / I::Tile::BN);
  if (args.tiles_m > 65535 || args.tiles_n > 65535) return hipErrorInvalidValue;
  return lw_launch<I>(dim3(blocks ? 8 : 1, args.tiles_n, args.tiles_m), s, args, (const WorkItem *)nullptr);
}

// grouped launch (tile queue): one workgroup per (item, tile of the item); m multiple of the tile, k of 64 - or k = 32 with
// even batch counts and 0 <= stride < 2^26 elements (the kernel's pair mode). S > 1: a SPLIT launch, grid (items * S, tiles_n, tiles_m)
template <int WM, int WN, int WK, bool SPLIT>
static hipError_t launch_lw_grouped_t(const GemmArgs &a, const WorkItem *items, int n_items, int S, hipStream_t s) {
  using I = LwLayer<WM, WN, WK, true, 1, LW_NSLOT, 1, SPLIT>;
  constexpr int BM = I::Tile::BM, BN = I::Tile::BN;
  const int tiles_m = a.m / BM, tiles_n = (a.n + BN - 1) / BN;
  GemmArgs args = a;
  args.tiles_m = args.tiles_n = 0;
  args.xn_shift = 0;
  if (SPLIT && !lw_split_scratch(args, s, (long long)n_items * tiles_m * tiles_n, S, BM * BN)) return hipErrorOutOfMemory;
  return lw_launch<I>(dim3((unsigned)(n_items * (SPLIT ? S : 1)), tiles_n, tiles_m), s, args, items);
}

// ---- SPLIT launches: S workgroups per output tile (kernel comment; scratch: split_scratch.h) ----------------------------------
// whole-layer call: linear grid of S * tiles workgroups
template <int WM, int WN, int WK> static hipError_t launch_lw_split_t(const GemmArgs &a, int S, hipStream_t s) {
  using I = LwLayer<WM, WN, WK, false, 1, LW_NSLOT, 1, true>;
  constexpr int BM = I::Tile::BM, BN = I::Tile::BN;
  GemmArgs args = a;
  args.tiles_m = a.m / BM;
  args.tiles_n = (a.n + BN - 1) / BN;
  args.xn_shift = 0;
  const long long tiles = (long long)args.tiles_m * args.tiles_n;
  if (!lw_split_scratch(args, s, tiles, S, BM * BN)) return hipErrorOutOfMemory; // the caller falls back to the unsplit launch
  return lw_launch<I>(dim3((unsigned)(tiles * S)), s, args, (const WorkItem *)nullptr);
}
// whole-layer call with a split tail (kernel comment, TAIL): linear grid, the body workgroups first, then S per tail tile. Scratch
// and counters for the tail tiles only. m, n multiples of the tile (the planner's tile choice); tail_tiles < tiles, S >= 2.
template <int WM, int WN, int WK, int NL, int NLB> static hipError_t launch_lw_tail_t(const GemmArgs &a, int tail_tiles, int S, hipStream_t s) {
  using I = LwLayer<WM, WN, WK, false, NL, LW_NSLOT, NLB, false, true>;
  constexpr int BM = I::Tile::BM, BN = I::Tile::BN;
  const int tiles_m = a.m / BM, tiles_n = a.n / BN;
  const long long tiles = (long long)tiles_m * tiles_n, body = tiles - tail_tiles;
  if (a.m % BM || a.n % BN || tail_tiles <= 0 || body <= 0 || S < 2 || S > SPLIT_MAX || body + (long long)tail_tiles * S > 0x7fffffffLL)
    return hipErrorInvalidValue;
  GemmArgs args = a;
  if (!lw_split_scratch(args, s, tail_tiles, S, BM * BN)) return hipErrorOutOfMemory; // the caller falls back to the plain launch
  lw_xcd_grid(args, tiles_m, tiles_n, body % 8 == 0 && tail_tiles % 8 == 0); // every XCD block: body / 8 body tiles, then tail_tiles / 8 tail tiles
  args.tail_body = (int)body;
  return lw_launch<I>(dim3((unsigned)(body + (long long)tail_tiles * S)), s, args, (const WorkItem *)nullptr);
}

// whole-layer call on EDGE tiles (brgemm_f32_lw_edge): ceil(m / BM) x ceil(n / BN) workgroups in XCD blocks where the tile counts divide
template <int WM, int WN, int WK, int NL = 1, int NSLOT = LW_NSLOT, int NLB = NL> static hipError_t launch_lw_edge_t(const GemmArgs &a, hipStream_t s) {
  using I = LwEdge<WM, WN, WK, NL, NSLOT, NLB>;
  constexpr int BM = I::Tile::BM, BN = I::Tile::BN;
  if (a.m < BM || a.n < BN || (a.n & 3) || a.k <= 0 || a.k % LW_BK || a.br < 1) return hipErrorInvalidValue;
  GemmArgs args = a;
  const bool blocks = lw_xcd_grid(args, (a.m + BM - 1) / BM, (a.n + BN - 1) / BN);
  if (args.tiles_m > 65535 || args.tiles_n > 65535) return hipErrorInvalidValue;
  return lw_launch<I>(dim3(blocks ? 8 : 1, args.tiles_n, args.tiles_m), s, args);
}

// whole-layer call with a RAGGED k (brgemm_f32_lw_kedge): the edge launcher's grid
template <int WM, int WN, int WK, int NL = 1, int NSLOT = LW_NSLOT, int NLB = NL> static hipError_t launch_lw_kedge_t(const GemmArgs &a, hipStream_t s) {
  using I = LwKEdge<WM, WN, WK, NL, NSLOT, NLB>;
  constexpr int BM = I::Tile::BM, BN = I::Tile::BN;
  if (a.m < BM || a.n < BN || (a.n & 3) || !kedge_k_ok(a.k) || a.br < 1) return hipErrorInvalidValue;
  GemmArgs args = a;
  const bool blocks = lw_xcd_grid(args, (a.m + BM - 1) / BM, (a.n + BN - 1) / BN);
  if (args.tiles_m > 65535 || args.tiles_n > 65535) return hipErrorInvalidValue;
  return lw_launch<I>(dim3(blocks ? 8 : 1, args.tiles_n, args.tiles_m), s, args);
}

// ---- HALVES: a 64x64 + K2 layer as two 64x32 + K2 workgroups per output tile (xsmm_hip_set_f32_halves; gemm_plan.cpp choose_f32_halves) -
// LwTile<2, 1, 2, 3>: 4 MFMA waves = the two K groups of ONE 32-column half of the 64x64 + K2 tile, on a 3-slot ring of 24 KiB slots
// (72 KiB: two workgroups fit a CU's 160 KiB, 7 waves each). Every output element gets what the 64x64 + K2 tile gives it: K group 0's
// chain over k 0..31 of every chunk, group 1's over k 32..63, summed in group order - the bits of launch_f32_lw(1). (The 64x32 + K4
// tile of launch_f32_lw(2) splits a chunk four ways: other bits.) Each SIMD then holds one MFMA wave of each of two INDEPENDENT
// workgroups - own barrier, own ring, own loaders - instead of two waves that meet the same barrier. No workgroup waits for another and
// nothing requires the two to be co-resident. The grid is launch_lw_t's with BN = 32: the halves of a tile are neighbours along the
// grid's y in one XCD block wherever the block's width in halves is even. m, n multiples of 64 (whole 64x64 tiles), k of 64.
// hipErrorInvalidValue: not launched, use launch_f32_lw(1).
hipError_t launch_f32_lw_halves(const GemmArgs &a, hipStream_t s) {
  if (a.m <= 0 || a.n <= 0 || a.m % 64 || a.n % 64 || a.k <= 0 || a.k % LW_BK || a.br < 0) return hipErrorInvalidValue;
  // loader waves: two for the A panel (16 requests per chunk) and one for B (8), every loader issues 8. C2, six alternating runs on one
  // box (profiles/f32_halves_ab.txt): 17.17-17.22 us; one loader per panel 17.27-17.31; the 64x64 + K2 tile 17.63-17.67
  return launch_lw_t<2, 1, 2, 2, 3, 1>(a, s);
}

// tile as in launch_f32_lw; split > 1: that many workgroups per output tile (K-split tiles 1 .. 3 only); n may end inside the last tile
hipError_t launch_f32_lw_grouped(int tile, const GemmArgs &a, const WorkItem *items, int n_items, int split, hipStream_t s) {
  if (split > 1) {
    hipError_t e = hipErrorInvalidValue;
    switch (tile) {
    case 1: e = launch_lw_grouped_t<2, 2, 2, true>(a, items, n_items, split, s); break;
    case 2: e = launch_lw_grouped_t<2, 1, 4, true>(a, items, n_items, split, s); break;
    case 3: e = launch_lw_grouped_t<1, 1, 4, true>(a, items, n_items, split, s); break;
    default: break;
    }
    if (e != hipErrorOutOfMemory && e != hipErrorInvalidValue) return e;
    (void)hipGetLastError(); // no scratch block (or a tile without a split instance): the unsplit launch
  }
  switch (tile) {
  case 0: return launch_lw_grouped_t<2, 2, 1, false>(a, items, n_items, 1, s);
  case 1: return launch_lw_grouped_t<2, 2, 2, false>(a, items, n_items, 1, s);
  case 2: return launch_lw_grouped_t<2, 1, 4, false>(a, items, n_items, 1, s);
  case 3: return launch_lw_grouped_t<1, 1, 4, false>(a, items, n_items, 1, s);
  default: return hipErrorInvalidValue;
  }
}
// whole-layer call on S workgroups per tile; hipErrorOutOfMemory / hipErrorInvalidValue: not launched, use launch_f32_lw
hipError_t launch_f32_lw_split(int tile, const GemmArgs &a, int split, hipStream_t s) {
  switch (tile) {
  case 1: return launch_lw_split_t<2, 2, 2>(a, split, s);
  case 2: return launch_lw_split_t<2, 1, 4>(a, split, s);
  case 3: return launch_lw_split_t<1, 1, 4>(a, split, s);
  default: return hipErrorInvalidValue;
  }
}

// whole-layer call whose last tail_tiles tiles run on `split` workgroups each; loader waves per tile as launch_f32_lw.
// hipErrorOutOfMemory / hipErrorInvalidValue: not launched, use launch_f32_lw
hipError_t launch_f32_lw_tail(int tile, const GemmArgs &a, int tail_tiles, int split, hipStream_t s) {
  switch (tile) {
  case 1: return launch_lw_tail_t<2, 2, 2, 2, 2>(a, tail_tiles, split, s);
  case 2: return launch_lw_tail_t<2, 1, 4, 2, 1>(a, tail_tiles, split, s);
  case 3: return launch_lw_tail_t<1, 1, 4, 1, 1>(a, tail_tiles, split, s);
  default: return hipErrorInvalidValue;
  }
}

// whole-layer call on edge tiles; tile and loader waves per tile as launch_f32_lw (1 .. 4). hipErrorInvalidValue: not launched - m or n
// below the tile, n not a multiple of 4, k not in 64-k chunks, no batch
hipError_t launch_f32_lw_edge(int tile, const GemmArgs &a, hipStream_t s) {
  switch (tile) {
  case 1: return launch_lw_edge_t<2, 2, 2, 2>(a, s);
  case 2: return launch_lw_edge_t<2, 1, 4, 2, LW_NSLOT, 1>(a, s);
  case 3: return launch_lw_edge_t<1, 1, 4>(a, s);
  case 4: return launch_lw_edge_t<4, 2, 1, 2, 3>(a, s);
  default: return hipErrorInvalidValue;
  }
}

// whole-layer call with a ragged k; tile and loader waves per tile as launch_f32_lw_edge (1 .. 4). hipErrorInvalidValue: not launched -
// k < 64, k not a multiple of 8, k a multiple of 64, m or n below the tile, n not a multiple of 4, no batch
hipError_t launch_f32_lw_kedge(int tile, const GemmArgs &a, hipStream_t s) {
  switch (tile) {
  case 1: return launch_lw_kedge_t<2, 2, 2, 2>(a, s);
  case 2: return launch_lw_kedge_t<2, 1, 4, 2, LW_NSLOT, 1>(a, s);
  case 3: return launch_lw_kedge_t<1, 1, 4>(a, s);
  case 4: return launch_lw_kedge_t<4, 2, 1, 2, 3>(a, s);
  default: return hipErrorInvalidValue;
  }
}

template <int WM, int WN, int WK, int NL> static hipError_t launch_f32_chain_t(const ChainArgs &a, hipStream_t s) {
  using I = LwChain<WM, WN, WK, NL>;
  ChainArgs args = a;
  args.tiles_m = a.m / I::Tile::BM;
  args.tiles_n = a.n / I::Tile::BN;
  const long long tiles = (long long)args.tiles_m * args.tiles_n;
  if (tiles <= 0 || tiles > 0x7fffffffLL) return hipErrorInvalidValue;
  return lw_launch<I>(dim3((unsigned)tiles), s, args);
}

// tile as in launch_f32_lw: 1 = 64x64 + K2, 2 = 64x32 + K4 (gemm_plan.h f32_chain_tile_dims)
hipError_t launch_f32_chain(int tile, const ChainArgs &a, hipStream_t s) {
  switch (tile) {
  case 1: return launch_f32_chain_t<2, 2, 2, 2>(a, s);
  case 2: return launch_f32_chain_t<2, 1, 4, 1>(a, s);
  default: return hipErrorInvalidValue;
  }
}

// tile: 0 = 64x64 (4 MFMA waves), 1 = 64x64 with K split over 2 wave groups (8 MFMA waves, two per
// SIMD), 2 = 64x32 with K split over 4 (8 MFMA waves), 3 = 32x32 with K split over 4 (4 MFMA waves)
hipError_t launch_f32_lw(int tile, const GemmArgs &a, hipStream_t s) {
  switch (tile) {
  case 0: return launch_lw_t<2, 2, 1>(a, s);
  // two loader waves per panel for the 8-wave tile (C2): the 16 + 16 requests of a chunk - above all of chunk 0, which every MFMA
  // wave waits for - go out in half the time; same-box A/B 18.10 -> 17.97 us. The 64x32 tile (C3) measured 1 % slower with them.
  // (launch_f32_lw_halves above runs the same tiles as two 64x32 + K2 workgroups each, the same bits: C2 17.64 -> 17.19 us same-box;
  // the planner's rule takes it wherever there is a tile per CU, this launch stays for everything else and as the fall-back)
  case 1: return launch_lw_t<2, 2, 2, 2>(a, s); // (four per panel: 18.25 us)
  // 64x32 with K split over FOUR wave groups: 8 MFMA waves = two per SIMD, like the 64x64 k2 tile - one wave's fragment reads and
  // barrier waits hide behind the other's MFMAs. C3 (512 x 1024 x 1024): 10.52 -> 10.21 us same-box against the K2 split (4 waves).
  // Its loader waves: two for the A panel (16 requests per chunk) and one for B (8) - every loader issues 8; C3 9.912 -> 9.881 us
  // against one per panel, four alternating pairs on one box (two each: 9.888; profiles/r04_c3_loaders_and_launch_knobs.txt).
  case 2: return launch_lw_t<2, 1, 4, 2, LW_NSLOT, 1>(a, s);
  // (the same tile with its K split over EIGHT wave groups - two MFMA waves per SIMD, one k-block per wave and chunk, the barrier behind
  // the block - measured 3-4.5 % slower on the reference's batch-256 layers: profiles/r04_c3_loaders_and_launch_knobs.txt (5))
  case 3: return launch_lw_t<1, 1, 4>(a, s);
  // 128x64 for large outputs: 8 MFMA waves (4 x 2 tiles of 32x32), two loader waves per panel, a 3-slot ring (48 KiB per slot)
  case 4: return launch_lw_t<4, 2, 1, 2, 3>(a, s);
  default: return hipErrorInvalidValue;
  }
}

} // namespace tpp
