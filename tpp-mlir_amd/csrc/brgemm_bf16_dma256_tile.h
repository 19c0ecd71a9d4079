// brgemm_bf16_dma256_tile.h - the 256 x 256 bf16 tile, written once: the body of the kernels of brgemm_bf16_dma256.hip (whole tiles) and of
// brgemm_bf16_dma256_edge.hip (EDGE: a ceil-divided grid whose last tile row / column is shifted back, brgemm_bf16_dma256_edge.h) and the layer
// step of the chain kernels of brgemm_bf16_dma256_chain.hip (CHAIN: a chain of whole-layer calls in one launch, xsmm_hip_set_chain_dma256 -
// the body is called once per layer and row block, the seam between two layers is that file's; brgemm_bf16_dma256_chain.h).
//
// The large-shape member of the bf16 BRGEMM family for gfx950:
// 256 x 256 workgroup tiles, four waves of 128 x 128 (4 x 4 accumulator tiles of
// v_mfma_f32_32x32x16_bf16 each), operands streamed global -> LDS by buffer_load ... lds (no
// staging registers).
//
// Why this tile: a CU pulls at most 50-64 B/clk from the L2 into the LDS (TA busy ~650 cycles per 32 KiB),
// and the 128 x 128 kernel needs 32 KiB of fill per 512 MFMA cycles - the fill path alone bounds it at
// ~80 % of the matrix-core rate and in practice it runs at ~50 %. A 256 x 256 workgroup
// tile halves the fill per flop (32 B/clk), and its 128 x 128 wave tiles read half the fragment bytes per
// MFMA ((4+4) fragments per 16 MFMAs instead of (2+2) per 4). Used when the output has about one such
// tile per CU (pick_bf16_tile); smaller outputs keep the 128 x 128 tiles so that every CU has work.
//
// Pipeline (per workgroup, 256 threads, 1 wave per SIMD so each lane may use 512 registers: 256
// accumulators + 2 fragment sets of 32):
//   ring : 4 slots x 32 KiB; a slot = one K chunk of 32: A [256 rows][64 B] | B 16 VNNI pair-rows x
//          [256 columns] dwords. Chunk t+3 is fetched (8 DMA instructions per wave, one every second
//          MFMA) during the second K step of chunk t, into the slot chunk t-1 just left.
//   A    : LDS image [256 rows][4 x 16 B]; 16-byte piece index XOR ((row>>2)&3), applied to the SOURCE
//          address of the DMA and again by the fragment read: ds_read_b128 conflict-free.
//   B    : the VNNI-2 pair-rows as they are; a lane's fragment (8 consecutive k of one column) is 4
//          dwords one pair-row (1 KiB) apart: two ds_read2st64_b32.
//          Opt-in (xsmm_hip_set_dma256_images; entry points brgemm_bf16_dma256_flatb / _vnni4): a FLAT B
//          [k][ldb] - the chunk's 32 rows of 512 B, 64-byte blocks XORed with row & 3 on the DMA's source
//          side, a fragment two ds_read_b64_tr_b16 - and a VNNI-4 B [k/4][ldb][4] - 8 k-group rows of
//          2 KiB as they are, a fragment two ds_read_b64. A B slot is 16 KiB, a wave issues 4 of its 16
//          one-KiB instructions and a fragment set is 12 LDS reads in all three images: one schedule.
//          The maps, written once: brgemm_bf16_dma256_images.h (tests/test_dma256_images.py).
//   sync : per chunk ONE s_waitcnt vmcnt (own DMA of chunk t+1 landed) + ONE raw s_barrier between its
//          two K steps; never __syncthreads inside the loop (it would drain the DMA queue).
//   out  : as the 128 x 128 kernel - operands swapped so a lane owns a row, bias / relu / one RNE
//          rounding (v_cvt_pk_bf16_f32), permlane32 swap, per-wave LDS tile, coalesced 16-byte stores.
#pragma once
#include "gemm_common.h"
#include "xsmm_desc.h"
#include "brgemm_bf16_dma256_images.h"
#include "brgemm_bf16_dma256_edge.h"
#include "chain_args.h"
#include <type_traits>

namespace tpp {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void lds_void_t;

// IMG: the B image (brgemm_bf16_dma256_images.h) - 0 VNNI-2, 2 flat, 4 VNNI-4. Everything but the B side of the DMA and of the fragment
// reads is one text.
// EDGE (brgemm_bf16_dma256_edge.h): m and n need not be multiples of 256 (m, n >= 256, n % 8 == 0). The grid is ceil-divided, the last tile
// row / column starts at m - 256 / n - 256 and the epilogue stores a 16-byte piece only if no other tile owns it. Ring, images, schedule
// and K loop are the same text; false compiles to the kernel without the parameter.
// the lane index from statements the compiler keeps where they stand (see the epilogue's fresh_lane)
__device__ __forceinline__ int d256_fresh_lane() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}

// CHAIN (brgemm_bf16_dma256_chain.hip, xsmm_hip_set_chain_dma256): the body as ONE LAYER STEP of a layer chain - the caller hands in the layer's
// arguments and the step's tile (ctm, ctn) instead of the block index, and calls the body once per step: offsets, wrap deltas, accumulators,
// prologue, K loop and epilogue are all taken anew from p at the top of each call. The A operand of a later layer was stored by other
// workgroups of the same launch: every LDS-DMA load of A carries sc1 (the L1 is bypassed; the aux field is an immediate, so layer 0 pays
// it too). The seam itself - drain, barrier, counter - is the caller's. false compiles to the kernel without the parameter.
template <int IMG, bool EDGE, bool CHAIN = false>
__device__ __forceinline__ void brgemm_bf16_dma256_body(const GemmArgs &p, int ctm = 0, int ctn = 0, int cwave = 0, int cl = 0) {
  static_assert(d256_image_ok(IMG), "0: VNNI-2 B image, 2: flat B image + transpose reads, 4: VNNI-4 B image + 8-byte reads");
  constexpr int BM = D256_BM, BN = D256_BN, BK2 = D256_BK, NSLOT = 4, TM = 4, TN = 4;
  constexpr int A_SLOT = D256_A_SLOT, B_SLOT = D256_B_SLOT, SLOT = A_SLOT + B_SLOT;
  constexpr int DMA_PER_CHUNK = 8; // per wave: 4 x 1 KiB of A + 4 x 1 KiB of B
  static_assert(SLOT == 32768, "ring slot");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_x[];

  // (CHAIN: the lane index is taken anew in every step and the wave index comes from the caller, in a scalar register - a thread index that
  // lives across the K loop for the next step's offsets is a register this kernel does not have)
  const int tid = CHAIN ? cwave * 64 + d256_fresh_lane() : (int)threadIdx.x, lane = tid & 63;
  const int wave = CHAIN ? cwave : __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
  const int tm = CHAIN ? ctm : (int)(blockIdx.x >> 1) * p.tiles_m + (int)blockIdx.z;
  const int tn = CHAIN ? ctn : (int)(blockIdx.x & 1) * p.tiles_n + (int)blockIdx.y;
  const int m0 = EDGE ? d256e_origin(tm, p.m) : tm * BM, n0 = EDGE ? d256e_origin(tn, p.n) : tn * BN; // wave-uniform: from the block index
  const unsigned short *__restrict__ A = (const unsigned short *)p.A;
  const unsigned short *__restrict__ B = (const unsigned short *)p.B;
  unsigned short *__restrict__ C = (unsigned short *)p.C;
  const int kchunks = p.k / BK2;
  const int T = p.br * kchunks;

  // per-lane source offsets of this wave's 8 DMA instructions (constant for the kernel):
  // A instruction v fills rows 16v .. 16v+15 (lane -> row 16v + lane/4, LDS piece lane%4),
  // B instruction v fills pair-row v (lane -> columns 4*lane .. 4*lane+3); flat image: rows 2v, 2v+1, source blocks swizzled;
  // VNNI-4 image: one half of k-group row v/2 (d256_b_dma_voff)
  unsigned voffA[4], voffB[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int v = wave * 4 + u;
    const int row = 16 * v + (lane >> 2), pos = lane & 3;
    voffA[u] = (unsigned)(row * (int)p.lda * 2 + ((pos ^ ((row >> 2) & 3)) << 4));
    voffB[u] = IMG == 0 ? (unsigned)(v * (int)p.ldb * 4 + (lane << 4)) : d256_b_dma_voff(IMG, v, lane, (int)p.ldb);
  }
  const unsigned short *gA = A + (int64_t)m0 * p.lda, *gB = B + d256_b_col_elems(IMG, n0);
  int kc = 0;
  const int64_t dA_wrap = p.stride_a - (int64_t)(kchunks - 1) * BK2;
  const int64_t dB_in = d256_b_chunk_elems(p.ldb), dB_wrap = p.stride_b - (int64_t)(kchunks - 1) * dB_in;
  auto dma_piece = [&](int slot, int u) __attribute__((always_inline)) {
    unsigned char *base = smem_x + slot * SLOT + wave * 4096;
    if (u < 4) {
      const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void *)gA, 0, 0x7fffffff, 0x00020000);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lds_void_t *)(base + u * 1024), 16, voffA[u], 0, 0, CHAIN ? 16 : 0);
    } else {
      const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void *)gB, 0, 0x7fffffff, 0x00020000);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, (lds_void_t *)(base + A_SLOT + (u - 4) * 1024), 16, voffB[u - 4], 0, 0, 0);
    }
  };
#define TPP_DMA256_ADVANCE()    \
  do {                          \
    if (++kc == kchunks) {      \
      kc = 0;                   \
      gA += dA_wrap;            \
      gB += dB_wrap;            \
    } else {                    \
      gA += BK2;                \
      gB += dB_in;              \
    }                           \
  } while (0)

  f32x16 acc[TM][TN];
  bf16x8_t af[2][TM];
  u32x4 bw[2][TN]; // B fragments as dwords: a fragment is filled by two 2-dword reads
  // flat image: the halves of a fragment as the transpose reads deliver them. Those reads are inline assembly, because hipcc puts an
  // s_waitcnt vmcnt(0) in front of a ds_read_b64_tr_b16 it knows of whenever one of this wave's LDS-DMA loads is in flight (it cannot
  // tell the read from one of the bytes the DMA is writing) and so drained the DMA queue 20 times per steady lap. What the compiler does
  // not know of it does not wait for either: flat_wait() below is the wait, written by hand.
  typedef unsigned int u32x2q_t __attribute__((ext_vector_type(2)));
  u32x2q_t bq[2][TN][2];
  // lane bases of the fragment reads (byte offsets inside a slot). One opaque base per column tile so
  // that the four pair-row reads of a fragment pair up as ds_read2st64_b32 (rows r, r+1) straight into
  // consecutive registers instead of being paired across tiles.
  int a_lane[2], b_lane[TN];
  a_lane[0] = (wm * 128 + li) * 64 + ((lh ^ ((li >> 2) & 3)) << 4); // K step 0: pieces lh
  a_lane[1] = a_lane[0] ^ 32;                                       // K step 1: pieces 2 + lh
  asm volatile("" : "+v"(a_lane[0]), "+v"(a_lane[1]));
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    b_lane[j] = A_SLOT + (IMG == 0 ? ((4 * lh) * BN + wn * 128 + j * 32 + li) * 4 : d256_b_frag_lds(IMG, wn, j, 0, lane, 0));
    asm volatile("" : "+v"(b_lane[j]));
  }
  // One of the 12 LDS reads of a fragment set, in the order the MFMAs need them: A0, B0 (two halves),
  // B1, B2, B3, A1, A2, A3. They are issued ONE PER MFMA (a burst of 12 reads from four waves at once
  // fills the LDS queue and stalls the MFMA issue behind it: measured 217 cycles per K step).
  auto frag_piece = [&](int buf, int slot, int ks, int idx) __attribute__((always_inline)) {
    const unsigned char *s = smem_x + slot * SLOT;
    if (idx == 0 || idx >= 9) {
      const int i = idx == 0 ? 0 : idx - 8;
      af[buf][i] = *(const bf16x8_t *)(s + a_lane[ks] + i * (32 * 64));
    } else {
      const int j = (idx - 1) >> 1, h = (idx - 1) & 1;
      if constexpr (IMG == 0) {
        const unsigned int *bp = (const unsigned int *)(s + b_lane[j] + (8 * ks) * BN * 4);
        bw[buf][j][2 * h] = bp[(2 * h) * BN];
        bw[buf][j][2 * h + 1] = bp[(2 * h + 1) * BN];
      } else {
        // four consecutive k of the lane's column per read: the hardware transpose of a [4 k][16 columns] block of the flat image (EXEC is
        // all ones here: every branch around a fragment read is wave-uniform), 8 contiguous bytes of the VNNI-4 image
        typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
        const unsigned char *bp = s + b_lane[j] + D256_KS_STEP * ks + D256_H_STEP * h;
        if constexpr (IMG == 2) {
          const unsigned la = (unsigned)(size_t)(__attribute__((address_space(3))) const unsigned char *)bp;
          asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(bq[buf][j][h]) : "v"(la));
        } else {
          const u32x2_t q = *(const u32x2_t *)bp;
          bw[buf][j][2 * h] = q[0];
          bw[buf][j][2 * h + 1] = q[1];
        }
      }
    }
  };
  // Flat image, in front of the MFMAs of a K step: the eight transpose reads of fragment set `set` have landed. LDS reads return in
  // order and a set is read as A0, B x 8, A1, A2, A3, so at most 3 outstanding means every B read is back (whatever else counts
  // into lgkmcnt only makes the wait longer). The reads' results pass through the statement, so nothing uses them in front of it; the
  // compiler's own counts for the A reads do not know of the transpose reads and are therefore never too lax.
  auto flat_wait = [&](int set) __attribute__((always_inline)) {
    if constexpr (IMG == 2) {
      asm volatile("s_waitcnt lgkmcnt(3)"
                   : "+v"(bq[set][0][0]), "+v"(bq[set][0][1]), "+v"(bq[set][1][0]), "+v"(bq[set][1][1]), "+v"(bq[set][2][0]), "+v"(bq[set][2][1]),
                     "+v"(bq[set][3][0]), "+v"(bq[set][3][1]));
#pragma unroll
      for (int j = 0; j < TN; ++j) bw[set][j] = u32x4{bq[set][j][0][0], bq[set][j][0][1], bq[set][j][1][0], bq[set][j][1][1]};
    }
  };
  auto frag_load = [&](int buf, int slot, int ks) __attribute__((always_inline)) {
#pragma unroll
    for (int idx = 0; idx < 12; ++idx) frag_piece(buf, slot, ks, idx);
  };
  // One chunk in ring slot `slot`. STEADY: chunks t+1..t+3 exist (everything unconditional, slot a
  // literal); otherwise one of the last <= 6 chunks: h1 / h2 / h3 say whether chunks t+1 / t+2 / t+3
  // exist. Two code paths only (the 4-chunk steady body, the run-time tail): all 256 accumulator
  // registers are live across every path, so there is no room for the copies that merging many
  // specialised paths would need.
  auto chunk = [&](auto steady_c, int slot, bool h1, bool h2, bool h3) __attribute__((always_inline)) {
    constexpr bool STEADY = decltype(steady_c)::value;
    // ---- K step 0 (fragments in set 0); set 1 <- K step 1 of this chunk, one read per MFMA
    flat_wait(0);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, bw[0][j]), af[0][i], acc[i][j], 0, 0, 0);
        if (i * TN + j < 12) frag_piece(1, slot, 1, i * TN + j);
        __builtin_amdgcn_sched_barrier(0);
      }
    const bool next = STEADY || h1;
    if (next) {
      // chunk t+1: this wave's DMA has landed (chunk t+2's may still fly), then everybody's
      if (STEADY || h2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(DMA_PER_CHUNK) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      if (!STEADY) { // the last chunks: plain bursts, a branch per MFMA would cost more
        frag_load(0, (slot + 1) & (NSLOT - 1), 0);
        if (h3) {
#pragma unroll
          for (int u = 0; u < 8; ++u) dma_piece((slot + 3) & (NSLOT - 1), u);
          TPP_DMA256_ADVANCE();
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // ---- K step 1 (set 1); set 0 <- K step 0 of chunk t+1; the DMA of chunk t+3 rides along, into
    // the slot chunk t-1 has left
    flat_wait(1);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, bw[1][j]), af[1][i], acc[i][j], 0, 0, 0);
        if (STEADY && i * TN + j < 12) frag_piece(0, (slot + 1) & (NSLOT - 1), 0, i * TN + j);
        if (STEADY && ((i * TN + j) & 1)) {
          dma_piece((slot + 3) & (NSLOT - 1), (i * TN + j) >> 1);
          if (i == TM - 1 && j == TN - 1) TPP_DMA256_ADVANCE();
        }
        __builtin_amdgcn_sched_barrier(0);
      }
  };
  using yes = std::integral_constant<bool, true>;
  using no = std::integral_constant<bool, false>;

  // prologue: chunks 0, 1, 2 in flight at once
#pragma unroll
  for (int c = 0; c < 3; ++c)
    if (T > c) {
#pragma unroll
      for (int u = 0; u < 8; ++u) dma_piece(c, u);
      TPP_DMA256_ADVANCE();
    }
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
  if (T > 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * DMA_PER_CHUNK) : "memory");
  else if (T > 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(DMA_PER_CHUNK) : "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  if (T > 0) frag_load(0, 0, 0);
  int t = 0;
  for (; t + 6 < T; t += 4) { // steady state: ring slots are compile-time constants (t % 4 == 0 here)
    chunk(yes{}, 0, true, true, true);
    chunk(yes{}, 1, true, true, true);
    chunk(yes{}, 2, true, true, true);
    chunk(yes{}, 3, true, true, true);
  }
  for (; t < T; ++t) chunk(no{}, t & (NSLOT - 1), t + 1 < T, t + 2 < T, t + 3 < T); // <= 6 chunks

  // ---- epilogue ------------------------------------------------------------------------
  // lane (li, lh) owns row 32*i + li of wave-tile row block i and, in registers 4g..4g+3 of
  // tile (i, j), columns 32*j + 8*g + 4*lh + (0..3)
  // The lane index is taken again HERE, from statements the compiler keeps where they stand: derived from threadIdx.x up front, the
  // epilogue's lane offsets stayed live across the K loop, whose 256 accumulators + 64 fragment registers leave no room for them - four
  // of them were spilled to scratch memory (20 bytes per lane) in the prologue and reloaded here. Once per part of the epilogue: a
  // value that lives across the beta-1 block, which wants every register for the accumulators, is spilled again.
  auto fresh_lane = []() __attribute__((always_inline)) {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
  };
  typedef unsigned int u32x2d __attribute__((ext_vector_type(2)));
  // What the epilogue takes from the arguments. CHAIN: read HERE, from the layer's entry in the kernarg segment, through a layer index the
  // compiler cannot see through - loaded in front of the K loop these seven scalar registers stay live across it, and that loop with the
  // chain's own state beside it has none to spare (they were spilled). (Without CHAIN every D256_EP is the argument itself, read where
  // the text names it.)
  [[maybe_unused]] unsigned short *cC = nullptr;
  [[maybe_unused]] const void *cD = nullptr;
  [[maybe_unused]] int64_t cldc = 0;
  [[maybe_unused]] int cep = 0;
  if constexpr (CHAIN) {
    int el = cl;
    asm volatile("" : "+s"(el));
    const __attribute__((address_space(4))) ChainArgs &q = *(const __attribute__((address_space(4))) ChainArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    cC = (unsigned short *)q.L[el].C;
    cD = q.L[el].D;
    cldc = q.L[el].ldc;
    cep = q.L[el].ep | EP_BETA0; // (beta 0: the chain launcher's precondition)
  }
#define D256_EP(chain_value, value) (CHAIN ? (chain_value) : (value))
  const __amdgpu_buffer_rsrc_t rsrcC = __builtin_amdgcn_make_buffer_rsrc(
      (void *)(D256_EP(cC, C) + (int64_t)(m0 + wm * 128) * D256_EP(cldc, p.ldc) + n0 + wn * 128), 0, 0x7fffffff, 0x00020000);
  const unsigned ldcb = (unsigned)((int)D256_EP(cldc, p.ldc) * 2);
  if (!(D256_EP(cep, p.ep) & EP_BETA0)) { // beta = 1: add C before the single rounding
    const int lane1 = fresh_lane(), li = lane1 & 31, lh = lane1 >> 5;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const u32x2d c2 = __builtin_amdgcn_raw_buffer_load_b64(
              rsrcC, (unsigned)(32 * i + li) * ldcb + (unsigned)((32 * j + 8 * g + 4 * lh) * 2), 0, 0);
          acc[i][j][4 * g + 0] += __uint_as_float(c2[0] << 16);
          acc[i][j][4 * g + 1] += __uint_as_float(c2[0] & 0xffff0000u);
          acc[i][j][4 * g + 2] += __uint_as_float(c2[1] << 16);
          acc[i][j][4 * g + 3] += __uint_as_float(c2[1] & 0xffff0000u);
        }
  }
  __syncthreads(); // every wave is done with the ring (all DMA landed): reuse it as per-wave output tiles
  { // (a scope of its own: these names shadow the K loop's)
  const int lane = fresh_lane(), li = lane & 31, lh = lane >> 5;
  const bool relu = (D256_EP(cep, p.ep) & EP_RELU) != 0;
  constexpr int ES = 272; // bytes per staged row: 128 bf16 + 16 B pad (conflict-free 16-byte accesses)
  unsigned char *ot = smem_x + wave * (64 * ES);
  // EDGE: what this lane stores (d256e_owns). The tile's first d256e_skip rows / columns are a neighbour's: row_lim is the first of the
  // wave's 128 rows this workgroup owns, less the lane's row inside a group of four; col_own: the lane's 16-byte piece of a row is owned.
  // Taken here, from the block index and the fresh lane index - the K loop has no register to spare.
  int row_lim = 0;
  bool col_own = true;
  if constexpr (EDGE) {
    row_lim = d256e_skip(tm, p.m) - wm * 128 - (lane >> 4);
    col_own = wn * 128 + (lane & 15) * 8 >= d256e_skip(tn, p.n);
  }
#pragma unroll
  for (int ih = 0; ih < 2; ++ih) { // 64 output rows of the wave at a time
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      float bias[4][4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        u32x2d b2 = {0u, 0u};
        if (D256_EP(cep, p.ep) & EP_BIAS)
          b2 = *(const u32x2d *)((const unsigned short *)D256_EP(cD, p.D) + n0 + wn * 128 + 32 * j + 8 * g + 4 * lh);
        bias[g][0] = __uint_as_float(b2[0] << 16);
        bias[g][1] = __uint_as_float(b2[0] & 0xffff0000u);
        bias[g][2] = __uint_as_float(b2[1] << 16);
        bias[g][3] = __uint_as_float(b2[1] & 0xffff0000u);
      }
#pragma unroll
      for (int ii = 0; ii < 2; ++ii) {
        const int i = 2 * ih + ii;
        unsigned int pk[4][2];
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
          for (int h2 = 0; h2 < 2; ++h2) {
            float v0 = acc[i][j][4 * g + 2 * h2] + bias[g][2 * h2];
            float v1 = acc[i][j][4 * g + 2 * h2 + 1] + bias[g][2 * h2 + 1];
            if (relu) { // wave-uniform; max(x, 0) == (x > 0 ? x : 0) incl. NaN -> 0
              v0 = __builtin_fmaxf(v0, 0.0f);
              v1 = __builtin_fmaxf(v1, 0.0f);
            }
            typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
            typedef float f32x2_t __attribute__((ext_vector_type(2)));
            const f32x2_t vv = {v0, v1};
            pk[g][h2] = __builtin_bit_cast(unsigned int, __builtin_convertvector(vv, bf16x2_t)); // v_cvt_pk_bf16_f32 (RNE)
          }
#pragma unroll
        for (int g = 0; g < 4; g += 2) {
          const auto s0 = __builtin_amdgcn_permlane32_swap(pk[g][0], pk[g + 1][0], false, false);
          const auto s1 = __builtin_amdgcn_permlane32_swap(pk[g][1], pk[g + 1][1], false, false);
          const u32x4 out = {s0[0], s1[0], s0[1], s1[1]};
          // lower half-wave: columns 32j + 8g .. +7 ; upper: 32j + 8(g+1) .. +7
          *(u32x4 *)(ot + (32 * ii + li) * ES + (32 * j + 8 * g + 8 * lh) * 2) = out;
        }
      }
    }
    // the same wave reads its 64 x 128 tile back row-contiguously: 16 lanes x 16 B = one 256-byte row
#pragma unroll
    for (int it = 0; it < 16; ++it) {
      const int row = it * 4 + (lane >> 4), ch = lane & 15;
      const u32x4 v = *(const u32x4 *)(ot + row * ES + ch * 16);
      if (!EDGE || (col_own && ih * 64 + it * 4 >= row_lim))
        __builtin_amdgcn_raw_buffer_store_b128(v, rsrcC, (unsigned)(lane >> 4) * ldcb + (unsigned)(ch * 16),
                                               (unsigned)(ih * 64 + it * 4) * ldcb, C_STORE_AUX);
    }
  }
  }
}

#undef TPP_DMA256_ADVANCE
#undef D256_EP

} // namespace tpp
