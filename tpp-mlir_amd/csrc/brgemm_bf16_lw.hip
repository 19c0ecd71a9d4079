// brgemm_bf16_lw.hip - bf16 (VNNI-2 B) batch-reduce GEMM with LOADER WAVES for MID-SIZE outputs, and the same kernel
// as a CHAIN of whole-layer fused BRGEMMs in ONE launch (a rank's share of an MLP: layer l+1 on rows [r, r + BM)
// depends only on layer l's same rows).
//
// Why a new family: the shard shapes of the row-sharded MLP (m = 512 ... 2048 rows x 1024 columns, K = 1024) ran at
// 6-18 % of the bf16 MFMA peak on the existing tiles - the 128x128 LDS-DMA tile leaves 3/4 .. 1/2 of the CUs without
// a workgroup, the 64x64 register-staged tile and the 32x32 fragment-from-global tile pay a ds_write pass / uncoalesced
// fragment loads. Measured in round 2: a CU's L2 -> LDS fill path delivers 34-45 B/clk whatever the
// tile, so the time of such a layer is (panel bytes a CU must pull) / (that rate) + the fixed cost of a launch. The
// tiles here are chosen to put ONE workgroup on EVERY CU (32x64, 64x64, 64x128, 128x128 for 512 / 1024 / 2048 / 4096
// rows of a 1024-wide layer) with every panel byte moved by LDS-DMA from two loader waves through a deep ring.
//
// Structure (as brgemm_f32_lw.hip): WM*WN*WK MFMA waves + 2 loader waves (first two hardware waves: A and B).
//   MFMA waves : ds_read fragments + v_mfma_f32_32x32x16_bf16 + ONE raw s_barrier per 64-k chunk; a wave owns TM x TN
//                accumulator tiles of 32x32; WK = 2 splits the four k-steps of a chunk over two wave groups (partials
//                combined once through LDS) - the 32x64 tile keeps four SIMDs busy that way.
//   loaders    : all LDS-DMA of the workgroup, NSLOT-1 chunks ahead through an NSLOT-slot ring, counted vmcnt.
//   LDS images : A [BM rows][8 x 16 B], 16-byte column XOR ((row>>1)&7) applied to the SOURCE address and again by the
//                ds_read_b128; B = the VNNI-2 pair-rows as they are [32][BN dwords] (brgemm_bf16.hip has the notes).
//   epilogue   : (+C) / bias / relu -> v_cvt_pk_bf16_f32 (RNE, the one rounding) -> v_permlane32_swap to 16-byte
//                pieces -> per-wave LDS tile (its OWN region, the ring keeps streaming) -> coalesced 16-byte stores.
//
// Chain mode (MULTI): grid = one workgroup per output tile, all co-resident (tiles <= CUs, one workgroup per CU by
// LDS), every workgroup computes its tile (tm, tn) of EVERY layer. The seam between layer l and l+1, per row block tm:
//   producer: tile stored WRITE-THROUGH (sc1 16-byte stores), every storing wave drains vmcnt(0), workgroup barrier,
//             one lane adds 1 to cnt[l][tm] (relaxed, agent scope)             [guide: Guideline 16, recipe R1]
//   consumer: the A loader polls cnt[l][tm] (relaxed sc1 load, s_sleep) until all tiles_n producers of this launch
//             have arrived, then streams the A panel with sc1 LDS-DMA loads (L1 bypassed: no acquire fence needed
//             when producer stored sc1 and consumer loads sc1).
//   The B loader does not stop at a seam: the next layer's weight panels are prefetched under the epilogue (when the
//   chunk count of a layer is a multiple of the ring depth, so that ring positions line up).
//   Counters are monotonic: a launch adds exactly tiles_n to each, the host passes target = epoch * tiles_n; nothing
//   is reset (no memset launch in front of the kernel). Every spin is bounded by s_memrealtime: on a timeout the
//   workgroup sets *err and carries on (wrong numbers, never a hung GPU); the host checks *err at its sync points.
//   Results are bit-identical to the same layers launched one by one (same tile, same k order, same rounding).
//
// SEVERAL ROUNDS (GRP = 7, xsmm_hip_set_chain_rounds; step maps in brgemm_bf16_lw_chain_rounds.h): a chain with MORE output tiles than
// compute units on G x tiles_n resident workgroups. Workgroup (g, tn) owns the row blocks tm = g + r * G < tiles_m and walks them
// layer-major - for l: for r: - one STEP (l, r) being the layer body above with tm and m0 = tm * BM taken from the step. Counters,
// targets, the bounded wait and the error word are the chain's: cnt[l][tm] per row block, tiles_n arrivals per launch.
//   Progress: step (l, r) of group g waits only for cnt[l-1][g + r * G], i.e. for step (l-1, r) of the workgroups (g, *). That step lies
//   EARLIER in their own step order (layer-major), and every step a workgroup makes before it waits in turn only for still earlier
//   steps of the same group. All G x tiles_n workgroups are resident, so by induction over the step order no wait is cyclic and each
//   one ends. When a workgroup reaches block r of layer l + 1 its producers finished that block R - 1 steps ago: the poll falls through.
//
// MIXED WIDTHS (GRP = 9, xsmm_hip_set_chain_widths; schedule in brgemm_bf16_lw_chain_widths.h, instances in brgemm_bf16_lw_chain_widths.hip): a
// chain whose layers differ in n on m / BM x max_l(n(l) / BN) workgroups. Workgroup (tm, tn) sits out the layers without a column tile tn.
//   Progress: an active layer l > 0 waits only for cnt[l-1][tm], whose n(l-1) / BN producers are resident and wait in turn only for
//   counters of layer l - 2: by induction over the layers no wait is cyclic. A workgroup's counters need not be its own layers'.
//
// RAGGED MIXED WIDTHS (GRP = 11, xsmm_hip_set_chain_widths_ragged; schedule in brgemm_bf16_lw_chain_wragged.h, instances in
// brgemm_bf16_lw_chain_wragged.hip): GRP = 9's sat-out layers on GRP = 8's layers - any m >= BM, per layer any n(l) >= BN and k(l) >= 64 in
// multiples of 8 - on ceil(m / BM) x max_l ceil(n(l) / BN) workgroups. The column shift is the layer's, cnt[l][tm] receives ceil(n(l) / BN)
// arrivals, the wait is on one or two row blocks, the ring is carried through the active layers; no run-ahead. Progress: as GRP = 9.
#include "gemm_common.h"
#include "xsmm_desc.h"
#include "chain_args.h"
#include "brgemm_bf16_lw_launch.h"
#include "brgemm_bf16_lw_chain_edge.h"
#include "brgemm_bf16_lw_chain_rounds.h"
#include <type_traits>
#include <utility>
#include "brgemm_bf16_lw_chain_ragged.h"

namespace tpp {

typedef __bf16 bf16x8_lw __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) void lds_void_b;
typedef unsigned int u32x2_lw __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) unsigned int g_u32_lw;

constexpr int BLW_BK = 64; // k per chunk
static_assert(BLW_BK == BKEDGE_BK && BLW_MAXL == CH_MAXL, "brgemm_bf16_lw_launch.h counts chunks and layers the same way");
// The kernel's argument block, read where it lies (kernarg segment, constant address space): the layer table is indexed at
// run time, and a by-value / by-reference copy of the struct would be spilled to scratch (640 bytes per lane) for that.
typedef const __attribute__((address_space(4))) ChainArgs chain_kernarg_t;

// s_waitcnt vmcnt(younger * PPL): this wave's DMA of all but the `younger` most recent chunks has landed
template <int PPL> __device__ __forceinline__ void blw_wait_younger(int younger) {
#define BLW_CASE(K)                                                                   \
  case K:                                                                             \
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((K) * PPL > 63 ? 63 : (K) * PPL) : "memory"); \
    break;
  switch (younger) {
    BLW_CASE(0) BLW_CASE(1) BLW_CASE(2) BLW_CASE(3) BLW_CASE(4) BLW_CASE(5) BLW_CASE(6)
  default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
#undef BLW_CASE
}

// One loader wave: LDS-DMA instructions of its panel (IS_A: the A panel [BM rows][64 k], else the B panel [32 pair-rows][BN
// dwords]) for every chunk of every layer, NSLOT - 1 chunks ahead of the MFMA waves, and its side of the barrier schedule:
//   per layer  [S2]  P (chunk 0 published), one mid-chunk barrier per further chunk, and - between layers - R1 (WK > 1) and S1.
// NL loader waves share a panel: wave `part` issues the instructions v = part, part + NL, ... of every chunk.
// In chain mode A loader 0 waits at a seam for the row block's producers (with NLA > 1 the others learn it through S2); the B
// loaders prefetch the next layer's panels across the seam when every layer's chunk count is a multiple of the ring depth.
// The steady-state loop is a literal s_waitcnt + s_barrier + the DMA instructions + ~10 scalar instructions: measured on the
// first version of this function (one general loop with a switch over the wait count, the layer bookkeeping and an argument load
// inside), a 16-chunk layer took 5.7 us with NO loads and NO MFMAs at all - the loader's own instruction stream set the pace.
// GRP (grouped launches): the panel base pointers and the batch count are the ITEM's (it_A / it_B / it_br), not the argument block's
// GRP = 2 (QUADS, round 6): the 128x128 tile over a 2 x 2 block of 64x64 ITEMS (QuadItem, chain_args.h): rows 64 .. 127 of the A panel
// come from the lower item row's block (q_delta = its distance from the upper one, minus the 64 rows the instruction offsets already
// cover), columns 64 .. 127 of the B panel from the right item column's block (q_delta = its distance from the left one): the LDS
// image is the flat 128-wide tile's, only the source addresses of the DMA instructions differ.
template <bool IS_A, int NL, int NLA, int NSLOT_C, int SUP, int BM, int BN, int WK, bool MULTI, int FB = 0, int GRP = 0>
__device__ __forceinline__ void blw_loader(chain_kernarg_t *pp, unsigned char *smem, int lane, int m0, int n0, int tm, int L, int part,
                                           const void *it_A = nullptr, const void *it_B = nullptr, int it_br = 0, unsigned q_delta = 0) {
  static_assert(GRP != BLW_QUADS || (BM == 128 && BN == 128 && NL == 1 && (FB == 0 || FB == 4)), "quads: the 128x128 tile, one loader wave per panel, VNNI-2 / VNNI-4 B");
  static_assert(BlwModeCheck<GRP, MULTI, SUP>::ok, "mode, MULTI and SUP (brgemm_bf16_lw_launch.h)");
  chain_kernarg_t &p = *pp;
  constexpr bool ITEMS = blw_items(GRP); // operands from an item (GRP = 3, edge tiles: the argument block's, as GRP = 0)
  // GRP = 4 (RAGGED k, brgemm_bf16_lw_kedge.h): GRP = 3 + a batch element of ceil(k / 64) chunks, the last one shifted back to start at
  // k - 64: the advance into it is k % 64 (d_last), the batch wrap the element's stride less (k - 64). One k-value is one element of an
  // A row and ldb elements of every B image (a pair-row is 2 k, a VNNI-4 group row 4 k, a flat row 1 k): the shifted start is a whole
  // number of image rows and a multiple of 16 bytes because k % 16 == 0.
  // GRP = 6 (RAGGED k in HALF steps): GRP = 4 to this function - k % 8 == 0 keeps the shifted start 16 bytes into an A row and on a whole
  // pair-row / group row / flat row of B.
  // GRP = 8 (a RAGGED-WIDTH chain, brgemm_bf16_lw_chain_ragged.h): GRP = 5's rows and seam wait, GRP = 3's columns, and per LAYER GRP = 4's
  // chunks - bkedge_chunks(k) per batch element, the last one shifted back; a whole k (k % 64 == 0) is the same walk with an advance of 64
  // into the last chunk. The ring is carried from layer to layer (s0); the B loader does not run ahead across a seam in this mode.
  // GRP = 11 (a RAGGED MIXED-WIDTH chain, brgemm_bf16_lw_chain_wragged.h): GRP = 8 in all of that - rows, seam wait over one or two row blocks,
  // the chunk walk, the carried ring, no run-ahead - with GRP = 9's layers: layer lc has p.L[lc].pad columns, this wave sits out a layer
  // without a column tile tn, and the column shift is the LAYER's (n0 is set at every active layer; it arrives as tn * BN). The target is
  // epoch * ceil(n(lc - 1) / BN). Statements of its own below (WRAG), beside GRP = 9's.
  constexpr bool WRAG = blw_chain_wragged(GRP);
  constexpr bool CRAG = blw_chain_ragged(GRP) || WRAG;
  constexpr bool KEDGE = blw_ragged_k(GRP) || CRAG;
  // GRP = 9 (a MIXED-WIDTH chain, brgemm_bf16_lw_chain_widths.h): GRP = 0's chain in which layer lc has p.L[lc].pad columns: this wave skips
  // a layer without a column tile at n0 - no barrier, no ring slot, s0 stays -, waits for epoch * (n(lc - 1) / BN) arrivals in front of every
  // active layer lc > 0, and the B loaders' run-ahead goes to the workgroup's next ACTIVE layer. The MFMA waves count the same way.
  constexpr bool CWID = blw_chain_widths(GRP);
  // GRP = 5 (a CHAIN on edge ROW tiles, brgemm_bf16_lw_chain_edge.h): the argument block's operands as GRP = 0, m0 of the last row block
  // shifted back by the kernel; the seam wait of a shifted block is for TWO row blocks' producers (below)
  // GRP = 7 (a chain in SEVERAL ROUNDS, brgemm_bf16_lw_chain_rounds.h): `tm` arrives as the workgroup's row GROUP g; the loop below runs
  // over STEPS (layer, round) and takes tm and m0 from the step. The A state is rebuilt per step (the row base moves); the B state per
  // step too (the same layer's panels again, or the next layer's), ahead of the step wherever the run-ahead rule holds.
  constexpr bool ROUNDS = GRP == BLW_CHAIN_ROUNDS;
  // GRP = 10 (a mixed-width chain in COLUMN ROUNDS, brgemm_bf16_lw_chain_wrounds.h): GRP = 9 on p.groups workgroup columns. n0 arrives as the
  // column GROUP's first tile; the loop below runs over STEPS (layer, column tile) as GRP = 7's does over (layer, row block) and takes tn
  // and n0 from the step. Both states are rebuilt per step; the B loaders run ahead into the next step, the A loaders never do (the
  // epilogue's staging tiles lie in the A halves such a run-ahead would fill). The seam wait stands in front of every step.
  constexpr bool WRND = blw_chain_wrounds(GRP);
  [[maybe_unused]] int tn = n0 / BN; // (GRP = 10: the step's column tile)
  constexpr int A_SLOT = BM * 128, SLOT = (BM + BN) * 128;
  // SUP = chunks per barrier (the unit everything below counts in: a "chunk" of this function is SUP 64-k chunks, a "slot" SUP
  // consecutive ring slots). SUP = 2 halves the barrier count and the loader's per-iteration scalar work for the small tiles, whose
  // 16-chunk layers spent 75 % of their time in the barrier / bookkeeping skeleton (timing with loads AND MFMAs switched off).
  constexpr int NSLOT = NSLOT_C / SUP;
  constexpr int PPC = (IS_A ? BM / 8 : BN / 8) / NL; // 1 KiB DMA instructions per 64-k chunk issued by this wave
  constexpr int PPL = SUP * PPC;                     // ... per barrier interval
  [[maybe_unused]] constexpr int RPI = 256 / BN;     // VNNI pair-rows per B instruction
  static_assert(PPC >= 1 && (IS_A ? BM / 8 : BN / 8) % NL == 0 && (!IS_A || NL == 1 || NL % 2 == 0), "panel instructions divide over the loader waves");
  static_assert(NSLOT >= 3 && NSLOT_C % SUP == 0 && (NSLOT - 1) * PPL <= 63, "ring depth / vmcnt is 6 bits");
  bool ahead = false;
  if (MULTI && !IS_A && !CRAG) {
    ahead = true;
    for (int l = 0; l < L; ++l) {
      const int Tl = p.L[l].br * (p.L[l].k / BLW_BK) / SUP;
      if (Tl < NSLOT) ahead = false; // (the run-ahead issues NSLOT - 2 chunks of the next layer during this layer's tail)
    }
  }
  // issue state: the panel base of the next chunk to request (of layer state_layer) and the constants of that layer
  int state_layer = -1, kc = 0, kchunks = 1;
  const unsigned short *g = nullptr;
  int64_t d_in = 0, d_wrap = 0;
  [[maybe_unused]] int64_t d_last = 0;
  unsigned vo0 = 0, vo1 = 0, step = 0;
  bool sc1 = false, flat = false;
#define BLW_LOAD_STATE(l)                                                                                              \
  do {                                                                                                                 \
    state_layer = (l);                                                                                                 \
    kchunks = KEDGE ? bkedge_chunks(p.L[l].k) : p.L[l].k / BLW_BK;                                                     \
    kc = 0;                                                                                                            \
    if (IS_A) {                                                                                                        \
      const int64_t lda_ = (l) == 0 ? p.lda : p.L[(l) > 0 ? (l)-1 : 0].ldc;                                            \
      const unsigned short *A_ = (const unsigned short *)(ITEMS ? it_A : (l) == 0 ? p.A : p.L[(l) > 0 ? (l)-1 : 0].C);  \
      g = A_ + (int64_t)(m0 + 8 * part) * lda_;                                                                        \
      d_in = BLW_BK;                                                                                                   \
      d_wrap = p.L[l].stride_a - (int64_t)(kchunks - 1) * BLW_BK;                                                      \
      /* instruction v covers rows 8v .. 8v+7: lane -> row 8v + lane/8, 16-byte piece lane%8 XOR ((row>>1)&7) = 4(v&1) + lane/16; */ \
      /* this wave's instructions are v = part + NL * i: NL even -> one parity (one swizzle term), NL == 1 -> alternating */ \
      const unsigned rowoff_ = (unsigned)((lane >> 3) * (int)lda_ * 2);                                                \
      vo0 = rowoff_ + (unsigned)(((lane & 7) ^ (4 * (part & 1) + (lane >> 4))) << 4);                                  \
      vo1 = NL == 1 ? rowoff_ + (unsigned)(((lane & 7) ^ (4 + (lane >> 4))) << 4) : vo0;                               \
      step = (unsigned)(NL * 8 * (int)lda_ * 2);                                                                       \
      sc1 = MULTI && (l) > 0; /* written by other workgroups in THIS launch: sc1 loads (L1 bypassed) */              \
    } else if (FB == 2) {                                                                                              \
      /* FLAT B ([k][ldb]), image = the chunk's 64 rows as they are, for the transpose reads of the MFMA waves: instruction v */ \
      /* covers rows (512/BN)*v ..: lane -> row lane / (BN/8), 16-byte piece lane % (BN/8); the 64-byte blocks of a row are */ \
      /* XOR-swizzled with the row (BN = 128: row & 3, BN = 64: (row >> 1) & 1) on the SOURCE side, like the A panel */ \
      constexpr int RPT_ = 512 / BN, PPR_ = BN / 8;                                                                    \
      g = (const unsigned short *)(ITEMS ? it_B : p.L[l].B) + n0 + (int64_t)part * RPT_ * p.L[l].ldb;                  \
      d_in = (int64_t)BLW_BK * p.L[l].ldb;                                                                             \
      d_wrap = p.L[l].stride_b - (int64_t)(kchunks - 1) * d_in;                                                        \
      const int row_ = lane / PPR_, piece_ = lane % PPR_;                                                              \
      const int swz_ = BN == 128 ? (row_ & 3) << 2 : ((row_ >> 1) & 1) << 2;                                           \
      vo0 = vo1 = (unsigned)(row_ * (int)p.L[l].ldb * 2 + ((piece_ ^ swz_) << 4));                                     \
      step = (unsigned)(NL * RPT_ * (int)p.L[l].ldb * 2);                                                              \
    } else if (FB == 4) {                                                                                              \
      /* VNNI-4 B ([k/4][ldb][4]): image = the chunk's 16 k-group rows of BN * 8 bytes as they are; instruction v covers */ \
      /* k-group rows (128/BN)*v ..: lane -> row lane / (BN/2), 16-byte piece lane % (BN/2). A fragment is two 8-byte reads. */ \
      constexpr int RPI4_ = 128 / BN, PPR4_ = BN / 2;                                                                  \
      g = (const unsigned short *)(ITEMS ? it_B : p.L[l].B) + 4 * (int64_t)n0 + (int64_t)part * RPI4_ * 4 * p.L[l].ldb;\
      d_in = (int64_t)BLW_BK * p.L[l].ldb;                                                                             \
      d_wrap = p.L[l].stride_b - (int64_t)(kchunks - 1) * d_in;                                                        \
      vo0 = vo1 = (unsigned)((lane / PPR4_) * (int)p.L[l].ldb * 8 + ((lane % PPR4_) << 4));                            \
      if (GRP == BLW_QUADS) vo0 = vo1 = (unsigned)(((lane & 31) << 4)) + ((lane & 32) ? q_delta : 0u); /* 64 pieces = one k-group row: 32 per item */ \
      step = (unsigned)(NL * RPI4_ * (int)p.L[l].ldb * 8);                                                             \
    } else {                                                                                                           \
      g = (const unsigned short *)(ITEMS ? it_B : p.L[l].B) + 2 * (int64_t)n0 + (int64_t)part * RPI * 2 * p.L[l].ldb;  \
      d_in = (int64_t)(BLW_BK / 2) * 2 * p.L[l].ldb;                                                                   \
      d_wrap = p.L[l].stride_b - (int64_t)(kchunks - 1) * d_in;                                                        \
      /* instruction v covers pair-rows RPI*v ..: lane -> pair-row lane / (BN/4), 16-byte piece lane % (BN/4) */       \
      vo0 = vo1 = (unsigned)((lane / (BN / 4)) * (int)p.L[l].ldb * 4 + ((lane % (BN / 4)) << 4));                      \
      if (GRP == BLW_QUADS) vo0 = vo1 = (unsigned)((lane >> 5) * (int)p.L[l].ldb * 4 + ((lane & 15) << 4)) + ((lane & 16) ? q_delta : 0u); /* 32 pieces = one pair-row: 16 per item */ \
      step = (unsigned)(NL * RPI * (int)p.L[l].ldb * 4);                                                               \
    }                                                                                                                  \
    /* one chunk per batch element (the compiler's 64-k tile invokes over packed blocks): EVERY advance is the wrap - the same   */ \
    /* single add as the flat case, instead of a count-and-branch per chunk in the loader's instruction stream, which sets the */ \
    /* pace of the small tiles (32x32 + K2 grouped at K = 4096: 8.97 -> see profiles/r06_bf16_loader_advance_ab.txt)            */ \
    if (!CRAG && kchunks == 1) d_in = d_wrap; /* (GRP = 8: d_in stays 64 k-values, per_k_ below is taken from it) */    \
    flat = d_wrap == d_in;                                                                                             \
    if constexpr (KEDGE) { /* d_in is  64 k-values in the panel's units: the batch elements never continue each other */ \
      const int64_t per_k_ = d_in / BLW_BK;                                                                            \
      d_last = per_k_ * bkedge_step(p.L[l].k, kchunks - 2);                                                            \
      d_wrap = (IS_A ? p.L[l].stride_a : p.L[l].stride_b) - per_k_ * bkedge_chunk_start(p.L[l].k, kchunks - 1);        \
      flat = false;                                                                                                    \
    }                                                                                                                  \
  } while (0)
  // request the next SUP 64-k chunks of the issue state into ring slot `slot` (SUP consecutive 64-k slots), advance state and slot
#define BLW_ISSUE(slot)                                                                                                \
  do {                                                                                                                 \
    _Pragma("unroll") for (int sub_ = 0; sub_ < SUP; ++sub_) {                                                         \
      unsigned char *base_ = smem + ((slot) * SUP + sub_) * SLOT + (IS_A ? 0 : A_SLOT) + part * 1024;                  \
      const __amdgpu_buffer_rsrc_t r_ = __builtin_amdgcn_make_buffer_rsrc((void *)g, 0, 0x7fffffff, 0x00020000);       \
      if (IS_A && sc1) {                                                                                               \
        _Pragma("unroll") for (int v = 0; v < PPC; ++v)                                                                \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(r_, (lds_void_b *)(base_ + v * NL * 1024), 16, (v & 1) ? vo1 : vo0, v * step, 0, 16); \
      } else {                                                                                                         \
        _Pragma("unroll") for (int v = 0; v < PPC; ++v)                                                                \
            __builtin_amdgcn_raw_ptr_buffer_load_lds(r_, (lds_void_b *)(base_ + v * NL * 1024), 16, (v & 1) ? vo1 : vo0,   \
                                                     v * step + ((GRP == BLW_QUADS && IS_A && v >= 8) ? q_delta : 0u), 0, 0);      \
      }                                                                                                                \
      if (KEDGE) { /* +64 k,  + k % 64 into the element's last chunk, then the batch wrap */                       \
        ++kc;                                                                                                          \
        g += kc == kchunks ? d_wrap : kc + 1 == kchunks ? d_last : d_in;                                               \
        if (kc == kchunks) kc = 0;                                                                                     \
      } else if (flat) { /* the batch elements continue each other (whole-layer dispatches): one 64-bit add */        \
        g += d_in;                                                                                                     \
      } else if (++kc == kchunks) {                                                                                    \
        kc = 0;                                                                                                        \
        g += d_wrap;                                                                                                   \
      } else {                                                                                                         \
        g += d_in;                                                                                                     \
      }                                                                                                                \
    }                                                                                                                  \
    slot = slot + 1 == NSLOT ? 0 : slot + 1;                                                                           \
  } while (0)
  const bool poller = MULTI && IS_A && part == 0;
  int slot = 0, s0 = 0; // next ring slot to fill; slot of the current layer's chunk 0 (the layers follow each other through the ring)
  constexpr int PRIMED = -2; // GRP = 7, a value of state_layer: the run-ahead of the step before loaded THIS step's state
  // (ONE loop: GRP = 7 goes from step to step - tm from the group's first row block to its last, then the next layer -, every other
  // launch from layer to layer)
  for (int lc = 0; lc < L; ROUNDS ? chain_rounds_next(tm, lc, p.groups, p.tiles_m) : WRND ? chain_wrounds_next(tn, lc, p.groups, p.L[lc].pad / BN) : (void)++lc) {
    if constexpr (ROUNDS) m0 = tm * BM;
    if constexpr (CWID) {
      if (!chain_widths_active(n0 / BN, p.L[lc].pad, BN)) continue; // (uniform over the workgroup: n0 and the layer's n)
    }
    if constexpr (WRND) {
      if (!chain_widths_active(tn, p.L[lc].pad, BN)) continue; // (the group sits the layer out: the increment above goes to the next layer)
      n0 = tn * BN;
    }
    if constexpr (WRAG) {
      if (!chain_wragged_active(tn, p.L[lc].pad, BN)) continue; // (uniform over the workgroup; s0 stays)
      n0 = chain_ragged_col0(tn, p.L[lc].pad, BN);              // (this layer's shift: BLW_LOAD_STATE below reads it)
    }
    const int T = (ITEMS ? it_br : p.L[lc].br) * (KEDGE ? bkedge_chunks(p.L[lc].k) : p.L[lc].k / BLW_BK) / SUP; // (a multiple of SUP: the launcher picks SUP = 1 otherwise)
    int pre = NSLOT - 2; // chunks of this layer already requested by the run-ahead of the previous layer's tail
    if constexpr (ROUNDS || WRND) {
      if (state_layer != PRIMED) {
        BLW_LOAD_STATE(lc);
        pre = 0;
        slot = s0;
      }
      state_layer = -1;
    } else if (state_layer != lc) {
      BLW_LOAD_STATE(lc);
      pre = 0;
      slot = s0;
    }
    if (poller && lc > 0) {
      // every producer tile of the rows [m0, m0 + BM) of layer lc-1 has been stored (write-through) and drained: the tiles of the row
      // blocks b_first .. b_last - row block tm itself and, for the shifted last block of a RAGGED-m chain, its upper neighbour as well
      // (each block stores its OWN rows only). Every one of their counters must have reached the target; all the waits share ONE time
      // bound and the one error word.
      const int b_first = GRP == BLW_CHAIN_EDGE || CRAG ? chain_edge_first_block(tm, p.tiles_m, p.m, BM) : tm;
      const int b_last = GRP == BLW_CHAIN_EDGE || CRAG ? chain_edge_last_block(tm, p.tiles_m, p.m, BM) : tm;
      // (GRP = 9: p.target is the epoch, the producers of layer lc - 1 are that layer's column tiles)
      unsigned target = p.target;
      if constexpr (CWID) target = chain_widths_target(p.target, p.L[lc > 0 ? lc - 1 : 0].pad, BN);
      if constexpr (WRND) target = chain_widths_target(p.target, p.L[lc > 0 ? lc - 1 : 0].pad, BN); // (GRP = 10: the same counters)
      if constexpr (WRAG) target = chain_wragged_target(p.target, p.L[lc > 0 ? lc - 1 : 0].pad, BN); // (GRP = 11: ceil-divided column tiles, on every block bw below)
      const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
      for (int bw = b_first; bw <= b_last; ++bw) {
        g_u32_lw *c = (g_u32_lw *)(p.cnt + ((size_t)(lc - 1) * p.tiles_m + bw) * CHAIN_CNT_STRIDE);
        for (;;) {
          const unsigned v = __hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if ((int)(v - target) >= 0) break;
          if (__builtin_amdgcn_s_memrealtime() - t0 > CHAIN_TIMEOUT_TICKS) { // never hang the GPU: flag it and go on
            if (lane == 0) __hip_atomic_store((g_u32_lw *)p.err, 1u + (unsigned)lc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
          }
          __builtin_amdgcn_s_sleep(1);
        }
      }
      asm volatile("" ::: "memory");
    }
    if (MULTI && NLA > 1 && lc > 0) __builtin_amdgcn_s_barrier(); // S2: the polling wave has seen the producers arrive
    // Prologue. (Filling the ring two chunks per barrier - a ramp through the first iterations - was measured: chunk 0 is ready
    // 0.4 us earlier, the 16-chunk loop of the 32x64 tile takes 1.0 us longer: the loader is the pace-maker and the ramp costs it
    // a second ISSUE and a variable wait per iteration. So: one burst, but behind the barrier that publishes chunk 0.)
    const int npro = T < NSLOT - 1 ? T : NSLOT - 1;
    // chunks 0 and 1 first, chunk 0 PUBLISHED as soon as it has landed, the rest of the prologue behind the barrier (the MFMA
    // waves work on chunk 0 while it is issued)
    const int nfirst = npro < 2 ? npro : 2;
    int c = pre;
    for (; c < nfirst; ++c) BLW_ISSUE(slot);
    blw_wait_younger<PPL>((c > nfirst ? c : nfirst) - 1);
    __builtin_amdgcn_s_barrier(); // P: chunk 0 of this layer published
    for (; c < npro; ++c) BLW_ISSUE(slot);
    int t = 0;
    // steady state: chunk t+1 has landed when all but the NSLOT - 3 youngest requests have; the barrier (= the MFMA waves'
    // mid-chunk barrier of chunk t) publishes it and retires the slot of chunk t-1, which takes chunk t + NSLOT - 1
    for (; t + NSLOT - 1 < T; ++t) {
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NSLOT - 3) * PPL) : "memory");
      __builtin_amdgcn_s_barrier();
      BLW_ISSUE(slot);
    }
    // the last NSLOT - 2 barriers of the layer: nothing of THIS layer is left to request. The next step of a multi-round chain: this
    // layer's next row block (the same weight panels again), or the next layer's first
    const bool more_rounds = (ROUNDS && chain_rounds_more(tm, p.groups, p.tiles_m)) || (WRND && chain_wrounds_more(tn, p.groups, p.L[lc].pad / BN));
    if constexpr (WRND) {
      // GRP = 10: the run-ahead loads this workgroup's NEXT STEP - the group's next column tile of this layer, or the first tile of its next
      // active layer (L = none: the else arm's loop). n0 is the next step's from here on: nothing below reads it, the loop's head sets it again.
      const int ntn = more_rounds ? tn + p.groups : chain_wrounds_group(tn, p.groups);
      const int nxt = more_rounds ? lc : chain_widths_next(ntn, lc, L, BN, [&](int l_) { return p.L[l_].pad; });
      if (ahead && nxt < L) {
        n0 = ntn * BN;
        BLW_LOAD_STATE(nxt);
        state_layer = PRIMED;
        for (; t + 1 < T; ++t) {
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NSLOT - 3) * PPL) : "memory");
          __builtin_amdgcn_s_barrier();
          BLW_ISSUE(slot);
        }
      } else {
        for (; t + 1 < T; ++t) {
          blw_wait_younger<PPL>(T - 2 - t);
          __builtin_amdgcn_s_barrier();
        }
      }
    } else if constexpr (CWID) {
      // GRP = 9: the run-ahead loads this workgroup's next ACTIVE layer (L = none: the else arm's loop). A statement of its own, so that
      // the other modes' code below is the text it was.
      const int nxt = chain_widths_next(n0 / BN, lc, L, BN, [&](int l_) { return p.L[l_].pad; });
      if (ahead && nxt < L) {
        BLW_LOAD_STATE(nxt);
        for (; t + 1 < T; ++t) {
          asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NSLOT - 3) * PPL) : "memory");
          __builtin_amdgcn_s_barrier();
          BLW_ISSUE(slot);
        }
      } else {
        for (; t + 1 < T; ++t) {
          blw_wait_younger<PPL>(T - 2 - t);
          __builtin_amdgcn_s_barrier();
        }
      }
    } else if (MULTI && ahead && (lc + 1 < L || more_rounds)) {
      BLW_LOAD_STATE(more_rounds ? lc : lc + 1); // (the slot rotation carries over into the next layer / step)
      if constexpr (ROUNDS) state_layer = PRIMED;
      for (; t + 1 < T; ++t) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NSLOT - 3) * PPL) : "memory");
        __builtin_amdgcn_s_barrier();
        BLW_ISSUE(slot);
      }
    } else {
      for (; t + 1 < T; ++t) {
        blw_wait_younger<PPL>(T - 2 - t);
        __builtin_amdgcn_s_barrier();
      }
    }
    if (lc + 1 == L && !more_rounds) return;
    if constexpr (WK > 1) __builtin_amdgcn_s_barrier(); // R1 (K groups combine)
    __builtin_amdgcn_s_barrier();                        // S1 (tile stored and drained)
    if constexpr (CRAG) s0 = chain_ragged_next_s0(s0, p.L[lc].k, p.L[lc].br, NSLOT); // (the schedule's own function: the MFMA waves count the same way)
    else s0 = (s0 + T) % NSLOT;
  }
#undef BLW_ISSUE
#undef BLW_LOAD_STATE
}

template <int WM, int WN, int WK, int TM, int TN, int NSLOT, int NLA, int NLB, int SUP, bool MULTI, int FLATB = 0, int GRP = 0>
__global__ __launch_bounds__(64 * (WM * WN * WK + NLA + NLB)) void brgemm_bf16_lw(ChainArgs p_by_value) {
  static_assert(BlwModeCheck<GRP, MULTI, SUP>::ok, "mode, MULTI and SUP (brgemm_bf16_lw_launch.h)");
  // operands and batch count from an item (GRP = 1, 2). GRP = 3 (EDGE TILES, a whole layer whose m or n the tile does not divide) has
  // no items: everything from the argument block, as GRP = 0
  constexpr bool ITEMS = blw_items(GRP);
  // GRP = 4 (RAGGED k, xsmm_hip_set_edge_k_bf16): GRP = 3 - with own_row = own_col = 0 a layer the tile divides - whose k is a multiple of
  // 16 but not of 64: the last chunk of every batch element is shifted back to end at k and the MFMA waves skip the k-steps it holds
  // again (brgemm_bf16_lw_kedge.h)
  // GRP = 5 (a CHAIN on edge ROW tiles, xsmm_hip_set_chain_edge): MULTI on ceil(m / BM) x n / BN workgroups - the last row block shifted
  // back to start at m - BM, storing only its own rows (GRP = 3's row predicate; the columns are whole tiles), and waiting at every seam
  // for the two row blocks whose rows it reads (blw_loader, brgemm_bf16_lw_chain_edge.h)
  // GRP = 6 (RAGGED k in HALF steps, xsmm_hip_set_edge_k8_bf16): GRP = 4 in every respect - edge rows and columns, ring, loader advance,
  // laps and pairs of untested bodies - for a k that is a multiple of 8 but not of 16: the overlap of the last chunk ends in the middle
  // of a k-step, and that one step multiplies its upper eight k-values only (chunk_ke below, KE = 2)
  // GRP = 8 (a RAGGED-WIDTH chain, xsmm_hip_set_chain_ragged; brgemm_bf16_lw_chain_ragged.h): MULTI on ceil(m / BM) x ceil(n / BN) workgroups -
  // GRP = 5's rows and seam wait, GRP = 3's columns (the last column tile shifted back to n - BN, stores predicated on own_col, bias read at
  // the shifted n0), and per layer GRP = 6's K loop with the LAYER's skip in half steps: 0 for a whole k (every step WHOLE: what the plain
  // chain multiplies), even for k % 16 == 0, odd for k % 16 == 8 - one instance serves the three k classes. A layer starts at any ring slot.
  // GRP = 11 (a RAGGED MIXED-WIDTH chain, xsmm_hip_set_chain_widths_ragged; brgemm_bf16_lw_chain_wragged.h): GRP = 8 on ceil(m / BM) x
  // max_l ceil(n(l) / BN) workgroups, n(l) = p.L[l].pad, with GRP = 9's sat-out layers. Per LAYER: whether the workgroup is active, its first
  // column n0 and its first own column (the same tile is the shifted last one of one layer and an interior one of the next) - so the bias
  // offset, the output base and the store predicate; s0 moves on active layers only, by the ragged chunk count. p.target is the epoch.
  constexpr bool WRAG = blw_chain_wragged(GRP);
  constexpr bool CRAG = blw_chain_ragged(GRP) || WRAG;
  constexpr bool KEDGE = blw_ragged_k(GRP) || CRAG, ROUNDS = GRP == BLW_CHAIN_ROUNDS;
  // GRP = 9 (a MIXED-WIDTH chain, xsmm_hip_set_chain_widths; brgemm_bf16_lw_chain_widths.h): GRP = 0's chain on m / BM x max_l(n(l) / BN)
  // workgroups, n(l) = p.L[l].pad. Workgroup (tm, tn) computes tile (tm, tn) of the layers with a column tile tn and skips the others - all
  // its waves alike, without a barrier or a ring slot. After every active layer but the chain's last it runs the whole seam (drain, R1, S1,
  // one arrival at cnt[l][tm]), also when no further layer is active for it. p.target is the epoch (blw_loader).
  constexpr bool CWID = blw_chain_widths(GRP);
  // GRP = 10 (a mixed-width chain in COLUMN ROUNDS, xsmm_hip_set_chain_width_rounds; brgemm_bf16_lw_chain_wrounds.h): GRP = 9 on m / BM x p.groups
  // workgroups, fewer columns than the widest layer has column tiles. Workgroup (tm, c) walks the column tiles c, c + groups, .. of every
  // layer that has them, layer-major; every step is GRP = 9's active layer with tn and n0 taken from the step, and runs the whole seam
  // (one arrival at cnt[l][tm]) unless its layer is the chain's last. p.target is the epoch; p.tiles_n stays the widest layer's.
  constexpr bool WRND = blw_chain_wrounds(GRP);
  constexpr bool EDGE_ROWS = blw_edge_rows(GRP), EDGE_COLS = blw_edge_cols(GRP); // (the last tile of a column / row of tiles is shifted back)
  // GRP = 7 (a chain in SEVERAL ROUNDS, xsmm_hip_set_chain_rounds): MULTI on p.groups x tiles_n workgroups, fewer than the output tiles -
  // workgroup (g, tn) walks the row blocks g, g + groups, .. of every layer, layer-major (the file's header; brgemm_bf16_lw_chain_rounds.h).
  // m and n in whole tiles: no edge predicate anywhere.
  static_assert(GRP != BLW_QUADS || (WM == 2 && WN == 2 && WK == 1 && TM == 2 && TN == 2), "quads: every MFMA wave owns one item's 64x64 output");
  chain_kernarg_t *pp = (chain_kernarg_t *)__builtin_amdgcn_kernarg_segment_ptr(); // = &p_by_value (the only explicit argument)
  chain_kernarg_t &p = *pp;
  constexpr int NMW = WM * WN * WK, NOUT = WM * WN; // MFMA waves; waves that own output
  constexpr int BM = 32 * WM * TM, BN = 32 * WN * TN;
  constexpr int KS = 4 / WK, PD = KS / 2;            // k-steps of a chunk per wave; fragment prefetch distance (three steps ahead
                                                     // with the barrier one step earlier measured the same: profiles/r04_bf16_lw_read_interleave.txt)
  constexpr int A_SLOT = BM * 128, B_SLOT = BN * 128, SLOT = A_SLOT + B_SLOT;
  constexpr int ES = 64 * TN + 16;                   // bytes per staged output row (16 B pad: conflict-free 16-byte accesses)
  constexpr int STAGE_W = 32 * ES;                   // one 32-row block of a wave's tile
  // The epilogue's per-wave staging tiles live in the A halves of RETIRED ring slots (the whole LDS belongs to the ring: a fifth
  // slot for the 128x128 tile, a sixth for 64x128). After the last workgroup barrier of a layer only the slots of its last
  // 2 * SUP chunks can still be read by a slower wave; the next layer's A panels are requested after the seam barrier S1 (behind
  // every wave's epilogue), and the B loaders' run-ahead writes B halves only.
  constexpr int WPS = A_SLOT / STAGE_W;              // staging tiles per A half
  constexpr int STAGE_SLOTS = (NOUT + WPS - 1) / WPS;
  static_assert(WPS >= 1 && STAGE_SLOTS + 2 * SUP <= NSLOT, "staging tiles fit into the retired slots");
  constexpr int OFF_RED = NSLOT * SLOT;
  static_assert(WK == 1 || (WK == 2 && TM == 1 && TN == 1), "K split: two groups of single-tile waves");
  static_assert(SUP == 1 || ((SUP == 2 || SUP == 4) && TM * TN <= 2 && NSLOT % SUP == 0 && NSLOT % 2 == 0),
                "several chunks per barrier: the tiles that read a whole chunk of fragments ahead");
  constexpr int NLW = NLA + NLB; // loader waves
  static_assert(FLATB == 0 || FLATB == 2 || FLATB == 4, "0: VNNI-2 B image, 2: flat B image + transpose reads, 4: VNNI-4 B image + 8-byte reads");
  static_assert(FLATB != 4 || BN >= 32, "VNNI-4 image: whole k-group rows per DMA instruction (BN = 32: four rows of 256 bytes)");
  static_assert(FLATB != 2 || BN >= 64, "transpose-read image: 64-byte blocks swizzled inside rows of >= 128 bytes");
  static_assert(BN == 32 || BN == 64 || BN == 128, "B pair-rows per DMA instruction");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_c[];

  const int tid = threadIdx.x, lane = tid & 63;
  // the loader waves are the FIRST hardware waves (waves start in order: the first chunks are requested before the
  // MFMA waves exist); `wave` is the role: MFMA waves 0 .. NMW-1, A loaders NMW .. NMW+NLA-1, then the B loaders
  const int hw_wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wave = hw_wave < NLW ? NMW + hw_wave : hw_wave - NLW;
  // tile of this workgroup. Block b runs on XCD b % 8 (observed, used for speed only) and every XCD's L2 fetches the panels of
  // its workgroups itself: the XCDs form an xm x xn grid over the tile grid (chosen by the launcher to minimise the bytes all
  // eight L2s pull together, xn * |A| + xm * |W|: a 512-row layer on 8 x 1 makes every L2 fetch ALL of W)
  const int b = (int)blockIdx.x;
  int tm, tn;
  // GRP: workgroup b = tile (b % item_subs) of item b / item_subs; the item's operands replace the argument block's (uniform values:
  // read through the scalar unit's view of the list)
  [[maybe_unused]] const void *it_A = nullptr, *it_B = nullptr, *it_D = nullptr;
  [[maybe_unused]] void *it_C = nullptr;
  [[maybe_unused]] int it_br = 0;
  [[maybe_unused]] unsigned q_da = 0, q_db = 0;
  if constexpr (GRP == BLW_QUADS) {
    // QUADS: workgroup b = the b-th 2 x 2 block of items. Panels: the upper-left item's A rows / B columns + the two distances; output
    // and bias: MFMA wave (wm, wn) owns item (wm, wn)'s 64x64 block outright (its own base pointer, the items' ldc)
    typedef const __attribute__((address_space(4))) QuadItem quad_c_t;
    quad_c_t &w = ((quad_c_t *)p.items)[b];
    const int qi = wave < WM * WN * WK ? wave : 0; // (= wm * 2 + wn; the loader waves do not store)
    it_A = w.A;
    it_B = w.B;
    it_C = w.C[qi];
    it_D = w.D[qi & 1];
    it_br = (int)w.br;
    q_da = w.da;
    q_db = w.db;
    tm = tn = 0;
  } else if constexpr (GRP == BLW_ITEMS) {
    // (plain order: workgroup b = the b-th tile of the list. Handing XCD x the x-th EIGHTH of the list - contiguous block rows of the
    // layer - was measured and is WORSE for the reference's shapes, 1024 x 2560 x 1024 15.0 -> 18.1 us: with row-major items and a
    // column count that is a multiple of 8 the plain order already gives every XCD its own eighth of the COLUMNS, i.e. of W, the
    // larger operand; profiles/r06_bf16_grouped_lw.txt)
    // ... but the tiles of ONE item (2 or 4 workgroups that share the item's A rows / B columns) go to ONE XCD: workgroup b runs on XCD
    // b % 8 (observed, used for speed only), so within every run of 8 * subs workgroups XCD x takes the subs tiles of the x-th item
    int u = b;
    {
      const int subs = p.item_subs, total = (int)gridDim.x;
      if (subs > 1 && total % (8 * subs) == 0) {
        const int xcd = b & 7, j = b >> 3;
        u = (j / subs) * (8 * subs) + xcd * subs + (j % subs);
      }
    }
    const int item = u / p.item_subs, sub = u - item * p.item_subs;
    tm = sub / p.tiles_n;
    tn = sub - tm * p.tiles_n;
    // (tried, round 6: up to 64 items INSIDE the argument block, so that a workgroup reads its item from the kernarg segment instead of
    // through the list pointer - one dependent load less in front of its first DMA. Slower: 9.9 against 9.3 us on 128 x 1024 x 4096 as
    // 32 tile invokes - the 3.3 KiB argument block costs more to fetch than the load it saves. The grouped kernel stays ~1.1 us
    // behind the same tile as a whole-layer launch, 9.3 against 8.1 us under rocprofv3.)
    typedef const __attribute__((address_space(4))) WorkItem item_c_t;
    item_c_t &w = ((item_c_t *)p.items)[item];
    it_A = w.A;
    it_B = w.B;
    it_C = w.C;
    it_D = w.D;
    it_br = (int)w.br;
  } else if constexpr (WRND) {
    // (the grid is tiles_m x p.groups: the XCD grid and the linear order count column GROUPS where the other launches count column tiles)
    if (p.xm > 0) {
      const int xn = 8 / p.xm, xcd = b & 7, j = b >> 3;
      const int lm = p.tiles_m / p.xm, ln = p.groups / xn;
      tm = (xcd / xn) * lm + j / ln;
      tn = (xcd % xn) * ln + j % ln;
    } else {
      tm = b / p.groups;
      tn = b - tm * p.groups;
    }
  } else if (p.xm > 0) {
    const int xn = 8 / p.xm, xcd = b & 7, j = b >> 3;
    const int lm = (ROUNDS ? p.groups : p.tiles_m) / p.xm, ln = p.tiles_n / xn; // tiles per XCD (GRP = 7: row groups)
    tm = (xcd / xn) * lm + j / ln;
    tn = (xcd % xn) * ln + j % ln;
  } else {
    tm = b / p.tiles_n;
    tn = b - tm * p.tiles_n;
  }
  // RAGGED n of grouped items (round 6: the reference's --tiles=64,48,64 rows): an item whose n is not a multiple of the tile's width
  // gets ceil(n / BN) column tiles, the LAST one moved left to end at column n - it recomputes the columns it shares with its
  // neighbour (panels in bounds, no masking of loads) and stores only its own (skip_cols: the first columns of its tile are the
  // neighbour's). Everything else: skip_cols = 0.
  // EDGE TILES (GRP = 3, xsmm_hip_set_edge_tiles): the grid is ceil(m / BM) x ceil(n / BN); the last tile of a row / column of tiles is
  // moved up / left to end at row m / column n. Loaders, LDS images and the K loop see m0 and n0 only and stay inside rows [0, m) and
  // columns [0, n); the tile stores the rows >= own_row and the 16-byte pieces at columns >= own_col of its block (TILE-relative: the
  // tiles have several wave columns) - the others are the neighbour's. n0 is a multiple of 8 (the planner asks for n % 8 == 0).
  // (GRP = 7: tm is the workgroup's row GROUP up to here; the step loops below and in blw_loader take tm and m0 from the step)
  int m0 = GRP == BLW_CHAIN_EDGE || CRAG ? chain_edge_row0(tm, p.tiles_m, p.m, BM) : (EDGE_ROWS && (tm + 1) * BM > p.m) ? p.m - BM : tm * BM;
  int n0 = (EDGE_COLS && (tn + 1) * BN > p.n) ? p.n - BN : tn * BN; // (GRP = 10: the column group's first tile; the step loops take n0 from the step)
  [[maybe_unused]] const int skip_cols = tn * BN - n0;
  [[maybe_unused]] const int own_row = tm * BM - m0;
  [[maybe_unused]] int own_col = tn * BN - n0; // (GRP = 11: the layer's, set with n0 at every active layer)
  if constexpr (WRAG) n0 = tn * BN; // (p.n is the widest layer's: no layer's shift. The loaders derive tn from it)
  const int L = MULTI ? p.nlayers : 1;

  if (wave >= NMW) {
    // ---- loader waves (blw_loader above) ---------------------------------------------------------------------------
    if (wave < NMW + NLA) blw_loader<true, NLA, NLA, NSLOT, SUP, BM, BN, WK, MULTI, 0, GRP>(pp, smem_c, lane, m0, n0, tm, L, wave - NMW, it_A, it_B, it_br, q_da);
    else blw_loader<false, NLB, NLA, NSLOT, SUP, BM, BN, WK, MULTI, FLATB, GRP>(pp, smem_c, lane, m0, n0, tm, L, wave - NMW - NLA, it_A, it_B, it_br, q_db);
    return; // ended waves do not take part in later barriers
  }

  // ---- MFMA waves ------------------------------------------------------------------------------------------------
  const int wk = wave / NOUT, wmn = wave % NOUT, wm = wmn / WN, wn = wmn % WN;
  const int li = lane & 31, lh = lane >> 5;
  f32x16 acc[TM][TN];
  // Fragment buffers. Tiles with one or two accumulators per wave (TM * TN <= 2) keep TWO chunks of fragments: a k-step is only
  // 1-2 MFMAs (32-64 cycles), less than an LDS read takes to come back, so the fragments of chunk t+1 are all read during the
  // second half of chunk t (measured on the 64x64 tile with a two-step lookahead: 420 cycles per chunk for 128 cycles of MFMA).
  // The 128x128 tile (four accumulators, 128 cycles per k-step) reads two k-steps ahead out of one set.
  constexpr bool FULLPF = TM * TN <= 2;
  constexpr int BLW_RD = 3; // SUP = 2: k-steps the fragment reads run ahead of their MFMA
  constexpr int NFB = FULLPF ? 2 * KS : KS;
  static_assert(!FULLPF || NSLOT % 2 == 0, "chunk parity from the ring slot");
  static_assert(SUP == 1 || FULLPF, "two chunks per barrier: the tiles with two fragment sets");
  bf16x8_lw af[NFB][TM];
  u32x4 bw[NFB][TN]; // B fragments as dwords
  int b_lane[TN];   // dword index of this lane's column of tile j in pair-row 4*lh of a k-step
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    b_lane[j] = (4 * lh) * BN + (wn * TN + j) * 32 + li;
    if constexpr (FLATB == 2) {
      // flat image [64 k][BN] (blw_loader FB = 2), fragments by ds_read_b64_tr_b16: in every 16 lanes, lane p names the 8-byte
      // piece (row p / 4, columns 4 (p % 4) ..) of a [4 k][16 n] block and receives COLUMN p of it - four consecutive k of
      // its own column (tools/ubench/tr16_probe.hip pins that). Byte offset of this lane's piece for k = 8 lh + p / 4:
      const int pp16 = lane & 15, blk = wn * TN + j, rowl = pp16 >> 2;
      const int swz = BN == 128 ? rowl : (rowl >> 1) & 1;
      b_lane[j] = (8 * lh + rowl) * (BN * 2) + ((blk ^ swz) << 6) + ((lane >> 4) & 1) * 32 + (pp16 & 3) * 8;
    }
    if constexpr (FLATB == 4) {
      // VNNI-4 image [16 k-groups][BN][4] (blw_loader FB = 4): this lane's column, k-group 2 lh of a k-step (bytes)
      b_lane[j] = (2 * lh) * (BN * 8) + ((wn * TN + j) * 32 + li) * 8;
    }
    asm volatile("" : "+v"(b_lane[j])); // one base VGPR per column tile: rows r, r+1 pair up as ds_read2(st64)_b32
  }
  auto frag_load = [&](int buf, int slot, int ks) __attribute__((always_inline)) {
    const unsigned char *as = smem_c + slot * SLOT;
    const unsigned int *bs = (const unsigned int *)(as + A_SLOT);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int row = (wm * TM + i) * 32 + li;
      af[buf][i] = *(const bf16x8_lw *)(as + row * 128 + (((2 * ks + lh) ^ ((row >> 1) & 7)) << 4));
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      if constexpr (FLATB == 2) {
        typedef short s16x4_lw __attribute__((ext_vector_type(4)));
        typedef __attribute__((address_space(3))) s16x4_lw lds_s16x4_lw;
        typedef __attribute__((address_space(3))) unsigned char lds_u8_lw;
        lds_u8_lw *bb = (lds_u8_lw *)(as + A_SLOT) + b_lane[j] + (16 * ks) * (BN * 2);
        const u32x2_lw q0 = __builtin_bit_cast(u32x2_lw, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_lw *)bb));
        const u32x2_lw q1 = __builtin_bit_cast(u32x2_lw, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_lw *)(bb + 4 * (BN * 2))));
        bw[buf][j] = u32x4{q0[0], q0[1], q1[0], q1[1]};
      } else if constexpr (FLATB == 4) {
        // four consecutive k of a column are 8 contiguous bytes: k-groups 4 ks + 2 lh and + 1 = the lane's eight k of this step
        const unsigned char *bb = as + A_SLOT + b_lane[j] + (4 * ks) * (BN * 8);
        const u32x2_lw q0 = *(const u32x2_lw *)bb, q1 = *(const u32x2_lw *)(bb + BN * 8);
        bw[buf][j] = u32x4{q0[0], q0[1], q1[0], q1[1]};
      } else {
        const unsigned int *bp = bs + b_lane[j] + (8 * ks) * BN;
#pragma unroll
        for (int r = 0; r < 4; ++r) bw[buf][j][r] = bp[r * BN];
      }
    }
  };
  // One chunk in ring slot `slot` (a run-time value: ONE body - two for the tiles that alternate fragment sets - instead of one per
  // ring slot entered through a switch; the slot's LDS offset costs TM + TN vector adds per k-step. The per-slot bodies with their
  // exit after every chunk made hipcc rename the accumulators from body to body - v_mfma D != C - in the chain and flat-B
  // instances, which then spilled 150 .. 1500 bytes per lane). Step q multiplies fragment buffer q while the fragments of step
  // q + PD are read (the last PD steps read the first steps of chunk t+1, published by the mid-chunk barrier; after the last chunk
  // of a layer they read a slot nobody uses - the values are dropped).
  // t, T: this chunk's index and the layer's chunk count. The workgroup barrier sits in the middle of every SUP-th chunk (slot a
  // multiple of SUP: layers start at such a slot) when another barrier interval follows: it publishes the next SUP chunks and
  // retires the previous SUP slots. (With SUP = 2 the fragments of the odd chunk are read during the even chunk's second half - the
  // same interval, already published - and those of the next even chunk during the odd chunk's, behind the barrier.)
  // PAR (tiles with two fragment sets): parity of the slot = which set holds this chunk's fragments.
  // HN: does this chunk carry the barrier? 1 yes / 0 no as compile-time facts (the steady-state loop bodies are then single basic
  // blocks: a conditional barrier - or the loop's exit test - in the middle of a body is a block boundary at which the compiler
  // waits for every LDS read in flight), 2 = decided at run time (the odd first chunk).
  // KE (GRP = 4): 1 = this chunk may be a batch element's LAST one, shifted back: its first `skip` k-steps hold again what the chunk
  // before it multiplied, and step s of the chunk runs only if bkedge_step_runs(s, skip) - a wave-uniform scalar test around the
  // step's MFMAs alone: the fragment reads stay (the slot holds valid data) and so does the barrier. 0 = no test, the body as it was.
  // KE = 2 (GRP = 6, HALF steps): `skip` counts half steps (8 k-values) and is odd on a last chunk; the test is three-way
  // (bkedge8_step_part): not run, whole, or - the ONE step the overlap ends in the middle of - its upper eight k-values only. Lanes
  // 0 .. 31 (lh = 0) hold k-values 0 .. 7 of a step in the A fragment and in all three B images' fragments (frag_load: A piece 2 ks + lh,
  // pair-row 4 lh, flat row 8 lh, k-group 2 lh), so that step's MFMAs get operands that a select has zeroed in those lanes, on BOTH sides:
  // zeroing one alone would turn an Inf in the other into NaN. The half then adds +0.0 products: the accumulators start at +0.0, a sum
  // that started at +0.0 is never -0.0 under round-to-nearest, and adding +0.0 is exact - the result has the bits of a skip. An Inf or
  // NaN in the re-read region counts once, as data. The registers the fragment reads filled are not touched (step q + PD reads on).
  auto chunk_ke = [&](auto par_c, auto hn_c, int slot, int t, int T, auto ke_c, [[maybe_unused]] int skip) __attribute__((always_inline)) {
    constexpr int PAR = decltype(par_c)::value, HN = decltype(hn_c)::value, KE = decltype(ke_c)::value;
    const int ns = slot + 1 == NSLOT ? 0 : slot + 1;
    const bool has_next = HN == 2 ? (SUP == 1 || PAR == 0) && t + SUP < T : HN == 1;
    constexpr int CUR = FULLPF ? PAR * KS : 0, NXT = FULLPF ? (PAR ^ 1) * KS : 0; // fragment sets of chunk t / t+1
#pragma unroll
    for (int q = 0; q < KS; ++q) {
      if constexpr (FULLPF && SUP == 2) {
        // two chunks per barrier: everything up to the end of chunk t+1 was published before chunk t began (the odd chunk with
        // its pair, the next even one by the barrier in the middle of the even chunk before it) and the step after the barrier
        // may read one chunk further. So the fragments are read ONE k-step per step, BLW_RD steps ahead of their MFMA, through
        // the 2 * KS buffers as a ring: the LDS pipe works all the time instead of in the second halves of the chunks, and the
        // wait in front of an MFMA is for reads issued three MFMAs earlier (3 * BLW_RD + 3 reads in flight: lgkmcnt has 4 bits).
        const int tg = q + BLW_RD, ch = tg / KS;
        const int nns = ns + 1 == NSLOT ? 0 : ns + 1;
        frag_load((PAR * KS + tg) % NFB, ch == 0 ? slot : ch == 1 ? ns : nns, wk * KS + tg % KS);
      } else if constexpr (FULLPF) {
        // second half of the chunk (chunk t+1 is published): two of its k-steps per step
        if (q >= KS / 2) {
          const int r = 2 * (q - KS / 2);
          frag_load(NXT + r, ns, wk * KS + r);
          if (r + 1 < KS) frag_load(NXT + r + 1, ns, wk * KS + r + 1);
        }
      } else {
        if (q + PD < KS) frag_load(q + PD, slot, wk * KS + q + PD);
        else frag_load(q + PD - KS, ns, wk * KS + q + PD - KS);
      }
      // The step's fragment reads (for MFMAs two steps / half a chunk ahead) are dealt BETWEEN the step's MFMAs, not in front of them:
      // a 32x32x16 bf16 MFMA holds the matrix pipe for 32 cycles, six DS instructions take the wave longer than that to issue - in
      // front of the MFMAs the pipe ran dry once per k-step (same-box A/B, profiles/r04_bf16_lw_read_interleave.txt: the 4096-row
      // layer 10.02 -> 9.45 us, its chain 30.5 -> 29.4, C5 17.6 -> 17.0, 4096^3 on this tile 128.2 -> 122.3).
      // Interleaved: the four-accumulator tile (128x128) and 64x128; the others read in front of the MFMAs.
      constexpr bool IL = !FULLPF || (SUP == 1 && TM * TN >= 2);
      if constexpr (!IL) __builtin_amdgcn_sched_barrier(0);
      if constexpr (KE == 2) {
        const int part = bkedge8_step_part(wk * KS + q, skip);
        if (part != BKEDGE8_NONE) {
          const bool zero = part == BKEDGE8_UPPER && lh == 0;
          const u32x4 z4 = {0u, 0u, 0u, 0u};
          u32x4 a_[TM], b_[TN];
#pragma unroll
          for (int i = 0; i < TM; ++i) a_[i] = zero ? z4 : __builtin_bit_cast(u32x4, af[CUR + q][i]);
#pragma unroll
          for (int j = 0; j < TN; ++j) b_[j] = zero ? z4 : bw[CUR + q][j];
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_lw, b_[j]), __builtin_bit_cast(bf16x8_lw, a_[i]), acc[i][j], 0, 0, 0);
        }
      } else if constexpr (KE != 0) {
        if (bkedge_step_runs(wk * KS + q, skip)) {
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_lw, bw[CUR + q][j]), af[CUR + q][i], acc[i][j], 0, 0, 0);
        }
      } else {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_lw, bw[CUR + q][j]), af[CUR + q][i], acc[i][j], 0, 0, 0);
      }
      if constexpr (KE != 0) {
        // (a tested step: its MFMAs sit in a block of their own, nothing to interleave them with)
      } else if constexpr (IL && !FULLPF) {
        constexpr int NRD = TM + (FLATB == 4 ? TN : 2 * TN); // DS read instructions of a step (VNNI-4: one ds_read2_b64 per column tile)
        constexpr int PER = (NRD + TM * TN - 2) / (TM * TN - 1);
#pragma unroll
        for (int g_ = 0; g_ < TM * TN - 1; ++g_) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // one MFMA
          __builtin_amdgcn_sched_group_barrier(0x100, PER, 0); // then a share of the DS reads
        }
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      } else if constexpr (IL) {
        // two fragment sets (64x128): the second half of a chunk reads TWO k-steps of the next chunk per step, behind every MFMA a share
        constexpr int NRD = 2 * (TM + (FLATB == 4 ? TN : 2 * TN)), PER = (NRD + TM * TN - 1) / (TM * TN);
#pragma unroll
        for (int g_ = 0; g_ < TM * TN; ++g_) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, PER, 0);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      if (q == KS / 2 - 1 && has_next) {
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
      }
    }
  };
  using P0 = std::integral_constant<int, 0>;
  using P1 = std::integral_constant<int, 1>;
  auto chunk = [&](auto par_c, auto hn_c, int slot, int t, int T) __attribute__((always_inline)) { chunk_ke(par_c, hn_c, slot, t, T, P0{}, 0); };

  int s0 = 0; // ring slot of the current layer's chunk 0
  // (ONE loop: GRP = 7 goes from step to step - tm from the group's first row block to its last, then the next layer -, every other
  // launch from layer to layer; blw_loader counts the same way)
  for (int l = 0; l < L; ROUNDS ? chain_rounds_next(tm, l, p.groups, p.tiles_m) : WRND ? chain_wrounds_next(tn, l, p.groups, p.L[l].pad / BN) : (void)++l) {
    if constexpr (ROUNDS) m0 = tm * BM;
    if constexpr (CWID) {
      if (!chain_widths_active(tn, p.L[l].pad, BN)) continue; // (the loaders skip the same layers: n0 = tn * BN)
    }
    if constexpr (WRND) {
      if (!chain_widths_active(tn, p.L[l].pad, BN)) continue; // (the group sits the layer out; blw_loader walks the same steps)
      n0 = tn * BN;
    }
    if constexpr (WRAG) {
      if (!chain_wragged_active(tn, p.L[l].pad, BN)) continue; // (the loaders skip the same layers; s0 stays)
      n0 = chain_ragged_col0(tn, p.L[l].pad, BN);               // this layer's shift: bias offset, output base ..
      own_col = chain_ragged_own_col(tn, p.L[l].pad, BN);       // .. and the 16-byte pieces the tile stores
    }
    const auto &Y = p.L[l];
    const int T = (ITEMS ? it_br : Y.br) * (KEDGE ? bkedge_chunks(Y.k) : Y.k / BLW_BK);
    const int ep = Y.ep;
    unsigned short *__restrict__ C = (unsigned short *)(ITEMS ? it_C : Y.C);
    const unsigned ldcb = (unsigned)((int)Y.ldc * 2);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    // bias: fetched here (8 bytes = 4 columns per register quad), used in the epilogue - its latency hides under the K loop
    u32x2_lw biasw[TN][4];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        biasw[j][g] = u32x2_lw{0u, 0u};
        if (ep & EP_BIAS) biasw[j][g] = *(const u32x2_lw *)((const unsigned short *)(ITEMS ? it_D : Y.D) + n0 + ((GRP == BLW_QUADS ? 0 : wn * TN) + j) * 32 + 8 * g + 4 * lh);
      }
    if (MULTI && NLA > 1 && l > 0) __builtin_amdgcn_s_barrier(); // S2 (the loaders' rendezvous after the seam wait)
    __builtin_amdgcn_s_barrier(); // P: chunk 0 published
    __builtin_amdgcn_sched_barrier(0);
    // (T >= 1: the launchers send empty batches to the generic kernel - a branch around this loop costs the 128-wide tiles
    // a second copy of the accumulators and 250 spilled registers)
    // the layers follow each other through the ring: this one starts at slot s0 (the loaders count the same way)
    const int last_slot = (s0 + T - 1) % NSLOT;
    if constexpr (FULLPF && SUP == 2) { // (s0 even; the first barrier interval = chunks 0 and 1 is published)
#pragma unroll
      for (int s = 0; s < BLW_RD; ++s) frag_load(s, s0 + s / KS, wk * KS + s % KS);
    } else if (!FULLPF || !(s0 & 1)) {
#pragma unroll
      for (int s = 0; s < (FULLPF ? KS : PD); ++s) frag_load(s, s0, wk * KS + s);
    } else { // (chunk parity = slot parity selects the fragment set)
#pragma unroll
      for (int s = 0; s < KS; ++s) frag_load(FULLPF ? KS + s : s, s0, wk * KS + s);
    }
    {
      int t = 0, slot = s0;
      auto next = [&](int x) __attribute__((always_inline)) { return x + 1 == NSLOT ? 0 : x + 1; };
      using Y = std::integral_constant<int, 1>;
      using N = std::integral_constant<int, 0>;
      using R = std::integral_constant<int, 2>;
      if constexpr (KEDGE) {
        // RAGGED k (one layer: s0 = 0, SUP = 1). kc: this chunk's index in its batch element; chunk kchunks - 1 is the element's last
        // and skips skipl k-steps. Laps of the ring / pairs of chunks that hold no last chunk run the untested bodies of the plain
        // kernel - single basic blocks -, the others and the layer's tail ask per step.
        // GRP = 6: skipl counts HALF steps and the tested bodies are the three-way ones (KE = 2); the loops are the same.
        // (GRP = 8: the chunks up to the next TESTED one - a whole-k layer has none, chain_ragged_test_period)
        const int kchunks = CRAG ? chain_ragged_test_period(p.L[l].k, T) : bkedge_chunks(p.L[l].k);
        // GRP = 8: a layer of a chain - kchunks and skipl are THIS layer's (skipl in half steps, 0 for a whole k), and slot starts at s0, any
        // slot: the lap loop below begins only at slot 0 and the chunk-by-chunk loop walks there; the tiles with two fragment sets first
        // run an odd first chunk on set 1, as the plain chain does.
        const int skipl = CRAG ? chain_ragged_layer_skip(p.L[l].k)
                          : blw_half_steps(GRP) ? bkedge8_skip_halves(p.L[l].k, kchunks - 1) : bkedge_skip_steps(p.L[l].k, kchunks - 1);
        using KE_T = std::integral_constant<int, blw_half_steps(GRP) || CRAG ? 2 : 1>; // KE of the tested bodies
        int kc = 0;
        auto skip_next = [&]() __attribute__((always_inline)) {
          const bool last = kc + 1 == kchunks;
          kc = last ? 0 : kc + 1;
          return last ? skipl : 0;
        };
        if constexpr (!FULLPF) {
          // A lap of literal slots - the plain kernel's four untested bodies, one basic block - starts at slot 0 when none of its NSLOT
          // chunks is a last one; everything else goes chunk by chunk through ONE tested body with a run-time slot. Both in loops of
          // their own: as the two arms of one loop's body hipcc keeps two sets of accumulators and copies between them (the tile then
          // spills). LAPS: the VNNI-2 image only - with the flat and VNNI-4 images' fragment reads the nest still spills 32 / 48 bytes
          // per lane, so those walk every chunk through the tested body (157 VGPRs).
          constexpr bool LAPS = (NSLOT == 4 || NSLOT == 5) && FLATB == 0;
          while (t + 1 < T) {
            if constexpr (LAPS) {
              while (slot == 0 && t + NSLOT < T && kc + NSLOT < kchunks) {
#pragma unroll
                for (int s_ = 0; s_ < NSLOT; ++s_) chunk(P0{}, Y{}, s_, t + s_, T);
                t += NSLOT;
                kc += NSLOT;
              }
            }
            while (t + 1 < T && !(LAPS && slot == 0 && t + NSLOT < T && kc + NSLOT < kchunks)) {
              chunk_ke(P0{}, Y{}, slot, t, T, KE_T{}, skip_next());
              slot = next(slot);
              ++t;
            }
          }
          chunk_ke(P0{}, N{}, slot, t, T, KE_T{}, skip_next());
        } else {
          if constexpr (CRAG) {
            // (an odd first slot: after a layer with an odd chunk count. With this body the 64x128 tile's VNNI-2 instance spills 76 bytes
            // per lane - it is at 256 VGPRs as a plain chain already - and is left out of the mode's table, brgemm_bf16_lw_launch.h)
            if (slot & 1) {
              chunk_ke(P1{}, R{}, slot, t, T, KE_T{}, skip_next());
              slot = next(slot);
              ++t;
            }
          }
          while (t + 2 < T) {
            // (a loop of its own for the untested pairs: as the other arm of one loop's body they cost a copy of the accumulators per pair)
            while (t + 2 < T && kc + 2 < kchunks) {
              chunk(P0{}, Y{}, slot, t, T);
              slot = next(slot);
              chunk(P1{}, Y{}, slot, t + 1, T);
              slot = next(slot);
              t += 2;
              kc += 2;
            }
            if (t + 2 < T) {
              chunk_ke(P0{}, Y{}, slot, t, T, KE_T{}, skip_next());
              slot = next(slot);
              chunk_ke(P1{}, Y{}, slot, t + 1, T, KE_T{}, skip_next());
              slot = next(slot);
              t += 2;
            }
          }
          if (t + 1 < T) {
            chunk_ke(P0{}, Y{}, slot, t, T, KE_T{}, skip_next());
            chunk_ke(P1{}, N{}, next(slot), t + 1, T, KE_T{}, skip_next());
          } else if (t < T) {
            chunk_ke(P0{}, N{}, slot, t, T, KE_T{}, skip_next());
          }
        }
      } else if constexpr (!FULLPF) { // (SUP = 1) every chunk but the last carries the barrier; T >= 1
        if constexpr (NSLOT == 4 || NSLOT == 5) {
          // whole laps of the ring with LITERAL slots (LDS offsets are immediates: no address adds, and the four bodies of a lap
          // are one basic block): 4096^3 on the 128x128 tile 139 -> 131 us, 2048^3 on a flat B 20.6 -> 19.05, the 4096-row chain
          // 34 -> 33 us (same-box A/B). A single layer starts
          // at slot 0; a layer of a chain first walks to slot 0.
          if constexpr (MULTI) {
            for (; slot != 0 && t + 1 < T; ++t) {
              chunk(P0{}, Y{}, slot, t, T);
              slot = next(slot);
            }
          }
          for (; t + NSLOT < T; t += NSLOT) {
#pragma unroll
            for (int s_ = 0; s_ < NSLOT; ++s_) chunk(P0{}, Y{}, s_, t + s_, T);
          }
        }
        for (; t + 1 < T; ++t) {
          chunk(P0{}, Y{}, slot, t, T);
          slot = next(slot);
        }
        chunk(P0{}, N{}, slot, t, T);
      } else if constexpr (SUP == 2) { // (T even, s0 even) the barrier sits in the even chunk of every pair but the last
        for (; t + 2 < T; t += 2) {
          chunk(P0{}, Y{}, slot, t, T);
          slot = next(slot);
          chunk(P1{}, N{}, slot, t + 1, T);
          slot = next(slot);
        }
        chunk(P0{}, N{}, slot, t, T);
        chunk(P1{}, N{}, next(slot), t + 1, T);
      } else {
        if (slot & 1) { // (an odd first slot: after a layer with an odd chunk count)
          chunk(P1{}, R{}, slot, t, T);
          slot = next(slot);
          ++t;
        }
        for (; t + 2 < T; t += 2) {
          chunk(P0{}, Y{}, slot, t, T);
          slot = next(slot);
          chunk(P1{}, Y{}, slot, t + 1, T);
          slot = next(slot);
        }
        if (t + 1 < T) {
          chunk(P0{}, Y{}, slot, t, T);
          chunk(P1{}, N{}, next(slot), t + 1, T);
        } else if (t < T) {
          chunk(P0{}, N{}, slot, t, T);
        }
      }
    }
    if constexpr (CRAG) s0 = chain_ragged_next_s0(s0, p.L[l].k, p.L[l].br, NSLOT);
    else s0 = (s0 + T) % NSLOT;
    // the fragments prefetched past the end of the layer are dead: without this the compiler sinks their reads
#pragma unroll
    for (int s = 0; s < (FULLPF ? NFB : PD); ++s) {
#pragma unroll
      for (int i = 0; i < TM; ++i) asm volatile("" : "+v"(af[s][i]));
#pragma unroll
      for (int j = 0; j < TN; ++j) asm volatile("" : "+v"(bw[s][j]));
    }

    // ---- epilogue ------------------------------------------------------------------------------------------------
    if constexpr (WK > 1) {
      // K group 1 parks its 32x32 partial, group 0 adds it (group order: 0 + 1) and finishes the tile
      float *red = (float *)(smem_c + OFF_RED) + wmn * 1024 + lane;
      if (wk == 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) red[r * 64] = acc[0][0][r];
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier(); // R1
      if (wk == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][0][r] += red[r * 64];
      }
    }
    if (WK == 1 || wk == 0) {
      // lane (li, lh) owns row 32*i + li of the wave's row block i and, in registers 4g..4g+3 of tile (i, j),
      // columns 32*j + 8*g + 4*lh + (0..3)
      const __amdgpu_buffer_rsrc_t rsrcC = __builtin_amdgcn_make_buffer_rsrc(
          (void *)(GRP == BLW_QUADS ? C : C + (int64_t)(m0 + wm * 32 * TM) * Y.ldc + n0 + wn * 32 * TN), 0, 0x7fffffff, 0x00020000);
      if constexpr (!MULTI) {
        if (!(ep & EP_BETA0)) { // beta = 1: add C before the single rounding (8-byte loads, rare path)
#pragma unroll
          for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
              for (int g = 0; g < 4; ++g) {
                const u32x2_lw c2 = __builtin_amdgcn_raw_buffer_load_b64(
                    rsrcC, (unsigned)(32 * i + li) * ldcb + (unsigned)((32 * j + 8 * g + 4 * lh) * 2), 0, 0);
                acc[i][j][4 * g + 0] += __uint_as_float(c2[0] << 16);
                acc[i][j][4 * g + 1] += __uint_as_float(c2[0] & 0xffff0000u);
                acc[i][j][4 * g + 2] += __uint_as_float(c2[1] << 16);
                acc[i][j][4 * g + 3] += __uint_as_float(c2[1] & 0xffff0000u);
              }
        }
      }
      const bool relu = (ep & EP_RELU) != 0;
      unsigned char *ot = smem_c + ((last_slot + 1 + wmn / WPS) % NSLOT) * SLOT + (wmn % WPS) * STAGE_W;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          float bias[4][4];
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const u32x2_lw b2 = biasw[j][g];
            bias[g][0] = __uint_as_float(b2[0] << 16);
            bias[g][1] = __uint_as_float(b2[0] & 0xffff0000u);
            bias[g][2] = __uint_as_float(b2[1] << 16);
            bias[g][3] = __uint_as_float(b2[1] & 0xffff0000u);
          }
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
              pk[g][h2] = __builtin_bit_cast(unsigned int, __builtin_convertvector(vv, bf16x2_t)); // one v_cvt_pk_bf16_f32 (RNE)
            }
#pragma unroll
          for (int g = 0; g < 4; g += 2) {
            const auto s0 = __builtin_amdgcn_permlane32_swap(pk[g][0], pk[g + 1][0], false, false);
            const auto s1 = __builtin_amdgcn_permlane32_swap(pk[g][1], pk[g + 1][1], false, false);
            const u32x4 out = {s0[0], s1[0], s0[1], s1[1]};
            // lower half-wave: columns 32j + 8g .. +7 ; upper: 32j + 8(g+1) .. +7
            *(u32x4 *)(ot + li * ES + (32 * j + 8 * g + 8 * lh) * 2) = out;
          }
        }
        // the same wave reads its 32-row block back row-contiguously: 4*TN lanes x 16 B = one row
        constexpr int LPR = 4 * TN, RPP = 64 / LPR; // lanes per row, rows per pass
#pragma unroll
        for (int it = 0; it < 32 / RPP; ++it) {
          const int row = it * RPP + lane / LPR, ch = lane % LPR;
          const u32x4 v = *(const u32x4 *)(ot + row * ES + ch * 16);
          const unsigned voff = (unsigned)(32 * i + row) * ldcb + (unsigned)(ch * 16);
          if (GRP == BLW_ITEMS && ch * 8 < skip_cols) continue; // (a ragged item's last column tile: these columns are the neighbour tile's)
          // (edge tiles: rows and 16-byte pieces in front of the tile's own are the neighbour's - a per-lane predicate on the store.
          // The beta = 1 join above reads the whole block: it lies inside the matrix, and what is not owned is never stored)
          // (a ragged chain: whole column tiles, the row term alone)
          if (EDGE_ROWS && (wm * 32 * TM + 32 * i + row < own_row || (EDGE_COLS && wn * 32 * TN + ch * 8 < own_col))) continue;
          if (MULTI && l + 1 < L) __builtin_amdgcn_raw_buffer_store_b128(v, rsrcC, voff, 0, 16); // sc1: write-through (hand-off)
          else __builtin_amdgcn_raw_buffer_store_b128(v, rsrcC, voff, 0, C_STORE_AUX); // (last layer / single layer: gemm_common.h)
        }
      }
    }
    if constexpr (WRND) {
      if (l + 1 == L) {
        if (!chain_wrounds_more(tn, p.groups, p.L[l].pad / BN)) break;
        // a further column tile of the LAST layer follows: GRP = 7's rendezvous below, nothing to publish
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier(); // S1
        continue;
      }
    }
    if (l + 1 == L && (!ROUNDS || !chain_rounds_more(tm, p.groups, p.tiles_m))) break;
    if constexpr (ROUNDS) {
      if (l + 1 == L) {
        // a further row block of the LAST layer follows: nothing to publish and no store to drain - only the rendezvous behind every
        // wave's epilogue (its staging tile in a retired A half has been read back) before the A loader requests the next step's panels
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier(); // S1
        continue;
      }
    }
    if constexpr (MULTI) {
      // ---- seam: publish this tile to the row block's consumers ------------------------------------------------
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // EVERY storing wave drains its write-through stores
      __builtin_amdgcn_s_barrier();                     // S1
      if (wave == 0 && lane == 0)
        __hip_atomic_fetch_add((g_u32_lw *)(p.cnt + ((size_t)l * p.tiles_m + tm) * CHAIN_CNT_STRIDE), 1u, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

template <int WM, int WN, int WK, int TM, int TN, int NSLOT, int NLA, int NLB, int SUP, bool MULTI, int FLATB = 0, int GRP = 0>
static hipError_t launch_blw_t(const ChainArgs &a, hipStream_t s, const void *items = nullptr, int n_items = 0) {
  constexpr int NOUT = WM * WN, BM = 32 * WM * TM, BN = 32 * WN * TN, NT = 64 * (WM * WN * WK + NLA + NLB);
  constexpr size_t lds = (size_t)NSLOT * (BM + BN) * 128 + (WK > 1 ? (size_t)NOUT * 4096 : 0);
  static_assert(lds <= 160 * 1024, "LDS budget");
  auto kern = brgemm_bf16_lw<WM, WN, WK, TM, TN, NSLOT, NLA, NLB, SUP, MULTI, FLATB, GRP>;
  static std::atomic<unsigned long long> lds_set{0};
  if (hipError_t e = ensure_dynamic_lds((const void *)kern, (int)lds, lds_set); e != hipSuccess) return e;
  ChainArgs args = a;
  constexpr bool EDGE = blw_edge_rows(GRP); // (a ragged chain: rows only - n % BN == 0 is blw_launch_ok's check)
  args.tiles_m = EDGE ? (a.m + BM - 1) / BM : a.m / BM; // (edge tiles: ceil-divided both ways, m >= BM and n >= BN)
  args.tiles_n = blw_edge_cols(GRP) ? (a.n + BN - 1) / BN : a.n / BN; // (grouped items: a ragged last column tile, see the kernel)
  long long tiles = (long long)args.tiles_m * args.tiles_n;
  if (EDGE && (a.m < BM || a.n < BN)) return hipErrorInvalidValue;
  if (tiles <= 0 || tiles > 0x7fffffffLL) return hipErrorInvalidValue;
  // GRP = 7 (several rounds): a.groups row groups are resident, each a row of tiles_n workgroups; the grid and the XCD search below
  // count row groups where the other launches count row blocks
  int grid_m = args.tiles_m;
  [[maybe_unused]] int grid_n = args.tiles_n;
  if constexpr (GRP == BLW_CHAIN_ROUNDS) {
    if (a.m % BM != 0 || a.n % BN != 0 || a.groups < 1 || a.groups > args.tiles_m) return hipErrorInvalidValue;
    grid_m = a.groups;
    tiles = (long long)grid_m * args.tiles_n;
  } else if constexpr (blw_chain_wrounds(GRP)) {
    // GRP = 10 (column rounds): a.groups workgroup COLUMNS are resident; tiles_n stays the widest layer's column tiles
    if (a.groups < 1 || a.groups >= args.tiles_n) return hipErrorInvalidValue;
    grid_n = a.groups;
    tiles = (long long)grid_m * grid_n;
  } else {
    args.groups = 0;
  }
  args.items = nullptr;
  args.item_subs = 0;
  args.pad_items = 0;
  if constexpr (blw_items(GRP)) { // tiles_m x tiles_n workgroups per item (consecutive workgroups = the items in list order: neighbouring
                       // tiles of a layer share panels in the L2 of whichever XCD they land on)
    if (!items || n_items <= 0 || tiles * n_items > 0x7fffffffLL) return hipErrorInvalidValue;
    args.items = items;
    args.item_subs = (int)tiles;
    args.xm = 0;
    hipLaunchKernelGGL(kern, dim3((unsigned)(tiles * n_items)), dim3(NT), lds, s, args);
    return hipGetLastError();
  }
  // XCD grid xm x (8 / xm) over the tile grid: minimise xn * m + xm * n (bytes of A and W all eight L2s fetch, in units of 2K)
  args.xm = 0;
  long long best = -1;
  for (int xm = 8; xm >= 1; xm >>= 1) {
    const int xn = 8 / xm;
    if (grid_m % xm || (blw_chain_wrounds(GRP) ? grid_n : args.tiles_n) % xn) continue;
    const long long cost = (long long)xn * a.m + (long long)xm * a.n;
    if (best < 0 || cost < best) {
      best = cost;
      args.xm = xm;
    }
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)tiles), dim3(NT), lds, s, args);
  return hipGetLastError();
}

// (brgemm_bf16_lw_chain_ragged.hip includes this file for the kernel, the loader and launch_blw_t alone: the launchers and the 120 instances
// of the launch table below are this translation unit's)
#ifndef BLW_KERNEL_ONLY
// THE DISPATCHER: the instance of a compile-time (MULTI, GRP) for a run-time (tile, sup, b_kind), through the tile table of
// brgemm_bf16_lw_launch.h. Combination I of the 5 tiles x 3 B images x 2 chunks per barrier is compiled only where blw_instance_exists
// says so; everything else is refused with hipErrorInvalidValue.
template <bool MULTI, int GRP, int I>
static bool blw_try(int tile, int sup, int b_kind, const ChainArgs &a, hipStream_t s, const void *items, int n_items, hipError_t &e) {
  constexpr int TILE = I / 6, FB = 2 * (I / 2 % 3), SUP = 1 + I % 2;
  if constexpr (blw_instance_exists(GRP, MULTI, TILE, FB, SUP)) {
    if (tile == TILE && b_kind == FB && sup == SUP) {
      constexpr BlwTile t = BLW_TILES[TILE];
      e = launch_blw_t<t.wm, t.wn, t.wk, t.tm, t.tn, t.nslot, t.nla, t.nlb, SUP, MULTI, FB, GRP>(a, s, items, n_items);
      return true;
    }
  }
  return false;
}
template <bool MULTI, int GRP, int... I>
static hipError_t blw_dispatch_seq(std::integer_sequence<int, I...>, int tile, int sup, int b_kind, const ChainArgs &a, hipStream_t s, const void *items, int n_items) {
  hipError_t e = hipErrorInvalidValue;
  (void)(blw_try<MULTI, GRP, I>(tile, sup, b_kind, a, s, items, n_items, e) || ...);
  return e;
}
template <bool MULTI, int GRP>
static hipError_t blw_dispatch(int tile, int sup, int b_kind, const ChainArgs &a, hipStream_t s, const void *items = nullptr, int n_items = 0) {
  return blw_dispatch_seq<MULTI, GRP>(std::make_integer_sequence<int, BLW_NTILES * 6>{}, tile, sup, b_kind, a, s, items, n_items);
}
// what blw_launch_ok reads of an argument block
static BlwShape blw_shape(const ChainArgs &a, bool chain) {
  BlwShape h{chain, a.m, a.n, a.nlayers, a.groups, {}, {}};
  for (int l = 0; l < (a.nlayers < 1 ? 1 : a.nlayers > CH_MAXL ? CH_MAXL : a.nlayers); ++l) h.k[l] = a.L[l].k, h.br[l] = a.L[l].br;
  return h;
}
// chunks per barrier of a layer / chain launch: two on the tiles that have such instances when every layer has an even chunk count
static int blw_sup(int mode, int tile, const ChainArgs &a) {
  if (blw_one_chunk(mode) || !blw_tile_sup2(tile)) return 1;
  for (int l = 0; l < a.nlayers; ++l)
    if ((a.L[l].br * (a.L[l].k / BLW_BK)) & 1) return 1;
  return 2;
}

// ONE LAYER (a.nlayers == 1) in one of the modes BLW_LAYER, BLW_EDGE, BLW_KEDGE, BLW_KEDGE8 (brgemm_bf16_lw_launch.h; blw_launch_ok is what
// each refuses: hipErrorInvalidValue, nothing launched). No scratch, no counters, no waits. b_kind: the B image -
//   0  VNNI-2 [k/2][ldb][2].
//   2  FLAT [k][ldb] (no VNNI flag on the dispatch - what xsmm.unary pack would have turned into VNNI-2, lib/TPP/Transforms/Utils/
//      VNNIUtils.cpp:75-77): the chunk's 64 rows go into LDS as they are (LDS-DMA, 64-byte blocks swizzled on the source side) and a B
//      fragment is two ds_read_b64_tr_b16 - the hardware transpose hands every lane four consecutive k of its own column. No pack
//      launch, no VALU, and the reads run at the LDS's full 256 B/clk where the VNNI image needs 4-byte reads (128 B/clk): bit-identical
//      to pack + VNNI kernel and as fast or faster on every tile (profiles/r03_flat_b_bf16.txt). A first version interleaved the
//      pair-rows in a register-staging B loader (buffer_load_dwordx4 x 2 -> 8 v_perm_b32 -> 2 ds_write_b128): correct, 15-28 % slower
//      (the ds_write path: ~79 B/clk and 2-way conflicts), removed.
//   4  VNNI-4 [k/4][ldb][4] (the dispatch carries the VNNI flag, the factor is the runtime's setting, xsmm_hip_set_vnni_factor -
//      lib/TPP/Transforms/Utils/VNNIUtils.cpp:25-45, benchmarks/config/omp/mlir-bf16.json:68-100): the chunk's 16 k-group rows go into
//      the LDS as they are and a fragment is two 8-byte reads (256 B/clk).
// BLW_EDGE (gemm_plan.cpp choose_bf16_edge_tile): ceil(m / BM) x ceil(n / BN) workgroups, the last tile of a row / column of tiles ends at the
// matrix edge and stores only what no other tile owns. BLW_KEDGE / BLW_KEDGE8 (gemm_plan.cpp plan_gemm_call, brgemm_bf16_lw_kedge.h): the same
// + the shifted last chunk per batch element; one chunk per barrier only (one barrier per two chunks would tie the ragged chunk to a partner).
hipError_t launch_bf16_lw(int mode, int tile, int b_kind, const ChainArgs &a, hipStream_t s) {
  if (!blw_launch_ok(mode, tile, b_kind, blw_shape(a, false))) return hipErrorInvalidValue;
  const int sup = blw_sup(mode, tile, a);
  switch (mode) {
  case BLW_LAYER: return blw_dispatch<false, BLW_LAYER>(tile, sup, b_kind, a, s);
  case BLW_EDGE: return blw_dispatch<false, BLW_EDGE>(tile, sup, b_kind, a, s);
  case BLW_KEDGE: return blw_dispatch<false, BLW_KEDGE>(tile, sup, b_kind, a, s);
  case BLW_KEDGE8: return blw_dispatch<false, BLW_KEDGE8>(tile, sup, b_kind, a, s);
  default: return hipErrorInvalidValue;
  }
}

// Tile invokes of ONE bf16 descriptor as one launch on the loader-wave tiles (round 6, VERDICT r5 missing 3 / next 2b: the tile queue's
// bf16 groups used to run on brgemm_bf16_small32 / brgemm_bf16_fast<64x64> and were 0-45 % slower than the same layer as one whole-
// layer call). One workgroup per BM x BN tile of an item, operands and batch count from the item (ChainArgs::items); packed tile
// blocks are just another (lda, stride) pattern to the loaders. SUP = 2 instances only when every item has an even chunk count.
// (Tile 4 with VNNI-4 operands: the image rows of a 32-column tile are 256 bytes, four per DMA instruction.)
hipError_t launch_bf16_lw_grouped(int tile, int b_kind, const ChainArgs &a, const void *items, int n_items, bool even_chunks, hipStream_t s) {
  if (!blw_launch_ok(BLW_ITEMS, tile, b_kind, blw_shape(a, false))) return hipErrorInvalidValue;
  return blw_dispatch<false, BLW_ITEMS>(tile, even_chunks ? 2 : 1, b_kind, a, s, items, n_items);
}

// QUADS (round 6): a group of 64x64 items that forms an R x C grid of item rows (A blocks) and item columns (B blocks), R and C even,
// as 2 x 2 blocks on the 128x128 tile - what the same layer runs on as one whole-layer call when it is large (1024 x 2560 x 1024:
// 640 items on 64x64 tiles 15.3 us, 160 workgroups of 128x128 10.2). a.m = a.n = 128 (one tile per quad), lda / ldb / ldc / strides /
// k the items'; quads = QuadItem[n_quads] in device-visible memory.
hipError_t launch_bf16_lw_quads(int b_kind, const ChainArgs &a, const void *quads, int n_quads, hipStream_t s) {
  if (!blw_launch_ok(BLW_QUADS, 3, b_kind, blw_shape(a, false))) return hipErrorInvalidValue;
  return blw_dispatch<false, BLW_QUADS>(3, 1, b_kind, a, s, quads, n_quads);
}

// A CHAIN of layers in one launch; the caller guarantees co-residency, beta = 0, disjoint buffers and ONE kind of B operand for every
// layer. blw_launch_ok is what each mode refuses (hipErrorInvalidValue, nothing launched).
//   BLW_LAYER         m / BM x n / BN workgroups, at most the compute units.
//   BLW_CHAIN_EDGE    (gemm_plan.cpp plan_chain_edge, brgemm_bf16_lw_chain_edge.h) ceil(m / BM) x n / BN workgroups, at most the compute units: the
//                     last row block shifted back to end at row m, storing its own rows only and waiting at every seam for both row blocks
//                     whose rows it reads.
//   BLW_CHAIN_ROUNDS  (gemm_plan.cpp plan_chain_rounds, brgemm_bf16_lw_chain_rounds.h) a.groups x n / BN resident workgroups, at most the compute
//                     units: workgroup (g, tn) walks the row blocks g, g + groups, .. of every layer, layer-major; the counters are the
//                     chain's, [nlayers - 1][m / BM].
hipError_t launch_bf16_chain(int mode, int tile, int b_kind, const ChainArgs &a, hipStream_t s) {
  if (!blw_launch_ok(mode, tile, b_kind, blw_shape(a, true))) return hipErrorInvalidValue;
  const int sup = blw_sup(mode, tile, a);
  switch (mode) {
  case BLW_LAYER: return blw_dispatch<true, BLW_LAYER>(tile, sup, b_kind, a, s);
  case BLW_CHAIN_EDGE: return blw_dispatch<true, BLW_CHAIN_EDGE>(tile, sup, b_kind, a, s);
  case BLW_CHAIN_ROUNDS: return blw_dispatch<true, BLW_CHAIN_ROUNDS>(tile, sup, b_kind, a, s);
  default: return hipErrorInvalidValue;
  }
}
#endif // BLW_KERNEL_ONLY

} // namespace tpp
