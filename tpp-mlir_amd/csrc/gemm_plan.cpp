// gemm_plan.cpp - the GEMM kernel planner (gemm_plan.h): host-only, no kernels, no HIP runtime calls. Its choices, case by case, are
// tests/golden/gemm_plan.txt (tests/test_gemm_plan.py): a change of a rule or a cost coefficient is a change of that table.
#include "gemm_plan.h"
#include "brgemm_f32_lw_kedge.h"
#include "brgemm_bf16_lw_launch.h" // the tile table; brgemm_bf16_lw_kedge.h
#include "brgemm_bf16_lw_chain_rounds.h"
#include "brgemm_bf16_dma256_images.h"
#include "brgemm_bf16_dma256_chain.h"
#include "brgemm_bf16_skinny.h"
#include "brgemm_bf16_skinny_split.h"
#include "brgemm_bf16_skinny_chain.h"
#include <string.h>

namespace tpp {

constexpr int BK = 64;           // k per chunk of the tiled kernels (BK of brgemm_f32.hip, BKH of brgemm_bf16.hip, ...)
constexpr int GK = 32;           // k per chunk of the generic kernel (brgemm_f32.hip brgemm_grouped)
constexpr int SPLIT_MAX_WG = 16; // = SPLIT_MAX of split_scratch.h
// what handing a tile's partial sums over between the workgroups of a SPLIT launch costs, in us: three dependent trips to the memory
// side (partial tile written through and acknowledged, arrival counter, the other partials read back) - 2.6-2.7 us measured - and a margin
constexpr double SPLIT_HANDOFF_US = 2.7 + 0.8;

static int64_t rounds(int64_t workgroups, int64_t cus) { return (workgroups + cus - 1) / cus; } // of one workgroup per CU

// the f32 loader-wave families (brgemm_f32_lw.hip, brgemm_f32_lw16.hip, brgemm_f32_x6.hip): 16-byte A / B row pieces, 32-bit lane offsets
static bool f32_lw_operands_ok(const GemmDesc &d) {
  return !((d.lda | d.ldb | d.stride_a | d.stride_b) & 3) && d.lda < (1 << 22) && d.ldb < (1 << 22) && d.ldc < (1 << 22);
}
// 32-k f32 tiles on the loader-wave kernels' pair mode (a 64-k chunk from the blocks of two batch elements): the strides in 32 bits
static bool f32_pairs_ok(const GemmDesc &d) {
  return d.k == 32 && d.stride_a >= 0 && d.stride_b >= 0 && d.stride_a < (1 << 26) && d.stride_b < (1 << 26);
}
// shapes the bf16x6 split kernel takes: the f32 loader-wave family's preconditions (pick_f32_variant) plus ldc a multiple of 4
static bool f32_x6_eligible(const GemmDesc &d) {
  return d.k > 0 && d.k % BK == 0 && d.m % 32 == 0 && d.n % 32 == 0 && !(d.ldc & 3) && f32_lw_operands_ok(d);
}

// bf16 + VNNI-2 B, k a multiple of 64, m and n of 64, 16-byte-aligned leading dimensions within the 32-bit lane offsets: what the
// LDS-DMA bf16 tile families (brgemm_bf16.hip, brgemm_bf16_lw.hip) need
static bool bf16_fast_eligible(const GemmDesc &d) { // (VNNI-4 operands: bf16_vnni4_eligible)
  return d.dtype == DT_BF16 && d.vnni_b && d.vnni_factor == 2 && d.k > 0 && d.k % BK == 0 && d.m % 64 == 0 && d.n % 64 == 0 &&
         !((d.lda | d.ldc | d.stride_a | d.stride_b) & 7) && !(d.ldb & 3) && d.lda < (1 << 22) && d.ldb < (1 << 21) && d.ldc < (1 << 22);
}
// flat-B bf16 for the loader-wave tiles: 16-byte row pieces of A, B and C, 64-k chunks, 32-bit lane offsets
static bool bf16_flat_eligible(const GemmDesc &d) {
  return d.dtype == DT_BF16 && !d.vnni_b && !d.vnni_c && d.k > 0 && d.k % 64 == 0 && d.m % 32 == 0 && d.n % 64 == 0 &&
         !((d.lda | d.ldb | d.ldc | d.stride_a | d.stride_b) & 7) && d.lda < (1 << 22) && d.ldb < (1 << 21) && d.ldc < (1 << 22);
}
// VNNI-4 B for the loader-wave tiles: k-group rows of 8 * ldb bytes in 16-byte pieces, 64-k chunks, 32-bit lane offsets
static bool bf16_vnni4_eligible(const GemmDesc &d) {
  return d.dtype == DT_BF16 && d.vnni_b && d.vnni_factor == 4 && !d.vnni_c && d.k > 0 && d.k % 64 == 0 && d.m % 32 == 0 && d.n % 64 == 0 &&
         !((d.lda | d.ldc | d.stride_a | d.stride_b) & 7) && !(d.ldb & 1) && d.lda < (1 << 22) && d.ldb < (1 << 20) && d.ldc < (1 << 22);
}
// item lists on the loader-wave tiles (brgemm_bf16_lw.hip launch_bf16_lw_grouped / launch_bf16_lw_quads; VNNI-2 or VNNI-4 B): the
// operand limits those launches were written and measured with - tighter than the whole-layer tiles' (lda < 2^21 against 2^22, ldb
// < 2^20 against 2^21 for VNNI-2), non-negative strides - and neither a forced kernel nor a VNNI C. n is the caller's.
static bool bf16_lw_items_ok(const GemmDesc &d, bool v4) {
  return d.dtype == DT_BF16 && d.vnni_b && !d.vnni_c && !d.generic_forced && !d.variant_forced && d.k > 0 && d.k % BK == 0 && d.m % 32 == 0 &&
         !((d.lda | d.stride_a | d.stride_b | d.ldc) & 7) && !(d.ldb & (v4 ? 1 : 3)) && d.lda < (1 << 21) && d.ldb < (1 << 20) &&
         d.ldc < (1 << 22) && d.stride_a >= 0 && d.stride_b >= 0;
}
// the 32x32 K-split bf16 kernel (brgemm_bf16_small.hip): fragments straight from global memory, 16-k steps, 8-byte output pieces
static bool bf16_small_operands_ok(const GemmDesc &d) {
  return d.dtype == DT_BF16 && d.vnni_b && d.m % 32 == 0 && d.k > 0 && d.k % 16 == 0 && !(d.lda & 7) && !(d.stride_a & 7) && !(d.ldc & 3);
}
static bool bf16_small_eligible(const GemmDesc &d) {
  return bf16_small_operands_ok(d) && d.vnni_factor == 2 && d.n % 32 == 0 && !(d.stride_b & 1);
}
// 2 x 2 blocks of 64x64 items on the 128x128 loader-wave tile (QUADS, launch_gemm_quads)
static bool quads_shape_ok(const GemmDesc &d) {
  const bool v2 = d.vnni_factor == 2 || d.vnni_factor == 0, v4 = d.vnni_factor == 4;
  return (v2 || v4) && !d.b_trans && d.m == 64 && d.n == 64 && bf16_lw_items_ok(d, v4);
}

// the generic kernel (brgemm_f32.hip brgemm_grouped) and which 16-byte load paths it may take (vec_ok: every A and B 16-byte aligned):
// vec f32 16-byte pieces (32-bit tile-relative lane offsets: 32 rows x ld x 4 B < 2^31); vec16 bf16 + VNNI-2 B, 8-element A pieces,
// pair-rows of B 16-byte aligned; vec16_4 bf16 + VNNI-4 B, 16-byte pieces of 2 columns
struct GenericOk { bool vec, vec16, vec16_4; };
static GenericOk generic_ok(const GemmDesc &d, bool vec_ok) {
  const bool tiles_ok = vec_ok && d.n % 4 == 0 && d.k % GK == 0; // ragged m / n edges are predicated
  const bool vec16x = d.dtype == DT_BF16 && d.vnni_b && !((d.lda | d.stride_a | d.stride_b) & 7) && d.lda < (1 << 21) && d.ldb < (1 << 21);
  GenericOk g;
  g.vec = vec_ok && d.n % 4 == 0 && d.k % 4 == 0 && d.dtype == DT_F32 && !d.vnni_b && !((d.lda | d.ldb | d.stride_a | d.stride_b) & 3) &&
          d.lda < (1 << 24) && d.ldb < (1 << 24);
  g.vec16 = tiles_ok && vec16x && d.vnni_factor == 2 && !(d.ldb & 3);
  g.vec16_4 = vec16x && d.vnni_factor == 4 && vec_ok && d.n % 2 == 0 && d.k % GK == 0 && !(d.ldb & 1);
  return g;
}
static GemmGeneric generic_kernel(const GemmDesc &d, const GenericOk &g) { // (VNNI-4 B: on the bf16 MFMA path with 16-byte pieces only)
  if (d.dtype == DT_F32) return g.vec ? GG_F32_VEC : GG_F32;
  return !d.vnni_b ? GG_BF16_FLAT : g.vec16_4 ? GG_BF16_VNNI4_VEC : g.vec16 ? GG_BF16_VNNI2_VEC : GG_BF16_VNNI2;
}

// The bf16 loader-wave tiles (brgemm_bf16_lw.hip), fitted to the sweep of the reference's whole shape set over every tile
// (tools/bf16_sweep.py, profiles/r06_bf16_sweep.txt): a launch costs rounds x (a + b x chunks), rounds = ceil(workgroups / CUs) (one
// workgroup per CU: a second round is a second kernel's worth), (a, b) in us from the K = 1024 / K = 4096 pairs of the sweep. Tile index
// as launch_bf16_lw: 0 = 32x64 + K2, 1 = 64x64, 2 = 64x128, 3 = 128x128, 4 = 32x32 + K2 (from 128 x 1024 x 1024 / x 4096 on that tile).
static const double BLW_A[5] = {3.56, 3.75, 4.66, 6.06, 3.52}, BLW_B[5] = {0.098, 0.135, 0.204, 0.236, 0.072};
static double blw_cost(int tile, int64_t rounds, double chunks) { return (double)rounds * (BLW_A[tile] + BLW_B[tile] * chunks); }

// f32: rounds of workgroups x per-chunk time - one 64x32 workgroup per CU at a time (96 KiB of LDS), two 32x32 ones (64 KiB). 256 x
// 3072 (384 tiles of 64x32 = 1.5 rounds) measured 15.9 us against 12.6 on 768 tiles of 32x32; where the rounds tie (C3: 256 / 512
// tiles, 128 x 4096) the larger tile stays - same time, half the LDS traffic (profiles/r05_split_sweep.txt)
static bool f32_32x32_beats_64x32(int64_t t32, int64_t t6432, int64_t cus) {
  return 0.23 * 1.05 * (double)rounds(t32, cus) < 0.46 * (double)rounds(t6432, cus);
}

// How many workgroups share the batch-reduce range of ONE output tile (SPLIT kernels of brgemm_f32_lw.hip) - 1 = no split.
// tile: 1 = 64x64 + K2, 2 = 64x32 + K4, 3 = 32x32 + K4; tiles: output tiles of the whole launch; chunks: 64-k chunks per tile.
// Fitted to profiles/r05_split_sweep.txt (whole-layer calls of the reference's skinny benchmark shapes over tile x split count):
//  * a workgroup alone on a CU needs c(tile) us per chunk (the matrix pipes' rate: 0.213 us for a 32x32x64 chunk);
//  * a split costs the hand-off whatever the count, so it pays only where it takes more than that off the K loop;
//  * more workgroups than CUs never paid: 128 x 1024 x 4096 on 32x32 tiles 17.1 us unsplit, 12.9 (S = 2: 256 workgroups), 13.6 (S = 4:
//    512), 15.6 (6), 20.6 (8) - every further round of workgroups pays its own prologue and hand-off.
// Hence: the largest S with tiles * S <= CUs, if the K-loop time it saves exceeds the hand-off. The answer depends on the
// descriptor, the batch count and the number of tiles in the launch only: the same call pattern always adds in the same order.
// xsmm_hip_force_split / TPP_HIP_SPLIT: 0 / 1 = never split, n > 1 = always n (clamped to the chunks), -1 = this model.
// the model's answer when a tile may take at most `room` workgroups (1 = no split)
static int f32_split_model(int tile, long long room, long long chunks) {
  const long long smax = chunks < SPLIT_MAX_WG ? chunks : SPLIT_MAX_WG;
  const double c = tile == 1 ? 0.92 : tile == 2 ? 0.46 : 0.213;
  long long S = room;
  if (S > smax) S = smax;
  if (S > chunks / 4) S = chunks / 4; // at least four chunks per workgroup
  if (S < 2) return 1;
  const long long per = (chunks + S - 1) / S;
  const double saved = c * (double)(chunks - per);
  return saved > SPLIT_HANDOFF_US ? (int)S : 1;
}
static int choose_f32_split(int tile, long long tiles, long long chunks, const GemmPlanEnv &env) {
  const int forced = env.forced_split;
  if (tile < 1 || tile > 3 || tiles <= 0 || chunks < 2) return 1;
  const long long smax = chunks < SPLIT_MAX_WG ? chunks : SPLIT_MAX_WG;
  if (forced >= 0) return forced <= 1 ? 1 : (int)(forced < smax ? forced : smax);
  return f32_split_model(tile, env.cus / tiles, chunks);
}

// TAIL SPLIT (xsmm_hip_set_tail_split, opt-in): a launch of q CUs + r tiles, q >= 1, runs q full rounds of workgroups and a last one
// that occupies r CUs for a whole K loop. With 0 < r <= CUs / 2 the r tiles of that round are split over the CUs it leaves idle, the
// q CUs tiles in front of them run unsplit, all in one launch (brgemm_f32_lw.hip launch_f32_lw_tail). Mode 1: the split model above
// with CUs / r workgroups of room per tail tile; mode n >= 2 (tests, measurements): n workgroups per tail tile (at most 16 and the
// chunks) wherever r n <= CUs, no saving test. Off while a split count is forced. Returns the workgroups per tail tile (1 = no
// tail split) and the tail tiles. Descriptor, batch count and CU count only, like the split: allowed in strict mode.
static int choose_f32_tail_split(int tile, long long tiles, long long chunks, const GemmPlanEnv &env, int *tail_tiles) {
  *tail_tiles = 0;
  if (env.tail_split == 0 || env.forced_split >= 0 || tile < 1 || tile > 3 || env.cus <= 0 || tiles <= env.cus) return 1;
  const long long r = tiles % env.cus;
  if (r == 0 || r > env.cus / 2) return 1;
  long long S;
  if (env.tail_split == 1) S = f32_split_model(tile, env.cus / r, chunks);
  else {
    S = env.tail_split < SPLIT_MAX_WG ? env.tail_split : SPLIT_MAX_WG;
    if (S > chunks) S = chunks;
    if (r * S > env.cus) S = 1;
  }
  if (S < 2) return 1;
  *tail_tiles = (int)r;
  return (int)S;
}

// HALVES (xsmm_hip_set_f32_halves; brgemm_f32_lw.hip launch_f32_lw_halves): a whole-layer call on the 64x64 + K2 tile whose every tile
// runs as two independent 64x32 + K2 workgroups, two to a CU - the same bits, so the variant, the kernel name and the launch's text stay
// what they are. Eligible: tile 1 with no split and no tail split (the caller's), m and n in whole 64x64 tiles; edge tiles and ragged k
// are planned elsewhere and never come here, queued groups and chains do not go through plan_gemm_call. Mode 2 (tests, measurements):
// wherever eligible. Mode 1, the rule: at least one tile per CU - every such class measured faster on one box
// (profiles/f32_halves_ab.txt): one round (C2 17.64 -> 17.19 us in six of six alternating pairs, 1024 x 1024 x 512 10.57 -> 10.27), two
// rounds (2048 x 1024 x 1024 33.98 -> 32.69), and most where the last round is partial, because a half is also half the scheduling
// unit: 1.5 rounds (1024 x 1536 x 1024 33.62 -> 25.6), 2.5 rounds (1024 x 2560 x 1024 49.93 -> 41.26). Fewer tiles than CUs - a forced
// tile only, the planner takes smaller tiles there - have not been measured and stay as they are.
// Descriptor and CU count only: allowed in strict mode.
static bool choose_f32_halves(int tile, const GemmDesc &d, long long tiles, const GemmPlanEnv &env) {
  if (env.halves == 0 || tile != 1 || tiles <= 0 || d.m % 64 != 0 || d.n % 64 != 0) return false;
  return env.halves == 2 || tiles >= env.cus;
}

// The 32x32 K-split bf16 kernel over several workgroups per tile, for skinny groups with a long reduction (the kernel is a
// latency-bound stream: 0.047 us per 16-k step of a workgroup). Measured (profiles/r05_bf16_skinny_small_vs_lw.txt): it pays only
// while every workgroup still has a CU to itself - 128 x 1024 x 4096 as 64x64x64 tile invokes 12.0 -> 9.8 us at S = 2 (10.3 at 4,
// 13.1 at 8), 256 x 1024 x 4096 12.3 -> 14.2 at S = 2. Hence the largest count with tiles x S <= CUs and at least 32 steps per
// workgroup, if it saves more than the hand-off costs. xsmm_hip_force_split overrides.
static int choose_bf16_small_split(long long t32, long long steps, const GemmPlanEnv &env) {
  int S = 1;
  const int forced = env.forced_split;
  if (forced >= 0) S = forced <= 1 ? 1 : (int)(forced < 16 ? forced : 16);
  else if (t32 > 0) {
    long long c = (long long)env.cus / t32;
    if (c > 16) c = 16;
    if (c > steps / 32) c = steps / 32;
    if (c >= 2 && 0.047 * (double)(steps - (steps + c - 1) / c) > SPLIT_HANDOFF_US) S = (int)c;
  }
  if (S > (int)steps) S = steps > 1 ? (int)steps : 1;
  return S;
}

// EDGE TILES (xsmm_hip_set_edge_tiles, opt-in): a whole-layer f32 call whose m or n no loader-wave tile divides - planned on the generic
// kernel - on the loader-wave tiles all the same: the last tile of a row or column of tiles is shifted back inside the matrix and stores
// only the elements no other tile owns (brgemm_f32_lw.hip brgemm_f32_lw_edge). A tile is a candidate when m >= BM and n >= BN. Mode 1:
// the comparisons pick_f32_variant makes among 128x64, 64x64 + K2, 64x32 + K4 and 32x32 + K4 - rounds of workgroups, the 1.85x round of
// 128x64, f32_32x32_beats_64x32, a tile per CU before a larger tile is taken - on CEIL-DIVIDED tile counts (the half-width tiles and
// the split launches have no edge form). Modes 6, 7, 9, 10 (tests, measurements): that GemmVariant's tile. Returns the variant, -1 = none.
// No rule of mode 1 is fitted to a ragged shape yet: profiles/edge_tiles_ab.txt.
// (mode 2 = mode 1 for f32 + the bf16 rule, choose_bf16_edge_tile; modes 20 .. 23 force a bf16 tile and leave f32 calls as with the mode off)
static int f32_edge_mode(int mode) { return mode == 2 ? 1 : mode >= 20 ? 0 : mode; }
static int choose_f32_edge_variant(const GemmDesc &d, int mode, int64_t cus) {
  const int64_t m = d.m, n = d.n;
  auto tiles = [&](int bm, int bn) { return (m >= bm && n >= bn) ? ((m + bm - 1) / bm) * ((n + bn - 1) / bn) : 0; };
  if (mode == V_F32_LW_64x64K2) return tiles(64, 64) > 0 ? mode : -1;
  if (mode == V_F32_LW_64x32K2) return tiles(64, 32) > 0 ? mode : -1;
  if (mode == V_F32_LW_32x32K4) return tiles(32, 32) > 0 ? mode : -1;
  if (mode == V_F32_LW_128x64) return tiles(128, 64) > 0 ? mode : -1;
  if (mode != 1) return -1;
  if (tiles(64, 64) >= cus) {
    const int64_t r64 = rounds(tiles(64, 64), cus), r128 = rounds(tiles(128, 64), cus);
    if (tiles(128, 64) > 0 && 1.85 * (double)r128 < (double)r64) return V_F32_LW_128x64;
    return V_F32_LW_64x64K2;
  }
  if (tiles(64, 32) >= cus) {
    if (tiles(32, 32) > 0 && f32_32x32_beats_64x32(tiles(32, 32), tiles(64, 32), cus)) return V_F32_LW_32x32K4;
    return V_F32_LW_64x32K2;
  }
  if (tiles(32, 32) > 0 && tiles(32, 32) >= tiles(64, 64) * 2 && tiles(64, 32) < cus) return V_F32_LW_32x32K4;
  if (tiles(64, 64) > 0) return V_F32_LW_64x64K2;
  if (tiles(64, 32) > 0) return V_F32_LW_64x32K2;
  if (tiles(32, 32) > 0) return V_F32_LW_32x32K4;
  return -1;
}

static int pick_f32_variant(const GemmDesc &d, int64_t cus) {
  if (d.k <= 0 || d.k % BK) return V_GENERIC;
  if (!f32_lw_operands_ok(d)) return V_GENERIC;
  const int64_t m = d.m, n = d.n;
  auto tiles = [&](int bm, int bn) { return (m % bm == 0 && n % bn == 0) ? (m / bm) * (n / bn) : 0; };
  // 64-row tiles run on the loader-wave kernels (brgemm_f32_lw.hip). Measured on C2 (256 tiles of 64x64, uniform
  // [-1, 1) inputs, profiles/r02_f32_variants.txt): 64x64 with the K chunks split over two wave groups (two MFMA
  // waves per SIMD cover each other's barrier stalls) 18.3 us, one group 18.7 us, the round-1 kernel 19.7-20.4 us.
  // Outputs with at least one 64x64 tile per CU: 64x64 or 128x64 tiles, whichever needs less time over its rounds
  // of workgroups (one per CU at a time). A 128x64 round takes ~1.85x a 64x64 round (measured, K = 1024: 32.7 vs
  // 17.6 us), so 128x64 wins at 1280-2048 x 1024 (one round instead of two) and for large outputs (0.93x), and
  // loses e.g. at 3072 x 1024 (two rounds against three).
  // Skinny outputs - at most one 32x16 tile per CU (the reference's M = 128 shapes: 128 x 1024 = 256 tiles, 128 x 768 = 192): the
  // half-width tiles of brgemm_f32_lw16.hip put a workgroup on every CU where 32x32 tiles would leave half the chip idle, and need
  // no hand-off between workgroups (the SPLIT launches pay 2.6-2.7 us for one); profiles/r05_lw16_vs_split.txt
  // (a 16x48 tile of the same family - 256 x 768 outputs are exactly 256 of them - was built and measured: 256 x 768 x 768 5.59 us
  // against 5.48 on 192 tiles of 32x32, x 3072 14.9 against 13.7: 16 KiB of panel per 98 kflop chunk, the launch is bound by the
  // L2 -> LDS traffic of all CUs together, ~16 TB/s; removed. profiles/r05_lw16_vs_split.txt)
  if (d.ldc % 4 == 0 && tiles(32, 16) > 0 && tiles(32, 16) <= cus) return V_F32_LW16_32x16;
  if (tiles(64, 64) >= cus) {
    const int64_t r64 = rounds(tiles(64, 64), cus), r128 = rounds(tiles(128, 64), cus);
    if (tiles(128, 64) > 0 && 1.85 * (double)r128 < (double)r64) return V_F32_128x64;
    return V_F32_LW_64x64K2;
  }
  if (tiles(64, 32) >= cus) {
    if (tiles(32, 32) > 0 && f32_32x32_beats_64x32(tiles(32, 32), tiles(64, 32), cus)) return V_F32_LW_32x32K4;
    return V_F32_LW_64x32K2;
  }
  if (tiles(32, 32) > 0 && tiles(32, 32) >= tiles(64, 64) * 2 && tiles(64, 32) < cus) return V_F32_LW_32x32K4;
  if (tiles(64, 64) > 0) return V_F32_LW_64x64K2;
  if (tiles(64, 32) > 0) return V_F32_LW_64x32K2;
  if (tiles(32, 32) > 0) return V_F32_LW_32x32K4;
  return V_GENERIC;
}

// tile choice for an eligible descriptor: 0 = 64x64 register-staged, 1 = 128x128 DMA, 2 = 256x256 DMA.
//  * 256 x 256 (LDS / L2 traffic per flop halves: measured 1.31-1.37 vs 0.88-1.03 PFLOP/s on 4096^3 ..
//    8192^3) when its tile waves fill the 256 CUs well enough to keep that 1.4x: tiles run one per CU,
//    so a grid of t tiles takes ceil(t / 256) rounds;
//  * 128 x 128 as soon as the 64 x 64 family would need a second round of workgroups (more than 256 tiles of
//    64 x 64 = more than 64 of 128 x 128): measured (n = 1024, K = 1024) the DMA kernel takes 9.2-9.4 us from 64
//    to 256 tiles while the 64 x 64 family jumps from 9.1 to 12.8 us past one tile per CU;
//  * 64 x 64 below that, so that more CUs have work.
static int pick_bf16_tile(const GemmDesc &d) {
  constexpr int64_t t256_min = 240, t128_min = 65; // crossovers measured in profiles/r01_sweep_shapes.txt
  const int64_t t256 = (d.m % 256 == 0 && d.n % 256 == 0) ? (d.m / 256) * (d.n / 256) : 0;
  const int64_t t128 = (d.m % 128 == 0 && d.n % 128 == 0) ? (d.m / 128) * (d.n / 128) : 0;
  auto fill = [](int64_t t) { return (double)t / (double)(((t + 255) / 256) * 256); }; // CU occupancy over the rounds
  if (t256 >= t256_min && 1.4 * fill(t256) >= fill(t128)) return 2;
  if (t128 >= t128_min) return 1;
  return 0;
}

static const int BLW_BM[4] = {BLW_TILES[0].bm(), BLW_TILES[1].bm(), BLW_TILES[2].bm(), BLW_TILES[3].bm()}; // 32, 64, 64, 128
static const int BLW_BN[4] = {BLW_TILES[0].bn(), BLW_TILES[1].bn(), BLW_TILES[2].bn(), BLW_TILES[3].bn()}; // 64, 64, 128, 128
void blw_tile_dims(int tile, int *bm, int *bn) { *bm = BLW_BM[tile & 3], *bn = BLW_BN[tile & 3]; }
static bool blw_divides(const GemmDesc &d, int tile) { return d.m % BLW_BM[tile] == 0 && d.n % BLW_BN[tile] == 0; }

// Mid-size bf16 outputs: the loader-wave family (brgemm_bf16_lw.hip), the largest tile that still gives at least 3/4 of the CUs
// a workgroup (one workgroup per CU: 160 KiB of LDS). Outputs too small for that even with 32x64 tiles stay with the 32x32 K-split
// family (m = 256, n = 1024, K = 1024: 4.9 us against 5.7 on 128 tiles of 32x64, profiles/r03_sweep_shapes.txt).
// Returns the tile index (0 .. 3) or -1.
static int pick_bf16_lw_tile(const GemmDesc &d, int64_t cus) {
  // Gate (unchanged since round 3): some tile of the family gives at least 3/4 of the CUs a workgroup. Which tile, round 6: the
  // cheapest by blw_cost. The old rule - the LARGEST tile that still reaches 3/4 of the CUs - put 1024 x 2560 on 320 tiles of 64x128
  // (two rounds: 15.1 us) instead of 160 tiles of 128x128 (one round: 10.2 us). The batch count arrives with the invoke: priced at 16
  // chunks (K = 1024; the order of two candidates flips with K only when their round counts differ AND the sums are within a few percent).
  bool gate = false;
  int best = -1;
  double best_t = 0;
  for (int t = 3; t >= 0; --t) {
    if (!blw_divides(d, t)) continue;
    const int64_t tiles = (d.m / BLW_BM[t]) * (d.n / BLW_BN[t]);
    if (tiles * 4 >= 3 * cus) gate = true;
    const double cost = blw_cost(t, rounds(tiles, cus), 16.0);
    if (best < 0 || cost < best_t) best = t, best_t = cost;
  }
  return gate ? best : -1;
}
// flat-B / VNNI-4 images: pick_bf16_lw_tile's tile, else the smallest the shape divides; a forced tile if the shape divides it
static int pick_bf16_lw_image_tile(const GemmDesc &d, int64_t cus, int first_variant, int forced_variant) {
  int t = pick_bf16_lw_tile(d, cus);
  for (int c = 0; t < 0 && c < 4; ++c)
    if (blw_divides(d, c)) t = c;
  if (forced_variant >= first_variant && forced_variant <= first_variant + 3 && blw_divides(d, forced_variant - first_variant)) return forced_variant;
  return t >= 0 ? first_variant + t : V_GENERIC;
}

// EDGE TILES, bf16 (xsmm_hip_set_edge_tiles modes 2 and 20 .. 23, opt-in): a whole-layer bf16 call no loader-wave tile divides - m not a
// multiple of 32 or n not of 64: planned on the generic kernel or the 32x32 K-split kernel - on the loader-wave tiles all the same
// (brgemm_bf16_lw.hip GRP = 3, launch_bf16_lw). What the three B images ask of leading dimensions, strides and lane offsets is
// bf16_fast_eligible / bf16_flat_eligible / bf16_vnni4_eligible without their m / n terms; returns the image (0 VNNI-2, 2 flat, 4 VNNI-4), -1 = none.
// ragged_k 1 (xsmm_hip_set_edge_k_bf16): the k % 64 term replaced by brgemm_bf16_lw_kedge.h's bkedge_k_ok; 2 (xsmm_hip_set_edge_k8_bf16): by
// bkedge8_k_ok; 3 (xsmm_hip_set_dma256_edge): by k % 32, the chunk of the 256x256 tile.
static int bf16_edge_b_kind(const GemmDesc &d, int ragged_k = 0) {
  if (d.dtype != DT_BF16 || d.vnni_c || d.k <= 0 ||
      (ragged_k == 3 ? d.k % 32 != 0 : ragged_k == 2 ? !bkedge8_k_ok(d.k) : ragged_k == 1 ? !bkedge_k_ok(d.k) : d.k % BK != 0))
    return -1;
  if ((d.lda | d.ldc | d.stride_a | d.stride_b) & 7 || d.lda >= (1 << 22) || d.ldc >= (1 << 22)) return -1;
  if (d.vnni_b && d.vnni_factor == 2) return !(d.ldb & 3) && d.ldb < (1 << 21) ? 0 : -1;
  if (d.vnni_b && d.vnni_factor == 4) return !(d.ldb & 1) && d.ldb < (1 << 20) ? 4 : -1;
  if (!d.vnni_b) return !(d.ldb & 7) && d.ldb < (1 << 21) ? 2 : -1;
  return -1;
}
// A tile is a candidate when m >= BM and n >= BN. Mode 2: the cheapest candidate by blw_cost - the divisible shapes' fitted model - over
// the rounds of its CEIL-DIVIDED tile count, priced at the call's own chunk count; ties go to the larger tile. Modes 20 .. 23 (tests,
// measurements): that tile. Returns the tile index 0 .. 3, -1 = none. The model is not fitted to ragged shapes: profiles/edge_tiles_bf16_ab.txt.
static int choose_bf16_edge_tile(const GemmDesc &d, int mode, int64_t chunks, int64_t cus) {
  auto tiles = [&](int t) { return (d.m >= BLW_BM[t] && d.n >= BLW_BN[t]) ? ((d.m + BLW_BM[t] - 1) / BLW_BM[t]) * ((d.n + BLW_BN[t] - 1) / BLW_BN[t]) : 0; };
  if (mode >= V_BF16_LW_32x64 && mode <= V_BF16_LW_128x128) return tiles(mode - V_BF16_LW_32x64) > 0 ? mode - V_BF16_LW_32x64 : -1;
  if (mode != 2) return -1;
  int best = -1;
  double best_t = 0;
  for (int t = 3; t >= 0; --t) {
    if (tiles(t) <= 0) continue;
    const double cost = blw_cost(t, rounds(tiles(t), cus), (double)chunks);
    if (best < 0 || cost < best_t) best = t, best_t = cost;
  }
  return best;
}

// EDGE TILES on the 256x256 tile (xsmm_hip_set_dma256_edge mode 1, opt-in; brgemm_bf16_dma256_edge.h): pick_bf16_tile's rule for the 256x256
// tile on CEIL-DIVIDED tile counts - at least 240 tiles of 256x256, and 1.4 x their CU occupancy over the rounds at least that of the
// ceil-divided 128x128 tiles.
// Measured (profiles/dma256_edge_ab.txt: one box, 256 CUs, K = 1024, beta 0 + bias + relu, five alternating rounds, us per call, every switch
// off / xsmm_hip_set_edge_tiles(2) -> this tile):
//   VNNI-2: 4000x4096 154.28 / 152.89 -> 35.03, 4096x4000 214.08 / 45.27 -> 35.96, 5000x5000 412.55 / 85.06 -> 64.76, 8000x8000 350.71 /
//           346.40 -> 135.03, 16000x1024 (63 x 4 tiles) 49.02 / 49.20 -> 38.73
//   flat:   4000x4096 119.10 / 118.32 -> 35.67, 8000x8000 352.75 / 347.39 -> 136.11;  VNNI-4: 119.39 / 118.36 -> 35.51, 344.87 / 342.03 -> 134.27
// each faster in 5 of 5 rounds against both. The gate: 4100x4096, 17 x 16 = 272 tiles - a second round with 16 tiles in it - 164.78 / 52.03
// -> 58.26: slower than the 128x128 edge tile in 5 of 5 rounds. The fill term refuses it as it stands (1.4 * 272 / 512 = 0.74 < 1056 /
// 1280 = 0.83), so no further gate is needed: mode 1 takes every measured row that gained and no other. Not measured: K other than 1024.
static bool dma256_edge_rule(const GemmDesc &d) {
  auto cdiv = [](int64_t x, int64_t t) { return (x + t - 1) / t; };
  const int64_t t256 = cdiv(d.m, 256) * cdiv(d.n, 256), t128 = cdiv(d.m, 128) * cdiv(d.n, 128);
  auto fill = [](int64_t t) { return (double)t / (double)(((t + 255) / 256) * 256); }; // CU occupancy over the rounds
  return t256 >= 240 && 1.4 * fill(t256) >= fill(t128);
}

// SKINNY-BATCH bf16 LAYERS (xsmm_hip_set_skinny_bf16, opt-in; brgemm_bf16_skinny.hip, brgemm_bf16_skinny.h): the column-block width BN of a
// bf16 call with 1 <= m <= 31 and B image `kind` (0 VNNI-2, 2 flat, 4 VNNI-4), or 0: the call stays on the generic kernel. Modes 16 / 32 / 64
// (tests, measurements): that width if its instance exists (not flat with 16: passed over) and n >= BN.
// Mode 1, THE RULE, from profiles/skinny_bf16_ab.txt (one box, 256 CUs, beta 0 + bias + relu, five alternating rounds, us per call, generic
// kernel -> BN 16 / 32 / 64; a BN is taken only where it was faster in EVERY round):
//   The generic kernel has two paths. On its 16-byte path (a VNNI B, k % 32 == 0) it is nearer the stream's bound than expected: 4096 x
//   4096 (B 32 MiB) runs at 2.8 TB/s against 6.29 TB/s for a copy. On its element path (every flat B; k % 32 != 0) it is 8 to 9 times slower.
//   m <= 16, 16-byte path: VNNI-2 4096x4096 m 1 / 8 / 16: 11.34 / 12.02 / 12.15 -> BN 32 9.19 / 10.55 / 10.88 (BN 16 slower in every round:
//     64-byte row pieces split every 128-byte line of B between two workgroups; BN 64 ahead by 1 .. 11 %); VNNI-4 m 8: 11.78 -> BN 16 8.35
//     (BN 32 10.03). 1024x1024 (n x K; B 2 MiB) 4.75 / 5.02 / 5.13 -> BN 16 4.51 / 4.49 / 4.80, 4096x1024 (8 MiB) 4.60 / 4.97 / 4.98 -> 3.92 /
//     4.31 / 4.59, 1024x4096 (8 MiB) 10.33 / 10.67 / 10.72 -> 5.71 / 6.75 / 7.72; BN 32 and 64 lose or win less on all three.
//     So: a B of at least 16 MiB runs on the BN whose row piece is one 128-byte line (VNNI-2 32, VNNI-4 16, flat 64), a smaller one on the
//     smallest BN with an instance (16; flat 32) - more workgroups pulling bytes. (Between 8 and 32 MiB nothing was measured.)
//   m >= 17 (two accumulator sets), 16-byte path: slower on EVERY BN in every round - 1024x1024 5.00 -> 5.72 / 7.01 / 8.38, 4096x4096 12.41
//     -> 14.31 / 15.10 / 16.65, 4096x1024 5.07 -> 5.96, 1024x4096 10.78 -> 11.36: every workgroup re-reads its 32 rows of A, as many bytes
//     as its B block on BN 32. THE GATE: such a call stays on the generic kernel.
//   The element path, every m: 1000x1000 (k = 1000) m 1 / 8 / 16 / 31: 34.82 / 35.04 / 37.31 / 41.49 -> BN 16 4.63 / 4.17 / 4.20 / 5.05; flat
//     4096x4096 m 8: 136.39 -> BN 64 14.87 (BN 32 15.28). Taken, on the BN of the size rule above.
// Not measured: other CU counts (the rule does not read them), several ranks, beta 1, a flat or VNNI-4 B off the rows named here.
// BN depends on n, k, br and the mode; the waves of a workgroup on br and k alone (skn_waves).
constexpr int64_t SKINNY_LINE_BYTES = 16 << 20; // a B of at least this many bytes: the BN of one 128-byte line per row piece
static int skinny_bf16_bn(const GemmDesc &d, int kind, int mode, int64_t br, bool ab16) {
  if (mode == 16 || mode == 32 || mode == 64) return skn_instance_exists(kind, mode) && d.n >= mode ? mode : 0;
  if (mode != 1) return 0;
  const GenericOk g = generic_ok(d, ab16);
  if ((g.vec16 || g.vec16_4) && d.m > 16) return 0; // the gate
  const int smallest = kind == 2 ? 32 : 16, line = 64 / skn_vfac(kind);
  int bn = 2 * br * d.k * d.n >= SKINNY_LINE_BYTES ? line : smallest;
  while (bn > smallest && d.n < bn) bn /= 2;
  return d.n >= bn ? bn : 0;
}

// K SPLIT ACROSS WORKGROUPS OF A SKINNY-BATCH LAUNCH (xsmm_hip_set_skinny_split, opt-in; brgemm_bf16_skinny_split.hip,
// brgemm_bf16_skinny_split.h): the parts P_eff of a call already on the skinny kernel with column blocks of bn, or 1: the plain skinny
// launch. Modes 2 .. 16 (tests, measurements): P = the mode. Reads the descriptor, the batch count and the CU count only.
// Mode 1, THE RULE, from profiles/skinny_split_ab.txt (one box, 256 CUs, beta 0 + bias + relu, five alternating rounds, us per call, the
// UNSPLIT skinny launch of the same BN -> P = 2 / 4 / 8 / 16; a P is taken only where it was faster in EVERY round). This replaces the
// provisional rule min(SPLIT_MAX, cus / blocks, S_all / 8), which took P 4 on 1024 x 1024 (n x K), 1000 x 1000 and 1024 x 4096 and lost there.
//   The hand-off costs about 1 us at P 2 and 2 us at P 4 on a call of 4 us, and grows with P: 1024 x 1024 m 1 on BN 16 3.91 -> 4.91 / 5.92 /
//   7.78 / 11.95. It pays only where a workgroup of the unsplit launch streams long enough to hide it. What decides is the bytes of B per
//   workgroup, 2 BN br k:
//   256 KiB and more, EVERY row, image and m (1, 8, 16, 31) gains in every round: 4096 x 4096 VNNI-2 BN 32 (128 blocks) m 1 / 8 / 16 / 31 9.07 /
//     10.53 / 10.90 / 15.09 -> P 2 8.17 / 9.22 / 9.33 / 12.29 (P 4 8.47 / 9.61 / 10.05 / 13.28); BN 64 (64 blocks, 512 KiB) 10.00 / 11.70 / 11.94 /
//     16.54 -> P 4 8.30 / 9.70 / 9.72 / 12.64 (P 2 less, P 8 level or slower); flat m 8 BN 64 14.77 -> P 4 10.40 (P 2 11.80), BN 32 15.23 -> P 2
//     14.62; VNNI-4 m 8 BN 32 10.00 -> P 2 9.06, BN 64 11.64 -> P 4 9.74; 1024 x 4096 BN 32 (32 blocks) m 1 / 8 / 16 / 31 7.46 / 9.20 / 10.33 / 14.69 ->
//     P 2 6.81 / 7.99 / 8.48 / 11.40, BN 64 (16 blocks) 8.16 / 9.98 / 11.01 / 15.99 -> P 4 6.99 / 8.33 / 8.44 / 11.22.
//   128 KiB: mixed - 1024 x 4096 BN 16 (64 blocks) m 1 / 8 / 16 5.74 / 6.65 / 7.68 -> P 2 6.02 / 6.61 / 7.02, P 4 6.52 / 7.01 / 7.17 (m 1 loses in
//     every round); 4096 x 4096 BN 16 (256 blocks) and VNNI-4 BN 16 8.32 -> 9.44 lose; every BN 64 row of K = 1024 loses. Not taken.
//   Less (1024 x 1024, 4096 x 1024, 1000 x 1000 on every BN): every P loses in every round, by 5 .. 50 % at P 2. Not taken.
//   P 8 gains less than P 4 wherever both gain, P 16 loses on every row but 1024 x 4096 m 31.
// So: P = 4, else 2, where the parts fit the compute units in one round (blocks * P <= cus) and a part keeps at least 128 KiB of B
// (2 BN br k >= P * 128 KiB); else the plain launch. On every measured (row, BN) this takes, that P was faster in every round, and it takes
// nothing else. With mode 1 of the skinny switch (which picks BN) it splits 4096 x 4096: VNNI-2 BN 32 P 2, flat BN 64 P 4; VNNI-4 stays on BN 16
// unsplit (8.32, the fastest side of its row). Not measured: other CU counts (the rule reads them only through blocks * P <= cus), several
// ranks, beta 1, other grid orders, K beyond 4096.
constexpr int64_t SKINNY_PART_BYTES = 128 << 10; // a part streams at least this many bytes of B
static int skinny_split_parts(const GemmDesc &d, int bn, int mode, int64_t br, int64_t cus) {
  const int64_t s_all = br * skn_steps((int)d.k), blocks = skn_blocks((int)d.n, bn);
  int P = mode;
  if (mode == 1) {
    P = 1;
    for (int c : {4, 2})
      if (P == 1 && blocks * c <= cus && 2 * bn * br * d.k >= c * SKINNY_PART_BYTES) P = c;
  }
  if (P < 2 || P > SKS_PMAX) return 1;
  const int p_eff = sks_parts(P, s_all);
  return p_eff >= 2 ? p_eff : 1;
}

// RAGGED k, bf16 (xsmm_hip_set_edge_k_bf16, opt-in; brgemm_bf16_lw_kedge.h): a whole-layer bf16 call whose k is a multiple of 16 but not of
// 64 (k >= 64) - planned on the generic or the 32x32 K-split kernel whatever its m and n - on a loader-wave tile (brgemm_bf16_lw.hip
// GRP = 4, launch_bf16_lw). The tile: `forced` (0 .. 3) if there is one, else the cheapest candidate by blw_cost over the rounds of its
// ceil-divided tile count, priced at br * ceil(k / 64) chunks; ties go to the larger tile. A candidate fits (m >= BM, n >= BN) and - unless
// a bf16 edge-tile mode is on as well (edge_on: the kernel then shifts back its last tile row / column too) - divides m and n.
// Returns the tile index 0 .. 3, -1 = none: the call stays where it is. Not fitted to ragged shapes: profiles/edge_k_bf16_ab.txt.
static int choose_bf16_kedge_tile(const GemmDesc &d, int forced, bool edge_on, int64_t chunks, int64_t cus) {
  auto tiles = [&](int t) -> int64_t {
    if (d.m < BLW_BM[t] || d.n < BLW_BN[t]) return 0;
    if (!edge_on && (d.m % BLW_BM[t] != 0 || d.n % BLW_BN[t] != 0)) return 0;
    return ((d.m + BLW_BM[t] - 1) / BLW_BM[t]) * ((d.n + BLW_BN[t] - 1) / BLW_BN[t]);
  };
  if (forced >= 0) return forced <= 3 && tiles(forced) > 0 ? forced : -1;
  int best = -1;
  double best_t = 0;
  for (int t = 3; t >= 0; --t) {
    if (tiles(t) <= 0) continue;
    const double cost = blw_cost(t, rounds(tiles(t), cus), (double)chunks);
    if (best < 0 || cost < best_t) best = t, best_t = cost;
  }
  return best;
}

static const char *variant_name(int v) {
  static const char *const names[32] = {
      "brgemm_f32_fast<64x64,k1>", "brgemm_f32_fast<64x32,k2>", "brgemm_f32_fast<32x32,k4>", "brgemm_f32_fast<128x64,k1>",
      "brgemm_f32_fast<64x64,k2>", "brgemm_f32_fast_lw<64x64,k1>", "brgemm_f32_fast_lw<64x64,k2>", "brgemm_f32_fast_lw<64x32,k4>",
      "brgemm_grouped(generic)", "brgemm_f32_fast_lw<32x32,k4>", "brgemm_f32_fast_lw<128x64,k1>", "brgemm_f32_lw16<32x16,k4>",
      "brgemm_f32_bf16x6<64x64,k1>", "brgemm_f32_bf16x6<64x32,k2>", "brgemm_f32_bf16x6<32x32,k4>", "brgemm_f32_bf16x6<128x64,k1>",
      "brgemm_bf16_fast<64x64>", "brgemm_bf16_dma<128x128>", "brgemm_bf16_dma<256x256>", "brgemm_bf16_small<32x32,k4>",
      "brgemm_bf16_lw<32x64,k2>", "brgemm_bf16_lw<64x64>", "brgemm_bf16_lw<64x128>", "brgemm_bf16_lw<128x128>",
      "brgemm_bf16_lw_flatb<32x64,k2>", "brgemm_bf16_lw_flatb<64x64>", "brgemm_bf16_lw_flatb<64x128>", "brgemm_bf16_lw_flatb<128x128>",
      "brgemm_bf16_lw_vnni4<32x64,k2>", "brgemm_bf16_lw_vnni4<64x64>", "brgemm_bf16_lw_vnni4<64x128>", "brgemm_bf16_lw_vnni4<128x128>"};
  return v >= 0 && v < 32 ? names[v] : names[V_GENERIC];
}

// split tiles the planner picks by itself for a bf16x6 descriptor (64x64, 64x32 + K2, 32x32 + K4, 128x64): the ones that beat the exact
// kernel of the same tile. None does yet (profiles/x6_first_ab.txt, kernel averages bf16x6 / exact: first version 1.25 - 4.36; with
// loader waves doing the split 1.29 - 3.99, e.g. 4096^3 1312.54 against 1015.14 us, 1024x2560x1024 103.87 against 57.49 us): a
// bf16x6 descriptor stays on the exact plan of mode 0 unless a split tile is forced (xsmm_hip_force_variant 12 .. 15).
static const bool X6_AUTO[4] = {false, false, false, false};
// output tiles of the f32 variants 0 .. 10 (8: the generic kernel, no tile)
static const int F32_BM[11] = {64, 64, 32, 128, 64, 64, 64, 64, 0, 32, 128}, F32_BN[11] = {64, 32, 32, 64, 64, 64, 64, 32, 0, 32, 64};

bool plan_gemm(GemmDesc &d, int forced_variant, const GemmPlanEnv &env) {
  const int64_t cus = env.cus;
  int v = V_GENERIC;
  if (d.vnni_c) forced_variant = V_GENERIC; // VNNI-2 C store: the generic kernel's epilogue only
  if (d.dtype == DT_F32 && !d.vnni_b) v = pick_f32_variant(d, cus);
  else if (d.dtype == DT_BF16 && d.vnni_b && d.vnni_factor == 4) {
    // VNNI-4 B ([k/4][n][4]: benchmarks/config/omp/mlir-bf16.json:68-100 `--vnni=4`): the loader-wave tiles with the VNNI-4 image;
    // everything else - ragged shapes, k not a multiple of 64 (the compiler-native 32x32x32 tiles) - on the generic kernel's element path
    if (bf16_vnni4_eligible(d)) v = pick_bf16_lw_image_tile(d, cus, V_BF16_LW4_32x64, forced_variant);
  } else if (d.dtype == DT_BF16 && bf16_fast_eligible(d)) {
    v = V_BF16_FAST + pick_bf16_tile(d);
    // small outputs (e.g. the reference's --batch=256 layers): 32x32 tiles with K split over the waves give
    // every CU a workgroup. Measured crossover with the 64x64 family (n = 1024, K = 1024): 5.1 vs 8.4 us at 64
    // tiles of 64x64, 7.5 vs 8.5 at 128, 12.3 vs 8.9 at 256 (profiles/r01_sweep_shapes.txt)
    if (v == V_BF16_FAST && bf16_small_eligible(d) && (d.m / 64) * (d.n / 64) < (3 * cus) / 4) v = V_BF16_SMALL32;
    // mid-size outputs (the 64x64 / 32x32 families, or 128x128 tiles for fewer than 3/4 of the CUs): one loader-wave workgroup
    // per CU. Measured (profiles/r03_sweep_shapes.txt, 1024-wide layer, K = 1024): see DESIGN.md 4.2.
    const int64_t t128 = (d.m / 128) * (d.n / 128);
    if (v == V_BF16_FAST || v == V_BF16_SMALL32 || (v == V_BF16_DMA128 && t128 * 4 < 3 * cus)) {
      const int lw = pick_bf16_lw_tile(d, cus);
      // (round 6: the 128x128 loader-wave tile also where brgemm_bf16_dma128 used to stay - fewer than 3/4 of the CUs busy: 1024 x 2560 x
      // 1024 = 160 tiles runs 10.2 us on it against 11.5 on dma128, profiles/r06_bf16_sweep_before.txt)
      if (lw >= 0) v = V_BF16_LW_32x64 + lw;
    } else if (v == V_BF16_DMA128 && t128 <= cus && pick_bf16_lw_tile(d, cus) == 3) {
      // ONE round of 128x128 tiles (the C4 layer 4096 x 1024, C5 2048 x 2048): since the end of round 3 the loader-wave tile is
      // at least as fast as brgemm_bf16_dma128 there (same box, profiles/r03_write_through_c_stores.txt: C5 18.2 against 18.7 us,
      // the C4 layer 10.4 against 10.6-11.5) - and it is the tile the 4096-row chain runs on. Several rounds: dma128 (not re-measured).
      v = V_BF16_LW_128x128;
    }
    const int tile = forced_variant - V_BF16_FAST; // a forced bf16 tile is honoured if the shape divides it
    if (tile >= 0 && tile <= 2 && d.m % (64 << tile) == 0 && d.n % (64 << tile) == 0) v = forced_variant;
    if (forced_variant == V_BF16_SMALL32 && bf16_small_eligible(d)) v = forced_variant;
    if (forced_variant >= V_BF16_LW_32x64 && forced_variant <= V_BF16_LW_128x128 && blw_divides(d, forced_variant - V_BF16_LW_32x64)) v = forced_variant;
  } else if (d.dtype == DT_BF16 && bf16_flat_eligible(d)) {
    // flat B ([k][n] row-major, what xsmm.unary pack would have turned into VNNI-2): the loader-wave tiles with the interleave
    // in the B loader (launch_gemm falls back to the generic kernel when an operand is not 16-byte aligned).
    v = pick_bf16_lw_image_tile(d, cus, V_BF16_LWF_32x64, forced_variant);
  } else if (d.dtype == DT_BF16 && bf16_small_eligible(d)) {
    v = V_BF16_SMALL32; // k a multiple of 16 only (e.g. the compiler-native 32x32x32 tile), m or n a multiple of 32 only
    if (forced_variant == V_BF16_LW_32x64) { // the 32x64 loader-wave tile needs m % 32 only (bf16_fast_eligible asks for 64)
      GemmDesc e = d;
      e.m = (d.m + 63) / 64 * 64;
      if (d.m % 32 == 0 && d.n % 64 == 0 && bf16_fast_eligible(e)) v = forced_variant;
    }
  }
  if (forced_variant >= 0 && d.dtype == DT_F32 && v != V_GENERIC) {
    // honour the forced tile only if the shape divides it
    if (forced_variant <= V_F32_LW_128x64 && forced_variant != V_GENERIC && d.m % F32_BM[forced_variant] == 0 && d.n % F32_BN[forced_variant] == 0)
      v = forced_variant;
    if (forced_variant == V_F32_LW16_32x16 && d.m % 32 == 0 && d.n % 16 == 0 && d.ldc % 4 == 0) v = forced_variant;
    if (forced_variant == V_GENERIC) v = V_GENERIC;
  } else if (forced_variant == V_GENERIC) {
    v = V_GENERIC;
  }
  if (d.f32_prec == 6 && d.dtype == DT_F32 && !d.vnni_b && !d.vnni_c && f32_x6_eligible(d)) {
    // bf16x6: the split kernel needs 64-k chunks, 16-byte row pieces, the 32-bit lane offsets and ldc a multiple of 4.
    // It takes the output tile of the exact plan where the split tile of that size measured faster than the exact kernel (X6_AUTO: none
    // yet); the skinny 32x16 tiles, the generic kernel and forced exact variants stay exact. A forced split tile (xsmm_hip_force_variant
    // 12 .. 15) is honoured if the shape divides it.
    const int fx = forced_variant - V_F32_X6_64x64;
    if (fx >= 0 && fx <= 3) {
      if (d.m % F32_BM[fx] == 0 && d.n % F32_BN[fx] == 0) v = forced_variant; // (split tile fx has the shape of exact variant fx)
    } else if (forced_variant < 0) { // (the split tile of the exact plan's size: 64x64, 64x32, 32x32, 128x64)
      static const int x6_tile[11] = {0, 1, 2, 3, 0, 0, 0, 1, -1, 2, 3};
      const int t = v <= V_F32_LW_128x64 ? x6_tile[v] : -1;
      if (t >= 0 && X6_AUTO[t]) v = V_F32_X6_64x64 + t;
    }
  }
  d.variant = v;
  d.generic_forced = forced_variant == V_GENERIC;
  d.variant_forced = forced_variant >= 0 && v == forced_variant;
  strncpy(d.name, variant_name(v), sizeof(d.name) - 1);
  d.name[sizeof(d.name) - 1] = 0;
  return true;
}

// the f32 chain tile (brgemm_f32_lw.hip, launch_f32_chain) a whole-layer f32 descriptor was planned on: 1 / 2, or -1 (another
// kernel family, a VNNI operand, k not in 64-k chunks ... - whatever pick_f32_variant sent elsewhere)
int f32_chain_tile(const GemmDesc &d) {
  if (gemm_on_x6(d)) return -1; // the bf16x6 split kernel: chains that hold such a call run call by call (it has no chain form)
  if (d.dtype != DT_F32 || d.vnni_b || d.vnni_c || d.k <= 0 || d.k % BK) return -1;
  // (the 32x32 + K4 tile - the reference's batch-256 layers, 3.4 us of MFMA work per tile - is NOT chained: measured 21.9 us per
  // three-layer step as one launch against 20.6 as three, profiles/r04_f32_chain.txt: a seam is four dependent memory round trips
  // - store drain, counter add, poll, A fetch - and 32 producers + 32 pollers share one counter line; the 64-row tiles gain 1-2.5 %)
  return d.variant == V_F32_LW_64x64K2 ? 1 : d.variant == V_F32_LW_64x32K2 ? 2 : -1;
}
bool f32_chain_tile_dims(int tile, int *bm, int *bn) { return (tile == 1 || tile == 2) && (*bm = 64, *bn = tile == 1 ? 64 : 32, true); }

int bf16_lw_b_kind(const GemmDesc &d) {
  if (d.dtype != DT_BF16 || d.vnni_c) return -1;
  if (d.vnni_b && d.vnni_factor == 4) return bf16_vnni4_eligible(d) ? 4 : -1;
  if (d.vnni_b) return bf16_fast_eligible(d) ? 0 : -1;
  return bf16_flat_eligible(d) ? 2 : -1;
}

int chain_edge_b_kind(const GemmDesc &d, int chain_edge, const char **why) {
  const char *w = nullptr;
  int kind = -1;
  if (!chain_edge) w = "ragged chains are off (xsmm_hip_set_chain_edge)";
  else if (d.dtype != DT_BF16) w = "a ragged chain is bf16: an f32 call";
  else if (d.vnni_c || !d.beta0) w = "a call of a ragged chain stores a VNNI C or is not beta 0";
  else if (d.generic_forced || d.variant_forced) w = "a call of a ragged chain was dispatched to a forced kernel";
  else if ((kind = bf16_edge_b_kind(d)) < 0) w = "a call of a ragged chain has k not in 64-k chunks or an operand off the grid of the LDS-DMA tiles";
  if (why) *why = w;
  return w ? -1 : kind;
}

ChainEdgePlan plan_chain_edge(int64_t m, int64_t n, int nlayers, const int64_t *k, const int64_t *br, int64_t cus, int forced_tile, bool strict) {
  if (strict) return ChainEdgePlan{-1, "strict mode: the tile of a ragged chain is not a function of the descriptor alone"};
  if (nlayers < 2 || nlayers > 8) return ChainEdgePlan{-1, "fewer than 2 or more than 8 calls"};
  for (int l = 0; l < nlayers; ++l)
    if (k[l] < BK || k[l] % BK != 0 || br[l] < 1) return ChainEdgePlan{-1, "a layer of a ragged chain has k not in 64-k chunks, or an empty batch"};
  auto fits = [&](int t) { return t >= 0 && t <= 3 && m >= BLW_BM[t] && n % BLW_BN[t] == 0 && ((m + BLW_BM[t] - 1) / BLW_BM[t]) * (n / BLW_BN[t]) <= cus; };
  int tile = fits(forced_tile) ? forced_tile : -1;
  for (int t = 0; t < 4 && tile < 0; ++t)
    if (fits(t)) tile = t;
  if (tile < 0) {
    if (m < BLW_BM[0]) return ChainEdgePlan{-1, "a ragged chain's m is below every tile's rows"};
    if (n % BLW_BN[0] != 0) return ChainEdgePlan{-1, "a ragged chain's n is not in whole column tiles"};
    return ChainEdgePlan{-1, "more tiles than compute units"};
  }
  if (m % BLW_BM[tile] == 0) return ChainEdgePlan{-1, "the tile's rows divide m: not a ragged chain"};
  return ChainEdgePlan{tile, ""};
}

int chain_ragged_b_kind(const GemmDesc &d, int chain_ragged, const char **why) {
  const char *w = nullptr;
  int kind = -1;
  if (!chain_ragged) w = "ragged-width chains are off (xsmm_hip_set_chain_ragged)";
  else if (d.dtype != DT_BF16) w = "a ragged-width chain is bf16: an f32 call";
  else if (d.vnni_c || !d.beta0) w = "a call of a ragged-width chain stores a VNNI C or is not beta 0";
  else if (d.generic_forced || d.variant_forced) w = "a call of a ragged-width chain was dispatched to a forced kernel";
  else if (!chain_ragged_k_ok(d.k)) w = "a call of a ragged-width chain has k below 64 or not a multiple of 8";
  else {
    GemmDesc e = d; // bf16_edge_b_kind's terms for leading dimensions, strides and lane offsets; its k term is the one above
    e.k = BK;
    if ((kind = bf16_edge_b_kind(e)) < 0) w = "a call of a ragged-width chain has an operand off the grid of the LDS-DMA tiles";
  }
  if (why) *why = w;
  return w ? -1 : kind;
}

ChainRaggedPlan plan_chain_ragged(int64_t m, int64_t n, int nlayers, const int64_t *k, const int64_t *br, int64_t cus, int forced_tile, int b_kind, int mode, bool strict) {
  if (mode != 1) return ChainRaggedPlan{-1, "ragged-width chains are off (xsmm_hip_set_chain_ragged)"};
  if (strict) return ChainRaggedPlan{-1, "strict mode: the tile of a ragged-width chain is not a function of the descriptor alone"};
  if (nlayers < 2 || nlayers > 8) return ChainRaggedPlan{-1, "fewer than 2 or more than 8 calls"};
  bool k_ragged = false;
  for (int l = 0; l < nlayers; ++l) {
    if (!chain_ragged_k_ok(k[l]) || br[l] < 1) return ChainRaggedPlan{-1, "a layer of a ragged-width chain has k below 64 or not a multiple of 8, or an empty batch"};
    if (k[l] % BK != 0) k_ragged = true;
  }
  if (n % 8 != 0) return ChainRaggedPlan{-1, "a ragged-width chain's n is not a multiple of 8"};
  auto tiles = [&](int t) { return ((m + BLW_BM[t] - 1) / BLW_BM[t]) * ((n + BLW_BN[t] - 1) / BLW_BN[t]); };
  auto fits = [&](int t) { return t >= 0 && t <= 3 && blw_chain_ragged_instance_exists(t, b_kind) && m >= BLW_BM[t] && n >= BLW_BN[t] && tiles(t) <= cus; };
  int tile = fits(forced_tile) ? forced_tile : -1;
  const bool forced = forced_tile >= 0 && forced_tile <= 3; // (tests and measurements: under a forcing edge-tile mode nothing is gated, whichever tile fits)
  for (int t = 0; t < 4 && tile < 0; ++t)
    if (fits(t)) tile = t;
  if (tile >= 0 && !k_ragged && n % BLW_BN[tile] == 0) return ChainRaggedPlan{-1, "the tile's columns divide n and every k is in 64-k chunks: not a ragged-width chain"};
  // THE GATE (measured, profiles/chain_ragged_ab.txt: 2000 rows of three 1000-wide VNNI-2 layers on 256 CUs, call by call 30.98 -> one
  // launch 35.07 us): a chain whose tile by the rule would be 64x128 - it fits, no smaller tile does - but whose B image has no instance
  // of that tile (VNNI-2: it would need scratch) lands on 128x128 with half the workgroups, while its separate calls run on 64x128. It
  // stays call by call. Not under a forcing edge-tile mode.
  if (!forced && tile == 3 && !blw_chain_ragged_instance_exists(2, b_kind) && blw_b_kind_ok(b_kind) && m >= BLW_BM[2] && n >= BLW_BN[2] && tiles(2) <= cus)
    return ChainRaggedPlan{-1, "gate: the rule's 64x128 tile has no instance for this B image and 128x128 in its place measured slower than call by call (profiles/chain_ragged_ab.txt)"};
  // THE SECOND GATE (same file: 1024 rows x [1024, 1000, 1000], layer 0 sixteen batch elements of 64, call by call 14.37 -> one launch 14.87 us,
  // every pair slower): a whole-k layer with an even chunk count runs as a single call with TWO chunks per barrier on the 32x64 and 64x64
  // tiles (blw_tile_sup2), this mode has one chunk per barrier only. A chain with such a layer on such a tile stays call by call.
  if (!forced && tile >= 0 && blw_tile_sup2(tile))
    for (int l = 0; l < nlayers; ++l)
      if (k[l] % BK == 0 && ((br[l] * (k[l] / BK)) & 1) == 0)
        return ChainRaggedPlan{-1, "gate: a whole-k layer that runs two chunks per barrier as a single call measured slower in a ragged-width chain (profiles/chain_ragged_ab.txt)"};
  if (tile < 0) {
    if (!blw_b_kind_ok(b_kind)) return ChainRaggedPlan{-1, "the calls of a ragged-width chain do not share one B image"};
    if (m < BLW_BM[0] || n < BLW_BN[0]) return ChainRaggedPlan{-1, "a ragged-width chain's m or n is below every tile"};
    return ChainRaggedPlan{-1, "more tiles than compute units (a ragged-width chain runs in one round)"};
  }
  return ChainRaggedPlan{tile, ""};
}

int chain_rounds_planned_tile(int n, const GemmDesc *const *d) {
  for (int i = 0; i < n; ++i)
    if (d[i]->dtype != DT_BF16) return -2;
  if (n < 1) return -1;
  const int v = d[0]->variant;
  const int t = v >= V_BF16_LW4_32x64 ? v - V_BF16_LW4_32x64 : v >= V_BF16_LWF_32x64 ? v - V_BF16_LWF_32x64 : v - V_BF16_LW_32x64;
  if (t < 0 || t > 3) return -1;
  for (int i = 1; i < n; ++i)
    if (d[i]->variant != d[0]->variant) return -1;
  return t;
}

ChainWidthsPlan plan_chain_widths(int64_t m, int nlayers, const int64_t *n, const int64_t *k, const int64_t *br, int64_t cus, int planned_tile, int b_kind, int mode, bool strict) {
  auto no = [](const char *why) { return ChainWidthsPlan{-1, why}; };
  if (mode != 1) return no("mixed-width chains are off (xsmm_hip_set_chain_widths)");
  if (planned_tile < -1) return no("a mixed-width chain is bf16: an f32 call");
  if (nlayers < 2 || nlayers > 8) return no("fewer than 2 or more than 8 calls");
  if (!blw_b_kind_ok(b_kind)) return no("the calls of a mixed-width chain do not share one B image of the loader-wave tiles");
  bool differ = false;
  int64_t widest = 0;
  for (int l = 0; l < nlayers; ++l) {
    if (k[l] < BK || k[l] % BK != 0 || br[l] < 1) return no("a layer of a mixed-width chain has k not in 64-k chunks, or an empty batch");
    if (n[l] != n[0]) differ = true;
    if (n[l] > widest) widest = n[l];
  }
  if (!differ) return no("every call has the same n: not a mixed-width chain");
  auto divides = [&](int t) {
    if (t < 0 || t > 3 || m < BLW_BM[t] || m % BLW_BM[t] != 0) return false;
    for (int l = 0; l < nlayers; ++l)
      if (n[l] < BLW_BN[t] || n[l] % BLW_BN[t] != 0) return false;
    return true;
  };
  auto fits = [&](int t) { return divides(t) && blw_chain_widths_instance_exists(t, b_kind, 1) && (m / BLW_BM[t]) * (widest / BLW_BN[t]) <= cus; };
  if (fits(planned_tile)) return ChainWidthsPlan{planned_tile, ""};
  if (strict) return no("strict mode: one launch only on the tile all calls were dispatched on");
  // THE GATE (measured, profiles/chain_widths_ab.txt: VNNI-2 on 256 CUs, call by call -> one launch, every pair slower: 1024 rows x [1024,
  // 4096, 1024] 29.17 -> 38.39 us on 128x128, 256 rows of the same 16.86 -> 19.82 on 64x64, 2048 rows x [1024, 2048, 1024] 25.58 -> 26.56
  // on 128x128, 1024 rows x [1024, 2048, 1024, 2048, 1024] 35.40 -> 38.60 on 64x128; the funnel [1024, 512, 256, 128], whose launch
  // runs on the smallest tile, 16.39 -> 11.80): the widest layer decides the launch's tile, and a layer that ALONE fits a smaller one -
  // its separate call covers the chip with more, smaller tiles, in the launch it keeps a fraction of the grid busy on the large one -
  // makes the chain slower. Such a chain stays call by call. A tile all calls were dispatched on (above) is not gated: the separate
  // calls run on that tile too.
  auto alone_fits = [&](int t, int l) {
    return blw_chain_widths_instance_exists(t, b_kind, 1) && m >= BLW_BM[t] && m % BLW_BM[t] == 0 && n[l] >= BLW_BN[t] && n[l] % BLW_BN[t] == 0 &&
           (m / BLW_BM[t]) * (n[l] / BLW_BN[t]) <= cus;
  };
  for (int t = 0; t < 4; ++t) {
    if (!fits(t)) continue;
    for (int l = 0; l < nlayers; ++l)
      for (int s = 0; s < t; ++s)
        if (alone_fits(s, l)) return no("gate: a layer fits a smaller tile alone than the widest layer leaves the launch - measured slower as one launch (profiles/chain_widths_ab.txt)");
    return ChainWidthsPlan{t, ""};
  }
  for (int t = 0; t < 4; ++t)
    if (divides(t)) return no("more tiles than compute units (a mixed-width chain runs in one round)");
  return no("no tile divides m and every n (a ragged shape stays call by call with different widths)");
}

ChainWidthRoundsPlan plan_chain_width_rounds(int64_t m, int nlayers, const int64_t *n, const int64_t *k, const int64_t *br, int64_t cus, int planned_tile, int b_kind, int mode, bool strict) {
  auto no = [](const char *why) { return ChainWidthRoundsPlan{-1, 0, why, false}; };
  const bool forced = chain_width_rounds_mode_forced(mode);
  if (mode != 1 && !forced) return no("column rounds of mixed-width chains are off (xsmm_hip_set_chain_width_rounds)");
  if (planned_tile < -1) return no("a mixed-width chain is bf16: an f32 call");
  if (nlayers < 2 || nlayers > 8) return no("fewer than 2 or more than 8 calls");
  if (!blw_b_kind_ok(b_kind)) return no("the calls of a mixed-width chain do not share one B image of the loader-wave tiles");
  bool differ = false;
  int64_t widest = 0;
  for (int l = 0; l < nlayers; ++l) {
    if (k[l] < BK || k[l] % BK != 0) return no("a layer of a mixed-width chain has k not in 64-k chunks");
    if (br[l] < 1) return no("a layer of a mixed-width chain has an empty batch");
    if (n[l] != n[0]) differ = true;
    if (n[l] > widest) widest = n[l];
  }
  if (!differ) return no("every call has the same n: not a mixed-width chain");
  auto divides = [&](int t) {
    if (t < 0 || t > 3 || m < BLW_BM[t] || m % BLW_BM[t] != 0 || m / BLW_BM[t] > 0x7fffffff) return false;
    for (int l = 0; l < nlayers; ++l)
      if (n[l] < BLW_BN[t] || n[l] % BLW_BN[t] != 0 || n[l] / BLW_BN[t] > 0x7fffffff) return false;
    return true;
  };
  auto max_t = [&](int t) { return (int)(widest / BLW_BN[t]); };
  auto fits = [&](int t, int64_t w) {
    return divides(t) && blw_chain_wrounds_instance_exists(t, b_kind) && w >= 1 && w < max_t(t) && (m / BLW_BM[t]) * w <= cus;
  };
  // the rule's W of a tile that divides: as few rounds of the widest layer as fit, balanced (0: none fits)
  auto balanced = [&](int t) {
    const int wfit = chain_wrounds_max_groups(max_t(t), (int)(m / BLW_BM[t]), cus);
    return wfit < 1 ? 0 : chain_wrounds_groups(max_t(t), wfit);
  };
  if (planned_tile < 0 && strict) return no("strict mode: the calls of a mixed-width chain do not share one planned loader-wave tile");
  if (forced) {
    const int64_t w = mode - 1000;
    int tile = -1;
    if (planned_tile >= 0) tile = fits(planned_tile, w) ? planned_tile : -1;
    else
      for (int t = 0; t < 4 && tile < 0; ++t)
        if (fits(t, w)) tile = t;
    if (tile < 0) return no("the forced column groups do not fit: whole tiles, 1 <= W < max_l(n_l / BN) and m / BM * W <= compute units");
    return ChainWidthRoundsPlan{tile, (int)w, "", false};
  }
  int tile = -1;
  if (planned_tile >= 0 && divides(planned_tile) && fits(planned_tile, balanced(planned_tile))) tile = planned_tile;
  const bool planned = tile >= 0;
  if (tile < 0 && strict) return no("strict mode: column rounds only on the tile all calls were dispatched on");
  if (tile < 0) {
    // the K-loop time by the fitted per-chunk rates: sum_l rounds(l) * BLW_B[tile] * br_l * k_l / 64; ties go to the larger tile
    double best = 0;
    for (int t = 0; t < 4; ++t) {
      if (!divides(t) || !fits(t, balanced(t))) continue;
      const int w = balanced(t);
      double cost = 0;
      for (int l = 0; l < nlayers; ++l) cost += (double)chain_wrounds_rounds((int)(n[l] / BLW_BN[t]), w) * BLW_B[t] * (double)br[l] * (double)(k[l] / BK);
      if (tile < 0 || cost <= best) tile = t, best = cost;
    }
  }
  if (tile < 0) {
    bool any = false, rows = false;
    for (int t = 0; t < 4; ++t)
      if (divides(t)) {
        any = true;
        if (m / BLW_BM[t] <= cus) rows = true;
      }
    if (!any) return no("no tile divides m and every n (a ragged shape stays call by call with different widths)");
    if (!rows) return no("more row blocks than compute units: not one column of workgroups fits");
    return no("nothing to round: no W below the widest layer's column tiles fits");
  }
  const int w = balanced(tile);
  // THE GATE (measured, profiles/chain_width_rounds_ab.txt; the rows are quoted in gemm_plan.h): on a tile of the rule's own choice no chain
  // gained - 1024-4096-1024 at 256, 1024, 2048 and 4096 rows ran +28 %, +33 %, +9 % and +7 %, the funnel +2 % in one session and -4 % in
  // the next -, on a tile all calls were dispatched on the launch gained 1 .. 2 % in every session
  if (!planned)
    return ChainWidthRoundsPlan{tile, w, "gate: not on a tile all calls were dispatched on - measured slower in column rounds than call by call (profiles/chain_width_rounds_ab.txt)", true};
  return ChainWidthRoundsPlan{tile, w, "", false};
}

int chain_widths_ragged_b_kind(const GemmDesc &d, int mode, const char **why) {
  const char *w = nullptr;
  int kind = -1;
  if (mode != 1) w = "ragged mixed-width chains are off (xsmm_hip_set_chain_widths_ragged)";
  else if (d.dtype != DT_BF16) w = "a ragged mixed-width chain is bf16: an f32 call";
  else if (d.vnni_c || !d.beta0) w = "a call of a ragged mixed-width chain stores a VNNI C or is not beta 0";
  else if (d.generic_forced || d.variant_forced) w = "a call of a ragged mixed-width chain was dispatched to a forced kernel";
  else if (!chain_ragged_k_ok(d.k)) w = "a call of a ragged mixed-width chain has k below 64 or not a multiple of 8";
  else {
    GemmDesc e = d; // bf16_edge_b_kind's terms for leading dimensions, strides and lane offsets; its k term is the one above
    e.k = BK;
    if ((kind = bf16_edge_b_kind(e)) < 0) w = "a call of a ragged mixed-width chain has an operand off the grid of the LDS-DMA tiles";
  }
  if (why) *why = w;
  return w ? -1 : kind;
}

ChainWidthsRaggedPlan plan_chain_widths_ragged(int64_t m, int nlayers, const int64_t *n, const int64_t *k, const int64_t *br, int64_t cus, int forced_tile, int b_kind, int mode, bool strict) {
  auto no = [](const char *why) { return ChainWidthsRaggedPlan{-1, why, false}; };
  if (mode != 1) return no("ragged mixed-width chains are off (xsmm_hip_set_chain_widths_ragged)");
  if (strict) return no("strict mode: the tile of a ragged mixed-width chain is not a function of the descriptor alone");
  if (nlayers < 2 || nlayers > 8) return no("fewer than 2 or more than 8 calls");
  if (!blw_b_kind_ok(b_kind)) return no("the calls of a ragged mixed-width chain do not share one B image of the loader-wave tiles");
  bool differ = false;
  int64_t widest = 0;
  for (int l = 0; l < nlayers; ++l) {
    if (!chain_ragged_k_ok(k[l]) || br[l] < 1) return no("a layer of a ragged mixed-width chain has k below 64 or not a multiple of 8, or an empty batch");
    if (n[l] % 8 != 0) return no("a layer of a ragged mixed-width chain has an n that is not a multiple of 8");
    if (n[l] != n[0]) differ = true;
    if (n[l] > widest) widest = n[l];
  }
  if (!differ) return no("every call has the same n: the equal-width chain switches decide");
  // THE PARTITION (the descriptors alone, no switch): a chain SOME tile divides entirely - BM | m, BN | every n(l), every k(l) % 64 == 0 -
  // is the mixed-width chain's (xsmm_hip_set_chain_widths / _width_rounds), or call by call with those off; never this rule's
  auto holds = [&](int t) { // m and every n(l) hold at least one tile
    if (t < 0 || t > 3 || m < BLW_BM[t]) return false;
    for (int l = 0; l < nlayers; ++l)
      if (n[l] < BLW_BN[t]) return false;
    return true;
  };
  auto entire = [&](int t) {
    if (!holds(t) || m % BLW_BM[t] != 0) return false;
    for (int l = 0; l < nlayers; ++l)
      if (n[l] % BLW_BN[t] != 0 || k[l] % BK != 0) return false;
    return true;
  };
  for (int t = 0; t < 4; ++t)
    if (entire(t)) return no("a tile divides m, every n and every k entirely: the mixed-width chain's (xsmm_hip_set_chain_widths), not a ragged one");
  auto ceil_div = [](int64_t a, int64_t b) { return (a + b - 1) / b; };
  auto tiles = [&](int t) { return ceil_div(m, BLW_BM[t]) * ceil_div(widest, BLW_BN[t]); };
  // (64x128 with the VNNI-2 image has no instance - it would need scratch, blw_chain_wragged_instance_exists - and is passed over)
  auto fits = [&](int t) { return holds(t) && blw_chain_wragged_instance_exists(t, b_kind) && tiles(t) <= cus; };
  const bool forced = forced_tile >= 0 && forced_tile <= 3; // (tests and measurements: under a forcing edge-tile mode nothing is gated, whichever tile fits)
  int tile = fits(forced_tile) ? forced_tile : -1;
  for (int t = 0; t < 4 && tile < 0; ++t)
    if (fits(t)) tile = t;
  if (tile < 0) {
    if (!holds(0)) return no("a ragged mixed-width chain's m or some n is below every tile");
    return no("more tiles than compute units (a ragged mixed-width chain runs in one round)");
  }
  // THE STRUCTURAL GATE (plan_chain_widths', measured there - profiles/chain_widths_ab.txt - and again here, profiles/chain_widths_ragged_ab.txt):
  // the widest layer decides the launch's tile; a layer that ALONE fits a smaller one covers the chip with more, smaller tiles as a separate
  // call and keeps a fraction of the grid busy on the large tile in the launch. Such a chain stays call by call. Not under a forcing
  // edge-tile mode.
  if (!forced) {
    auto alone_fits = [&](int t, int l) {
      return blw_chain_wragged_instance_exists(t, b_kind) && m >= BLW_BM[t] && n[l] >= BLW_BN[t] && ceil_div(m, BLW_BM[t]) * ceil_div(n[l], BLW_BN[t]) <= cus;
    };
    for (int l = 0; l < nlayers; ++l)
      for (int s = 0; s < tile; ++s)
        if (alone_fits(s, l))
          return ChainWidthsRaggedPlan{tile, "gate: a layer fits a smaller tile alone than the widest layer leaves the launch - slower as one launch (profiles/chain_widths_ab.txt, profiles/chain_widths_ragged_ab.txt)", true};
  }
  return ChainWidthsRaggedPlan{tile, "", false};
}

int chain_rounds_b_kind(const GemmDesc &d) {
  if (d.dtype != DT_BF16 || d.vnni_c || !d.beta0 || d.generic_forced || d.variant == V_GENERIC) return -1;
  return bf16_edge_b_kind(d);
}

ChainRoundsPlan plan_chain_rounds(int64_t m, int64_t n, int nlayers, const int64_t *k, const int64_t *br, int64_t cus, int planned_tile, int mode, bool strict) {
  auto no = [](const char *why) { return ChainRoundsPlan{-1, 0, why, false}; };
  if (mode != 1 && !chain_rounds_mode_forced(mode)) return no("multi-round chains are off (xsmm_hip_set_chain_rounds)");
  if (planned_tile < -1) return no("a multi-round chain is bf16: an f32 call");
  if (nlayers < 2 || nlayers > 8) return no("fewer than 2 or more than 8 calls");
  for (int l = 0; l < nlayers; ++l)
    if (k[l] < BK || k[l] % BK != 0 || br[l] < 1) return no("a layer of a multi-round chain has k not in 64-k chunks, or an empty batch");
  auto divides = [&](int t) { return t >= 0 && t <= 3 && m >= BLW_BM[t] && n >= BLW_BN[t] && m % BLW_BM[t] == 0 && n % BLW_BN[t] == 0; };
  int tile = -1;
  if (planned_tile >= 0) {
    if (!divides(planned_tile)) return no("the planned tile does not divide a multi-round chain's m and n");
    tile = planned_tile;
  } else {
    if (strict) return no("strict mode: the calls of a multi-round chain do not share one planned loader-wave tile");
    for (int t = 3; t >= 0 && tile < 0; --t)
      if (divides(t)) tile = t;
    if (tile < 0) return no("a multi-round chain's m or n is not in whole tiles");
  }
  const int64_t tiles_m = m / BLW_BM[tile], tiles_n = n / BLW_BN[tile];
  if (tiles_m > 0x7fffffff || tiles_n > 0x7fffffff) return no("more row blocks than a launch can count");
  const int gmax = chain_rounds_max_groups((int)tiles_n, cus);
  if (gmax < 1) return no("a row of tiles is wider than the compute units");
  if (chain_rounds_mode_forced(mode)) {
    const int64_t g = mode - 1000;
    if (g < 1 || g >= tiles_m || g * tiles_n > cus) return no("the forced row groups do not fit: 1 <= G < tiles_m and G * tiles_n <= compute units");
    return ChainRoundsPlan{tile, (int)g, "", false};
  }
  if (tiles_m <= gmax) return no("the chain fits in one round: not a multi-round chain");
  const int groups = chain_rounds_groups((int)tiles_m, gmax);
  if (chain_rounds_rounds((int)tiles_m, groups) > CHAIN_ROUNDS_GATE)
    return ChainRoundsPlan{tile, groups, "gate: more than two rounds measured slower than call by call (profiles/chain_rounds_ab.txt)", true};
  return ChainRoundsPlan{tile, groups, "", false};
}

int chain_dma256_b_kind(const GemmDesc &d) {
  if (d.dtype != DT_BF16) return -2;
  if (d.vnni_c || !d.beta0 || d.generic_forced) return -1;
  const int kind = bf16_edge_b_kind(d, 3); // (k % 32, the tile's chunk; leading dimensions, strides, lane offsets)
  return kind >= 0 && d256_b_ldb_ok(kind, d.ldb) ? kind : -1;
}

bool chain_dma256_on_tile(const GemmDesc &d, int dma256_images) {
  if (d.dtype != DT_BF16 || d.vnni_c || d.generic_forced) return false;
  if (d.variant == V_BF16_DMA256) return true;
  if (dma256_images == 0 || d.variant_forced || d.variant < V_BF16_LWF_32x64 || d.variant > V_BF16_LW4_128x128 || d.m % 256 != 0 || d.n % 256 != 0) return false;
  const int kind = bf16_lw_b_kind(d);
  return (kind == 2 || kind == 4) && (dma256_images == 2 || pick_bf16_tile(d) == 2);
}

// THE GATE of plan_chain_dma256, mode 1 (gemm_plan.h). Measured (profiles/chain_dma256_ab.txt: one box, 256 CUs, three layers, bias + relu, five
// alternating pairs, us per step, call by call with every chain switch off -> one launch): 1024-wide layers (4 column tiles) at 16384 rows
// 109.65 -> 108.56 (one round; flat 110.19 -> 109.41, VNNI-4 109.20 -> 108.29) and at 32768 rows 214.65 -> 203.22 (two rounds) gain - every
// VNNI-2 and VNNI-4 pair faster, four of five flat pairs -; 4096 rows x 4096-wide layers (16 x 16 tiles, 128 chunks per layer) lose in every
// pair, 334.03 -> 337.64: a consumer there waits for sixteen producers behind layers of 112 us, and the launch it saves is 1 % of a layer.
// So a chain of MORE THAN EIGHT column tiles stays call by call (sixteen lose, four gain; nothing between was measured). (8192 rows x
// 1024, 128 tiles, lose 73.02 -> 82.61 under mode 2 - their calls run on the 128x128 tile, which fills the chip; mode 1 never takes them.)
static bool chain_dma256_gated(int64_t tiles_m, int64_t tiles_n, int groups) {
  (void)tiles_m, (void)groups;
  return tiles_n > CHAIN_DMA256_GATE_TILES_N;
}

ChainDma256Plan plan_chain_dma256(int64_t m, int64_t n, int nlayers, const int64_t *k, const int64_t *br, int64_t cus, bool all_on_tile, int b_kind, int mode, bool strict) {
  auto no = [](const char *why) { return ChainDma256Plan{false, 0, why, false}; };
  if (mode != 1 && mode != 2 && !chain_dma256_mode_forced(mode)) return no("chains on the 256x256 tile are off (xsmm_hip_set_chain_dma256)");
  if (b_kind == -2) return no("a chain on the 256x256 tile is bf16: an f32 call");
  if (nlayers < 2 || nlayers > 8) return no("fewer than 2 or more than 8 calls");
  if (!d256_image_ok(b_kind)) return no("the calls of a chain on the 256x256 tile share no B image (VNNI-2 / flat / VNNI-4, beta 0, on the tile's grid)");
  if (m < D256C_BM || n < D256C_BN || m % D256C_BM != 0 || n % D256C_BN != 0) return no("256 does not divide a chain's m and n");
  for (int l = 0; l < nlayers; ++l)
    if (!d256c_k_ok(k[l], br[l])) return no("a layer of a chain on the 256x256 tile has k not in 32-k chunks, or an empty batch");
  const int64_t tiles_m = m / D256C_BM, tiles_n = n / D256C_BN;
  if (!d256c_shape_ok(m, n, nlayers, 8, 1)) return no("more tiles than a launch can count");
  const int gmax = chain_rounds_max_groups((int)tiles_n, cus);
  if (gmax < 1) return no("a row of tiles is wider than the compute units");
  if (strict && !all_on_tile) return no("strict mode: one launch only where every call was dispatched on the 256x256 tile");
  if (chain_dma256_mode_forced(mode)) {
    const int64_t g = mode - 1000;
    if (g < 1 || g > tiles_m || g * tiles_n > cus) return no("the forced row groups do not fit: 1 <= G <= tiles_m and G * tiles_n <= compute units");
    return ChainDma256Plan{true, (int)g, "", false};
  }
  if (mode == 1 && !all_on_tile) return no("by rule only where every call runs on the 256x256 tile as a single call");
  const int groups = tiles_m <= gmax ? (int)tiles_m : chain_rounds_groups((int)tiles_m, gmax);
  if (mode == 1 && chain_dma256_gated(tiles_m, tiles_n, groups))
    return ChainDma256Plan{true, groups, "gate: more than eight column tiles measured slower as one launch than call by call (profiles/chain_dma256_ab.txt)", true};
  return ChainDma256Plan{true, groups, "", false};
}

// SKINNY-BATCH LAYER CHAINS (xsmm_hip_set_chain_skinny, opt-in; brgemm_bf16_skinny_chain.hip, brgemm_bf16_skinny_chain.h; gemm_plan.h has the contract).
int chain_skinny_b_kind(const GemmDesc &d, const char **why) {
  auto no = [&](const char *w) {
    if (why) *why = w;
    return -1;
  };
  if (d.dtype != DT_BF16) return no("a call is not bf16");
  if (!d.beta0 || d.vnni_c) return no("a call is not beta 0, or stores a VNNI C");
  if (d.generic_forced || d.variant_forced) return no("a call was dispatched with a forced kernel");
  if (!skc_ld_ok(d.lda, d.ldb, d.ldc, d.stride_a, d.stride_b, d.n, d.k))
    return no("a leading dimension does not cover its operand, or a leading dimension or stride is no multiple of 8 elements");
  return !d.vnni_b ? 2 : d.vnni_factor == 4 ? 4 : 0;
}
// Mode 1, BN and THE GATE, from profiles/chain_skinny_ab.txt (one box, 256 CUs, three layers, bias + relu, five alternating rounds, us per step;
// the baseline (a) = the same calls one by one under xsmm_hip_set_skinny_bf16(1) + xsmm_hip_set_skinny_split(1), the best existing form ->
// one launch on BN 16 / 32 / 64; a (row, BN) is taken only where it was faster than (a) in EVERY round). This replaces the provisional rule
// (the single call's BN for the layer with the most bytes of B, and the single call's m >= 17 gate):
//   Small layers, VNNI-2 - the launch's fixed parts and the stream's restarts are what a step costs: 1024 -> [1024] * 3 (B 2 MiB a layer) m 1 /
//     8 / 16 / 31: 16.92 / 17.38 / 17.50 / 18.24 -> BN 16 11.77 / 12.92 / 13.62 / 17.71 (BN 32 12.53 / 14.38 / 15.02 / 18.85: wins but for m 31;
//     BN 64 14.00 / 16.52 / 17.18 / 23.52); 1000 -> [1000] * 3: 17.11 / 17.24 / 17.07 / 17.43 -> BN 16 11.92 / 12.88 / 13.17 / 16.08; the funnel
//     784 -> 512 -> 256 -> 128: 15.41 / 15.18 / 15.13 / 15.37 -> BN 16 10.58 / 10.66 / 10.62 / 13.37 (BN 32 10.62 / 11.38 / 11.65 / 14.26). BN 16 wins
//     every round of every such row, m = 31 included (by 3 .. 13 %; 22 .. 31 % at m <= 16), and is the fastest side but for a tie at m 1 of
//     the funnel. So: BN = the smallest with an instance, and NO m >= 17 gate - what gates the single call there is the re-read of A per
//     workgroup, which the chain pays too but more than earns back at the seams.
//   Large layers - the chain has ceil(n / BN) workgroups per layer where the split single call has that times P pulling bytes: 4096 -> [4096]
//     * 3 (B 32 MiB a layer) m 1 / 8 / 16 / 31: 27.83 / 29.92 / 30.04 / 37.60 -> BN 32 31.87 / 34.12 / 36.03 / 45.12, BN 16 42.06 .. 47.16, BN 64
//     34.58 .. 51.58; flat 32.22 / 36.10 / 35.99 / 42.71 -> BN 64 37.93 / 42.52 / 45.17 / 56.66; VNNI-4 24.50 / 26.60 / 27.90 / 36.46 -> BN 16 26.18 /
//     28.12 / 31.57 / 42.50; 4096 -> 4096 -> 11008 -> 4096: 42.94 / 47.85 / 49.82 / 62.17 -> BN 64 58.77 / 62.05 / 63.41 / 75.99: every BN loses
//     every round (one round of VNNI-4 m 1 apart). THE GATE: a chain with a layer whose B exceeds 2 MiB - the largest that gained; between
//     2 and 32 MiB nothing was measured - stays call by call.
//   A flat or a VNNI-4 B was measured on 4096 -> [4096] * 3 alone, where it lost: no row of theirs gained, so mode 1 takes VNNI-2 chains
//     only. THE GATE names this too. The forced modes take every image.
// Not measured: other CU counts (the rule reads them through G alone), several ranks, beta 1 (not a chain), layers between 2 and 32 MiB,
// small flat and VNNI-4 chains, the launch without the weights ahead of the wait (not built).
constexpr int64_t SKINNY_CHAIN_GATE_BYTES = 2 << 20; // mode 1: the most bytes of B a layer of a taken chain has
ChainSkinnyPlan plan_chain_skinny(int64_t m, int nlayers, const int64_t *n, const int64_t *k, const int64_t *br, int64_t cus, int b_kind, int mode, bool strict) {
  auto no = [](const char *why) { return ChainSkinnyPlan{0, 0, why, false}; };
  const int forced_bn = mode >= 1000 ? mode % 1000 : mode == 1 ? 0 : mode, forced_g = chain_skinny_mode_forced_g(mode) ? mode / 1000 : 0;
  if (mode != 1 && !(skn_bn_ok(forced_bn) && (!chain_skinny_mode_forced_g(mode) || (forced_g >= 1 && forced_g <= SKC_GMAX))))
    return no("skinny-batch chains are off (xsmm_hip_set_chain_skinny)");
  if (nlayers < 2 || nlayers > SKC_MAXL) return no("fewer than 2 or more than 8 calls");
  if (m < 1 || m > SKN_M_MAX) return no("m is not 1 .. 31: the tiles' chain forms decide");
  if (!skn_image_ok(b_kind)) return no("the calls' B operands differ in kind (VNNI-2 / flat / VNNI-4)");
  if (strict) return no("strict mode: the launch has the bits of the calls under xsmm_hip_set_skinny_bf16, not of the calls as dispatched");
  int64_t narrowest = n[0], most_bytes = 0;
  for (int l = 0; l < nlayers; ++l) {
    if (br[l] < 1) return no("a batch is empty");
    if (!skn_shape_ok(m, n[l], k[l], br[l], 16)) return no("a layer has n < 16, n % 8 != 0, k < 8 or k % 8 != 0");
    if (n[l] >= (1 << 24) || k[l] >= (1 << 24)) return no("a layer is wider or deeper than 2^24");
    if (n[l] < narrowest) narrowest = n[l];
    if (2 * br[l] * k[l] * n[l] > most_bytes) most_bytes = 2 * br[l] * k[l] * n[l];
  }
  int bn = forced_bn;
  if (mode == 1) bn = b_kind == 2 ? 32 : 16; // the smallest with an instance
  if (!skn_instance_exists(b_kind, bn)) return no("no instance of this B image on this column-block width (flat B on 16)");
  if (narrowest < bn) return no("a layer is narrower than the column block");
  int max_blocks = 0;
  for (int l = 0; l < nlayers; ++l)
    if (skn_blocks((int)n[l], bn) > max_blocks) max_blocks = skn_blocks((int)n[l], bn);
  if (cus < 1) return no("the stream's compute units are unknown");
  if (forced_g > cus) return no("more resident workgroups forced than compute units");
  const int groups = forced_g ? forced_g : skc_groups(max_blocks, cus);
  if (mode == 1 && b_kind != 0)
    return ChainSkinnyPlan{bn, groups, "gate: no measured chain with a flat or a VNNI-4 B gained as one launch (profiles/chain_skinny_ab.txt)", true};
  if (mode == 1 && most_bytes > SKINNY_CHAIN_GATE_BYTES)
    return ChainSkinnyPlan{bn, groups, "gate: a layer with more than 2 MiB of B measured slower as one launch than call by call on the split skinny kernel (profiles/chain_skinny_ab.txt)", true};
  return ChainSkinnyPlan{bn, groups, "", false};
}

// ---- plan_chain: the layer-chain launch decision (gemm_plan.h has the order of precedence) ---------------------------------------
static const ChainLaunchPlan &chain_calls(ChainLaunchPlan &p, const char *why) {
  p.form = CF_CALLS, p.why = why;
  return p;
}
static void chain_note(ChainLaunchPlan &p, const char *rule, const char *why) {
  if (p.n_notes < 4) p.notes[p.n_notes++] = ChainLaunchPlan::Note{rule, why};
}
// the launch of `form` on `tile`: what try_chain_launch reads besides - the tile's dimensions, the grid and counter-block key (floor- or
// ceil-divided as the form says), ChainArgs::n. ns[l] = layer l's columns.
static const ChainLaunchPlan &chain_takes(ChainLaunchPlan &p, ChainForm form, int tile, int b_kind, int groups, int64_t m, int nlayers, const int64_t *ns) {
  p.form = form, p.tile = tile, p.b_kind = b_kind, p.groups = groups, p.why = "";
  if (form == CF_DMA256) p.bm = D256C_BM, p.bn = D256C_BN;
  else if (form == CF_F32) (void)f32_chain_tile_dims(tile, &p.bm, &p.bn);
  else blw_tile_dims(tile, &p.bm, &p.bn);
  const int up_m = form == CF_EDGE || form == CF_RAGGED || form == CF_WRAGGED ? p.bm - 1 : 0; // (edge row tiles)
  const int up_n = form == CF_RAGGED || form == CF_WRAGGED ? p.bn - 1 : 0;                      // (edge column tiles)
  p.mixed = form == CF_WIDTHS || form == CF_WROUNDS || form == CF_WRAGGED;
  int64_t widest = ns[0];
  for (int l = 0; l < nlayers; ++l) {
    if (ns[l] > widest) widest = ns[l];
    if (p.mixed) p.tiles_l[l] = (int)((ns[l] + up_n) / p.bn);
  }
  p.args_n = (int)widest;
  p.tiles_m = (int)((m + up_m) / p.bm);
  p.tiles_n = (int)((widest + up_n) / p.bn);
  return p;
}

ChainLaunchPlan plan_chain(int n, const GemmDesc *const *d, const int64_t *br, const ChainPlanEnv &env, ChainCus &cus) {
  ChainLaunchPlan p{};
  if (n < 2 || n > CHAIN_PLAN_MAXL) return chain_calls(p, "fewer than 2 or more than 8 calls");
  // the calls' facts, each gathered once
  const int64_t m = d[0]->m, nn = d[0]->n;
  int64_t ks[CHAIN_PLAN_MAXL], ns[CHAIN_PLAN_MAXL];
  bool differ_m = false, differ_n = false; // (differ_m: or a batch is empty)
  for (int i = 0; i < n; ++i) {
    ks[i] = d[i]->k, ns[i] = d[i]->n;
    differ_m = differ_m || d[i]->m != m || br[i] < 1;
    differ_n = differ_n || d[i]->n != nn;
  }
  const char *const differ_why = "the calls differ in m or n, or a batch is empty";

  // 0. SKINNY BATCHES (xsmm_hip_set_chain_skinny, brgemm_bf16_skinny_chain.hip): asked in front of everything, and only with the switch non-zero, a
  // bf16 first call and m <= 31 - chains no other form takes (each asks for m >= 32). Widths may differ. Where the rule refuses or gates,
  // everything below is what it is without this switch.
  if (env.skinny != 0 && d[0]->dtype == DT_BF16 && m <= SKN_M_MAX) {
    const char *w = "the calls differ in m, or a batch is empty";
    if (!differ_m) {
      w = nullptr;
      int kind = chain_skinny_b_kind(*d[0], &w);
      for (int i = 1; i < n && kind >= 0; ++i) {
        const int kind_i = chain_skinny_b_kind(*d[i], &w);
        if (kind_i < 0) kind = -1;
        else if (kind_i != kind) kind = -1, w = "the calls' B operands differ in kind (VNNI-2 / flat / VNNI-4)";
      }
      if (kind >= 0) {
        const ChainSkinnyPlan sp = plan_chain_skinny(m, n, ns, ks, br, cus.get(), kind, env.skinny, env.strict);
        if (sp.bn > 0 && !sp.gated) { // (gated: the rule's answer is on record in why, nothing is launched)
          p.form = CF_SKINNY, p.tile = sp.bn, p.b_kind = kind, p.groups = sp.groups, p.why = "";
          p.bm = (int)m, p.bn = sp.bn, p.tiles_m = skc_key_tiles_m(), p.tiles_n = skc_key_tiles_n(sp.groups), p.mixed = false;
          p.args_n = (int)ns[0];
          for (int l = 1; l < n; ++l)
            if (ns[l] > p.args_n) p.args_n = (int)ns[l];
          return p;
        }
        w = sp.why;
      }
    }
    chain_note(p, "skinny-batch launch", w);
  }

  // 1. ON THE 256x256 TILE (xsmm_hip_set_chain_dma256, brgemm_bf16_dma256_chain.hip): asked first, and only with the switch non-zero. The rule sees
  // the calls' shapes, their shared B image and whether every call runs on that tile as a single call (mode 1 reads xsmm_hip_set_dma256_images
  // for it, nothing else reads another mode). Where it takes the chain no other switch is looked at; where it refuses or gates, everything
  // below is what it is without this switch.
  if (env.dma256) {
    const char *w = differ_why;
    if (!differ_m && !differ_n) {
      const int images = env.dma256 == 1 ? env.dma256_images : 0;
      int kind = chain_dma256_b_kind(*d[0]);
      bool on_tile = true;
      for (int i = 0; i < n; ++i) {
        const int kind_i = chain_dma256_b_kind(*d[i]);
        if (kind != -2 && kind_i != kind) kind = kind_i == -2 ? -2 : -1;
        on_tile = on_tile && chain_dma256_on_tile(*d[i], images);
      }
      const ChainDma256Plan dp = plan_chain_dma256(m, nn, n, ks, br, cus.get(), on_tile, kind, env.dma256, env.strict);
      if (dp.take && !dp.gated) return chain_takes(p, CF_DMA256, 3, kind, dp.groups, m, n, ns); // (gated: the rule's answer is on record in why, nothing is launched)
      w = dp.why;
    }
    chain_note(p, "launch on the 256x256 tile", w);
  }

  // f32 chains: every call planned on the SAME K-split loader-wave tile (the launch is then bit-identical to the calls), all of its
  // workgroups resident at once. No switch is read.
  if (d[0]->dtype == DT_F32) {
    const int tile = f32_chain_tile(*d[0]);
    for (int i = 0; i < n; ++i) {
      const GemmDesc &g = *d[i];
      if (g.dtype != DT_F32 || !g.beta0 || f32_chain_tile(g) < 0 || f32_chain_tile(g) != tile)
        return chain_calls(p, "an f32 call is not beta 0 / not planned on the K-split loader-wave tile of the first call");
      if (g.ldc & 3) return chain_calls(p, "an f32 output's leading dimension is not a multiple of 4");
    }
    if (differ_m || differ_n) return chain_calls(p, differ_why);
    int bm = 0, bn = 0;
    (void)f32_chain_tile_dims(tile, &bm, &bn);
    if (m % bm != 0 || nn % bn != 0 || (m / bm) * (nn / bn) > cus.get()) return chain_calls(p, "more tiles than compute units");
    return chain_takes(p, CF_F32, tile, 0, 0, m, n, ns);
  }

  // bf16. divisible = every call passes the rules of the plain chain: bf16, beta 0, no VNNI C, one B image of the loader-wave tiles
  // (VNNI-2, flat or VNNI-4: a template parameter of the launch), not on the generic kernel.
  if (differ_m) return chain_calls(p, differ_why);
  const int lw_kind = bf16_lw_b_kind(*d[0]);
  bool divisible = true, some_generic = false;
  for (int i = 0; i < n; ++i) {
    const GemmDesc &g = *d[i];
    if (g.dtype != DT_BF16 || g.vnni_c || !g.beta0 || lw_kind < 0 || bf16_lw_b_kind(g) != lw_kind) divisible = false;
    if (g.variant == V_GENERIC) {
      // (a forced generic kernel stays generic; one that is generic only because no tile divides m may run ragged)
      if (g.generic_forced) return chain_calls(p, "a call was dispatched to the generic kernel");
      divisible = false, some_generic = true;
    }
  }
  const int et = env.edge_tiles;
  const int forced_tile = et >= V_BF16_LW_32x64 && et <= V_BF16_LW_128x128 ? et - V_BF16_LW_32x64 : -1; // (what a forcing edge-tile mode names: the ragged rules read it)

  if (differ_n) {
    // 2. and 4. MIXED WIDTHS (xsmm_hip_set_chain_widths) and COLUMN ROUNDS (xsmm_hip_set_chain_width_rounds): one question about calls the
    // plain chain's rules pass but for their n - a forced W (1000 + W) in front of plan_chain_widths, column rounds by rule (1) where
    // plan_chain_widths refuses or gates or its switch is off. Ragged shapes never combine with these two.
    if (env.widths || env.width_rounds) {
      const char *w = "a call differs in m, has an empty batch, is not bf16 / beta 0 / on a loader-wave tile, or the calls' B operands differ in kind";
      if (divisible) {
        const int planned = chain_rounds_planned_tile(n, d);
        if (chain_width_rounds_mode_forced(env.width_rounds)) { // (a forced W that does not fit: everything below as with the switch off)
          const ChainWidthRoundsPlan rp = plan_chain_width_rounds(m, n, ns, ks, br, cus.get(), planned, lw_kind, env.width_rounds, env.strict);
          if (rp.tile >= 0 && !rp.gated) return chain_takes(p, CF_WROUNDS, rp.tile, lw_kind, rp.groups, m, n, ns);
          w = rp.why;
        }
        if (env.widths) {
          const ChainWidthsPlan wp = plan_chain_widths(m, n, ns, ks, br, cus.get(), planned, lw_kind, env.widths, env.strict);
          if (wp.tile >= 0) return chain_takes(p, CF_WIDTHS, wp.tile, lw_kind, 0, m, n, ns);
          w = wp.why;
        }
        // (mode 1 without a tile all calls were dispatched on: plan_chain_width_rounds' gate, or a refusal in front of it - never a launch.
        // Answered here, without asking for the stream's compute units: on a launch-bound chain the runtime calls behind them
        // showed - 1024 rows x [1024, 512, 256, 128], gated, call by call with the switch off / on 16.38 / 17.06 us per step in every pair;
        // with this answer 18.65 / 18.65 in a later session, profiles/chain_width_rounds_ab.txt)
        if (env.width_rounds == 1 && planned < 0) w = "column rounds by rule only on a tile all calls were dispatched on (plan_chain_width_rounds' gate)";
        else if (env.width_rounds == 1) {
          const ChainWidthRoundsPlan rp = plan_chain_width_rounds(m, n, ns, ks, br, cus.get(), planned, lw_kind, env.width_rounds, env.strict);
          if (rp.tile >= 0 && !rp.gated) return chain_takes(p, CF_WROUNDS, rp.tile, lw_kind, rp.groups, m, n, ns); // (gated: on record in why, nothing is launched)
          w = rp.why;
        }
      }
      chain_note(p, "mixed-width launch", w);
    }
    // 6. RAGGED MIXED WIDTHS (xsmm_hip_set_chain_widths_ragged): where the mixed-width rules do not take the chain - every call passes
    // chain_widths_ragged_b_kind with the same B image and plan_chain_widths_ragged names a tile without a gate.
    if (env.widths_ragged) {
      const char *w = nullptr;
      int kind = chain_widths_ragged_b_kind(*d[0], env.widths_ragged, &w);
      for (int i = 1; i < n && kind >= 0; ++i)
        if (chain_widths_ragged_b_kind(*d[i], env.widths_ragged, &w) != kind) kind = -1;
      if (kind >= 0) {
        const ChainWidthsRaggedPlan rp = plan_chain_widths_ragged(m, n, ns, ks, br, cus.get(), forced_tile, kind, env.widths_ragged, env.strict);
        if (rp.tile >= 0 && !rp.gated) return chain_takes(p, CF_WRAGGED, rp.tile, kind, 0, m, n, ns); // (gated: on record in why, nothing is launched)
        w = rp.why;
      }
      chain_note(p, "ragged mixed-width launch", w ? w : "the calls' B operands differ in kind");
    }
    return chain_calls(p, differ_why);
  }

  // equal widths. RAGGED m (xsmm_hip_set_chain_edge): every call passes chain_edge_b_kind with the same B image; edge_why = why not.
  const char *edge_why = nullptr;
  int edge_kind = -1;
  if (env.edge) {
    edge_kind = chain_edge_b_kind(*d[0], env.edge, &edge_why);
    for (int i = 1; i < n && !edge_why; ++i) {
      const char *w = nullptr;
      if (chain_edge_b_kind(*d[i], env.edge, &w) != edge_kind) edge_why = w ? w : "the calls' B operands differ in kind (VNNI-2 / flat / VNNI-4)";
    }
  }
  const bool edge_on = env.edge && !edge_why;
  ChainEdgePlan ep{-1, nullptr};
  ChainRoundsPlan rp{-1, 0, nullptr, false};

  if (divisible) {
    const int planned = chain_rounds_planned_tile(n, d); // the loader-wave tile ALL calls were planned on
    auto fits = [&](int t) { // all workgroups must be co-resident (one per CU by LDS): the grid may not exceed the CUs
      int bm, bn;
      blw_tile_dims(t, &bm, &bn);
      return m % bm == 0 && nn % bn == 0 && (m / bm) * (nn / bn) <= cus.get();
    };
    // 2. a forced G (1000 + G) in front of the one-round rules (one that does not fit: everything below as with the switch off)
    if (chain_rounds_mode_forced(env.rounds)) {
      rp = plan_chain_rounds(m, nn, n, ks, br, cus.get(), planned, env.rounds, env.strict);
      if (rp.tile >= 0) return chain_takes(p, CF_ROUNDS, rp.tile, lw_kind, rp.groups, m, n, ns);
    }
    // 3. the tile every layer was planned on, if it fits: the launch is then bit-identical to the separate launches
    if (planned >= 0 && fits(planned)) return chain_takes(p, CF_PLAIN, planned, lw_kind, 0, m, n, ns);
    // 5. the one-round ragged-m launch in front of several rounds: the two switches never combine, and where a tile of other rows fits on
    // its ceil-divided grid the ragged launch wins - 32 * 257 rows x 64 of flat B, planned on 32x64 (257 tiles), run as 129 edge row
    // blocks of 64x64 with both switches on as with xsmm_hip_set_chain_edge alone (tests/test_chain_dispatch.py found the rounds)
    if (edge_on) ep = plan_chain_edge(m, nn, n, ks, br, cus.get(), forced_tile, env.strict);
    if (env.rounds == 1) rp = plan_chain_rounds(m, nn, n, ks, br, cus.get(), planned, env.rounds, env.strict);
    const bool rounds = env.rounds == 1 && rp.tile >= 0 && !rp.gated; // (gated: the rule's answer is on record in why, nothing is launched)
    // the tile all calls were planned on has more tiles than compute units: several rounds on THAT tile - the descriptors' own, G changes
    // no bit, so strict mode takes it too - in front of one round on another tile, whose bits need not be the calls'
    if (rounds && planned >= 0 && ep.tile < 0) return chain_takes(p, CF_ROUNDS, rp.tile, lw_kind, rp.groups, m, n, ns);
    // (the parent's order, kept: strict mode refuses HERE - behind several rounds on the planned tile, in front of the smallest tile that fits)
    if (env.strict) return chain_calls(p, env.rounds == 1 ? rp.why : "strict mode: one launch only on the tile the layers were planned on");
    for (int t = 0; t < 4; ++t) // the smallest tile that fits (most CUs busy)
      if (fits(t)) return chain_takes(p, CF_PLAIN, t, lw_kind, 0, m, n, ns);
    if (ep.tile >= 0) return chain_takes(p, CF_EDGE, ep.tile, edge_kind, 0, m, n, ns);
    // only a shape every tile of which divides - one the ragged rule has just refused - may run in several rounds on a tile of the rule's choice
    if (rounds) return chain_takes(p, CF_ROUNDS, rp.tile, lw_kind, rp.groups, m, n, ns);
    return chain_calls(p, edge_on ? ep.why : env.rounds == 1 ? rp.why : "more tiles than compute units");
  }

  // calls the plain chain's rules refuse because of their SHAPE: no loader-wave tile divides one (no B image by bf16_lw_b_kind, planned on
  // the generic kernel)
  if (chain_rounds_mode_forced(env.rounds)) {
    // 2. a forced G is asked in front of the one-round rules, so also in front of their m and n terms (bf16_lw_b_kind: 64 rows for VNNI-2):
    // every call has one B image by chain_rounds_b_kind
    int kind = chain_rounds_b_kind(*d[0]);
    for (int i = 1; i < n; ++i)
      if (chain_rounds_b_kind(*d[i]) != kind) kind = -1;
    if (kind >= 0) {
      rp = plan_chain_rounds(m, nn, n, ks, br, cus.get(), chain_rounds_planned_tile(n, d), env.rounds, env.strict);
      if (rp.tile >= 0) return chain_takes(p, CF_ROUNDS, rp.tile, kind, rp.groups, m, n, ns);
      // (the parent's order, kept: a forced G that does not fit ends the decision HERE unless the ragged-m rule may still be asked - the
      // ragged-width rule below is not asked on its own)
      if (!edge_on) return chain_calls(p, rp.why);
    }
  }
  // 5. one round on edge row tiles
  if (edge_on) {
    ep = plan_chain_edge(m, nn, n, ks, br, cus.get(), forced_tile, env.strict);
    if (ep.tile >= 0) return chain_takes(p, CF_EDGE, ep.tile, edge_kind, 0, m, n, ns);
  }
  // 6. RAGGED WIDTH (xsmm_hip_set_chain_ragged): where the others refuse because of n or k - a k % 64, an n % 64, plan_chain_edge's refusal
  // (n not in whole column tiles). Every call passes chain_ragged_b_kind with the same B image and plan_chain_ragged names a tile.
  if (env.ragged) {
    const char *w = nullptr;
    int kind = chain_ragged_b_kind(*d[0], env.ragged, &w);
    for (int i = 1; i < n && kind >= 0; ++i)
      if (chain_ragged_b_kind(*d[i], env.ragged, &w) != kind) kind = -1;
    if (kind >= 0) {
      const ChainRaggedPlan gp = plan_chain_ragged(m, nn, n, ks, br, cus.get(), forced_tile, kind, env.ragged, env.strict);
      if (gp.tile >= 0) return chain_takes(p, CF_RAGGED, gp.tile, kind, 0, m, n, ns);
      w = gp.why;
    }
    chain_note(p, "ragged-width launch", w ? w : "the calls' B operands differ in kind");
  }
  if (env.widths_ragged) chain_note(p, "ragged mixed-width launch", "every call has the same n: the equal-width chain switches decide");
  if (edge_on) return chain_calls(p, ep.why);
  if (edge_why) return chain_calls(p, edge_why);
  return chain_calls(p, some_generic ? "a call was dispatched to the generic kernel"
                                     : "a call is not bf16 / beta 0 / aligned for the LDS-DMA tiles, or the calls' B operands differ in kind (VNNI-2 / flat / VNNI-4)");
}

static GemmLaunch launch(GemmLauncher l, int tile = 0, const char *text = "", int split = 1, int b_kind = 0, bool even = false) {
  return GemmLaunch{l, tile, split, b_kind, even, false, GG_F32, text};
}
static GemmLaunch generic(GemmGeneric g, const char *text = "") { return GemmLaunch{GL_GENERIC, 0, 1, 0, false, false, g, text}; }

// An operand read transposed (a folded xsmm.unary transpose, rt_rewrites.h): the generic kernel. A sibling made under mode 1 of
// xsmm_hip_set_fold_transpose (B only) stays on the element-wise loads it has always had. A mode-2 sibling (GemmDesc::trans_mode)
// runs on the 16-byte instance of its form when the lane offsets and pieces allow - every A and B pointer 16-byte aligned, k in
// whole pieces, leading dimensions and strides in whole pieces and below 2^24 (32 rows x ld x 4 B < 2^31); a transposed A
// is staged in 4-row pieces of m and its B operand in 4-column pieces of n, a transposed B needs nothing of n (columns are the
// rows of its image) - and on the element instance of its form otherwise. text: what a GROUP reports ("" for a single call, as before).
static GemmLaunch trans_launch(const GemmDesc &d, bool vec_ok, bool group) {
  if (d.dtype != DT_F32 || d.vnni_b || (d.a_trans && (d.b_trans || d.vnni_c))) return launch(GL_INVALID);
  const bool vec = d.trans_mode == 2 && vec_ok && d.k % 4 == 0 && !((d.lda | d.ldb | d.stride_a | d.stride_b) & 3) && d.lda < (1 << 24) &&
                   d.ldb < (1 << 24) && (!d.a_trans || (d.m % 4 == 0 && d.n % 4 == 0));
  if (d.a_trans) return vec ? generic(GG_F32_AT_VEC, group ? "brgemm_grouped<f32,v4>, A read transposed" : "")
                            : generic(GG_F32_AT, group ? "brgemm_grouped<f32>, A read transposed" : "");
  return vec ? generic(GG_F32_BT_VEC, group ? "brgemm_grouped<f32,v4>, B read transposed" : "")
             : generic(GG_F32, group ? "brgemm_grouped<f32>, B read transposed" : "");
}

GemmLaunch plan_gemm_call(const GemmDesc &d, int64_t br_in, const GemmAlign &al, const GemmPlanEnv &env) {
  if (d.m <= 0 || d.n <= 0) return launch(GL_NONE);
  const int64_t cus = env.cus;
  const int br = (int)(br_in < 0 ? 0 : br_in);
  int v = d.variant;
  if (d.b_trans || d.a_trans) return trans_launch(d, al.ab16, false);
  // bf16x6: the planned split tile whatever the batch count, split setting or pointer alignment (unaligned A / B: element loads)
  if (gemm_on_x6(d))
    return GemmLaunch{GL_F32_X6, v - V_F32_X6_64x64, 1, 0, false, al.ab16, GG_F32, ""};
  if (v != V_GENERIC && !al.ab16) v = V_GENERIC;
  // the bf16 kernel stores 16-byte row pieces and reads the bias 8 bytes at a time
  const bool bias_ok8 = !d.bias || al.d8;
  if (v >= V_BF16_FAST && v != V_BF16_SMALL32 && !(al.c16 && bias_ok8)) v = V_GENERIC;
  if (v == V_BF16_SMALL32 && !(al.c8 && bias_ok8)) v = V_GENERIC;
  // Skinny-batch bf16 layers, if asked for (xsmm_hip_set_skinny_bf16, a switch of its own; brgemm_bf16_skinny.hip, brgemm_bf16_skinny.h): a
  // bf16 call with 1 <= m <= 31 that is planned - not forced - on the generic kernel, whichever of the three B images it has, on ceil(n / BN)
  // workgroups that stream B straight into MFMA operand registers. No other refinement takes a call with m < 32, so its place in this
  // function is free; it reads no other mode. Decided here only - what is queued, grouped, chained or folded never sees it -, from the
  // descriptor, the batch count, the pointers' alignment and the CU count: allowed in strict mode. The alignment rules are the launcher's
  // (launch_bf16_skinny: A, B, C 16-byte and the bias row 8-byte aligned, every leading dimension and stride a multiple of 8 elements);
  // refused there, the call runs the launch it has with the mode off (launch_gemm). The one switch read inside this block is
  // xsmm_hip_set_skinny_split: the K range of the launch over several workgroups per column block (split, text); a split refused by ITS
  // launcher runs the unsplit launch of the same BN.
  if (env.skinny_bf16 != 0 && d.dtype == DT_BF16 && !d.vnni_c && !d.generic_forced && !d.variant_forced && d.variant == V_GENERIC &&
      skn_shape_ok(d.m, d.n, d.k, br, 16) && d.lda >= d.k && d.ldb >= d.n && d.ldc >= d.n && !((d.lda | d.ldb | d.ldc | d.stride_a | d.stride_b) & 7) &&
      d.stride_a >= 0 && d.stride_b >= 0 && d.n < (1 << 30) && d.k < (1 << 30) && al.ab16 && al.c16 && bias_ok8) {
    const int kind = !d.vnni_b ? 2 : d.vnni_factor == 4 ? 4 : 0;
    const int bn = skinny_bf16_bn(d, kind, env.skinny_bf16, br, al.ab16);
    if (bn > 0) {
#define SK_NAMES(F) {{"brgemm_bf16_skinny" F "<16x16>", "brgemm_bf16_skinny" F "<16x32>", "brgemm_bf16_skinny" F "<16x64>"}, \
                     {"brgemm_bf16_skinny" F "<32x16>", "brgemm_bf16_skinny" F "<32x32>", "brgemm_bf16_skinny" F "<32x64>"}}
      static const char *const skinny_names[2][3][2][3] = {{SK_NAMES(""), SK_NAMES("_flatb"), SK_NAMES("_vnni4")},
                                                           {SK_NAMES("_split"), SK_NAMES("_split_flatb"), SK_NAMES("_split_vnni4")}};
#undef SK_NAMES
      // the K range of the launch over several workgroups per column block, if asked for (xsmm_hip_set_skinny_split): read here only
      const int parts = env.skinny_split != 0 ? skinny_split_parts(d, bn, env.skinny_split, br, cus) : 1;
      return launch(GL_BF16_SKINNY, bn, skinny_names[parts > 1][kind / 2][skn_mb((int)d.m) == 32][bn == 16 ? 0 : bn == 32 ? 1 : 2], parts, kind);
    }
  }
  // Edge tiles on the 256x256 tile, if asked for (xsmm_hip_set_dma256_edge, a switch of its own; brgemm_bf16_dma256_edge.hip,
  // brgemm_bf16_dma256_edge.h): a large call - m, n >= 256 - whose m or n the 256x256 tile does not divide, whatever kernel it is planned -
  // not forced - on and whichever of the three B images it has, on the ceil-divided grid of that tile. Mode 1: dma256_edge_rule; mode 2
  // (tests, measurements): every eligible call. Asked before the loader-wave edge tiles and read by no other switch. Decided here only -
  // what is queued, grouped, chained or made a quad never sees it -, from the descriptor, the batch count, the pointers' alignment and the CU
  // count: allowed in strict mode. n % 8 keeps the shifted column tile on 16 bytes of C, of every B image and of the bias row. The launcher's
  // own checks: launch_bf16_dma256_edge; refused there, the call runs the launch it has with the mode off (launch_gemm).
  if (env.dma256_edge != 0 && d.dtype == DT_BF16 && !d.vnni_c && !d.generic_forced && !d.variant_forced && d.m >= 256 && d.n >= 256 &&
      (d.m % 256 != 0 || d.n % 256 != 0) && d.n % 8 == 0 && d.k % 32 == 0 && br >= 1 && al.ab16 && al.c16 && bias_ok8) {
    const int kind = bf16_edge_b_kind(d, 3);
    if (kind >= 0 && (env.dma256_edge == 2 || dma256_edge_rule(d))) {
      static const char *const names[3] = {"brgemm_bf16_dma<256x256>, edge tiles", "brgemm_bf16_dma_flatb<256x256>, edge tiles",
                                           "brgemm_bf16_dma_vnni4<256x256>, edge tiles"};
      GemmLaunch l = launch(GL_BF16_FAST, 2, names[kind / 2], 1, kind);
      l.edge = true;
      return l;
    }
  }
  // bf16 edge tiles, if asked for (choose_bf16_edge_tile): a call no loader-wave tile divides, before the refinements of the 32x32 K-split
  // kernel below. Decided here only - what is queued, grouped, chained or made a quad never sees it -, from the descriptor, the batch
  // count, the pointers' alignment and the CU count: allowed in strict mode. n % 8 keeps the shifted column tile on 16 bytes of C, of a
  // flat B and of the bias row. The launcher's own checks: blw_launch_ok, BLW_EDGE.
  if ((env.edge_tiles == 2 || (env.edge_tiles >= V_BF16_LW_32x64 && env.edge_tiles <= V_BF16_LW_128x128)) && d.dtype == DT_BF16 && !d.vnni_c &&
      !d.generic_forced && !d.variant_forced && (d.variant == V_GENERIC || d.variant == V_BF16_SMALL32) && (d.m % 32 != 0 || d.n % 64 != 0) &&
      d.n % 8 == 0 && br >= 1 && al.ab16 && al.c16 && bias_ok8) {
    const int kind = bf16_edge_b_kind(d);
    const int tile = kind >= 0 ? choose_bf16_edge_tile(d, env.edge_tiles, (int64_t)br * (d.k / BK), cus) : -1;
    if (tile >= 0) {
      static const char *const edge_names[3][4] = {
          {"brgemm_bf16_lw<32x64,k2>, edge tiles", "brgemm_bf16_lw<64x64>, edge tiles", "brgemm_bf16_lw<64x128>, edge tiles", "brgemm_bf16_lw<128x128>, edge tiles"},
          {"brgemm_bf16_lw_flatb<32x64,k2>, edge tiles", "brgemm_bf16_lw_flatb<64x64>, edge tiles", "brgemm_bf16_lw_flatb<64x128>, edge tiles",
           "brgemm_bf16_lw_flatb<128x128>, edge tiles"},
          {"brgemm_bf16_lw_vnni4<32x64,k2>, edge tiles", "brgemm_bf16_lw_vnni4<64x64>, edge tiles", "brgemm_bf16_lw_vnni4<64x128>, edge tiles",
           "brgemm_bf16_lw_vnni4<128x128>, edge tiles"}};
      GemmLaunch l = launch(GL_BF16_LW, tile, edge_names[kind / 2][tile], 1, kind);
      l.edge = true;
      return l;
    }
  }
  // bf16 ragged k, if asked for (xsmm_hip_set_edge_k_bf16, a switch of its own; choose_bf16_kedge_tile): k >= 64 a multiple of 16 but not of
  // 64. Decided here only, like the edge tiles, from the descriptor, the batch count, the pointers' alignment and the CU count: allowed
  // in strict mode. The tile a forcing edge_k_bf16 value names, else the one a forcing edge-tile mode names, else the rule's; a tile that
  // does not divide m and n needs a bf16 edge-tile mode on as well. The launcher's own checks: blw_launch_ok, BLW_KEDGE.
  if (env.edge_k_bf16 != 0 && d.dtype == DT_BF16 && !d.vnni_c && !d.generic_forced && !d.variant_forced &&
      (d.variant == V_GENERIC || d.variant == V_BF16_SMALL32) && bkedge_k_ok(d.k) && d.n % 8 == 0 && br >= 1 && al.ab16 && al.c16 && bias_ok8) {
    const bool force_e = env.edge_tiles >= V_BF16_LW_32x64 && env.edge_tiles <= V_BF16_LW_128x128;
    const bool edge_on = env.edge_tiles == 2 || force_e;
    const int forced = env.edge_k_bf16 >= V_BF16_LW_32x64 && env.edge_k_bf16 <= V_BF16_LW_128x128 ? env.edge_k_bf16 - V_BF16_LW_32x64
                       : force_e ? env.edge_tiles - V_BF16_LW_32x64 : -1;
    // The rule's gate (measured, profiles/edge_k_bf16_ab.txt: 256x1024x400 3.31 -> 4.27 us, 128x1024x80 3.12 -> 3.55 on the tiles): a call
    // planned on the 32x32 K-split kernel whose 32x32 tiles fit ONE round of the CUs, with a reduction below that kernel's crossover
    // against the loader-wave tiles (br * k < 1024, the long-reduction rule below), stays there. A forced tile is a forced tile.
    const bool gated = forced < 0 && d.variant == V_BF16_SMALL32 && (d.m / 32) * (d.n / 32) <= cus && (int64_t)br * d.k < 1024;
    const int kind = gated ? -1 : bf16_edge_b_kind(d, 1);
    const int tile = kind >= 0 ? choose_bf16_kedge_tile(d, forced, edge_on, (int64_t)br * bkedge_chunks((int)d.k), cus) : -1;
    if (tile >= 0) {
#define KE_NAMES(F, S) {"brgemm_bf16_lw" F "<32x64,k2>" S, "brgemm_bf16_lw" F "<64x64>" S, "brgemm_bf16_lw" F "<64x128>" S, "brgemm_bf16_lw" F "<128x128>" S}
      static const char *const kedge_names[2][3][4] = {
          {KE_NAMES("", ", ragged k"), KE_NAMES("_flatb", ", ragged k"), KE_NAMES("_vnni4", ", ragged k")},
          {KE_NAMES("", ", edge tiles, ragged k"), KE_NAMES("_flatb", ", edge tiles, ragged k"), KE_NAMES("_vnni4", ", edge tiles, ragged k")}};
#undef KE_NAMES
      const bool mn_ragged = d.m % BLW_BM[tile] != 0 || d.n % BLW_BN[tile] != 0;
      GemmLaunch l = launch(GL_BF16_LW, tile, kedge_names[mn_ragged][kind / 2][tile], 1, kind);
      l.edge_k = true;
      return l;
    }
  }
  // bf16 ragged k in HALF steps, if asked for (xsmm_hip_set_edge_k8_bf16, a switch of its own; brgemm_bf16_lw_kedge.h bkedge8_*): k >= 64 a
  // multiple of 8 but not of 16 (1000, 200, 72). The block above with bkedge8_k_ok and env.edge_k8_bf16: the two switches partition the
  // lengths (k % 16 == 0 / == 8) and neither looks at the other's mode. The launcher's own checks: blw_launch_ok, BLW_KEDGE8.
  if (env.edge_k8_bf16 != 0 && d.dtype == DT_BF16 && !d.vnni_c && !d.generic_forced && !d.variant_forced &&
      (d.variant == V_GENERIC || d.variant == V_BF16_SMALL32) && bkedge8_k_ok(d.k) && d.n % 8 == 0 && br >= 1 && al.ab16 && al.c16 && bias_ok8) {
    const bool force_e = env.edge_tiles >= V_BF16_LW_32x64 && env.edge_tiles <= V_BF16_LW_128x128;
    const bool edge_on = env.edge_tiles == 2 || force_e;
    const int forced = env.edge_k8_bf16 >= V_BF16_LW_32x64 && env.edge_k8_bf16 <= V_BF16_LW_128x128 ? env.edge_k8_bf16 - V_BF16_LW_32x64
                       : force_e ? env.edge_tiles - V_BF16_LW_32x64 : -1;
    // The gate of the block above, carried over unchanged; what was measured for these k: profiles/edge_k8_bf16_ab.txt.
    const bool gated = forced < 0 && d.variant == V_BF16_SMALL32 && (d.m / 32) * (d.n / 32) <= cus && (int64_t)br * d.k < 1024;
    const int kind = gated ? -1 : bf16_edge_b_kind(d, 2);
    const int tile = kind >= 0 ? choose_bf16_kedge_tile(d, forced, edge_on, (int64_t)br * bkedge_chunks((int)d.k), cus) : -1;
    if (tile >= 0) {
#define KE_NAMES(F, S) {"brgemm_bf16_lw" F "<32x64,k2>" S, "brgemm_bf16_lw" F "<64x64>" S, "brgemm_bf16_lw" F "<64x128>" S, "brgemm_bf16_lw" F "<128x128>" S}
      static const char *const kedge8_names[2][3][4] = {
          {KE_NAMES("", ", ragged k, half step"), KE_NAMES("_flatb", ", ragged k, half step"), KE_NAMES("_vnni4", ", ragged k, half step")},
          {KE_NAMES("", ", edge tiles, ragged k, half step"), KE_NAMES("_flatb", ", edge tiles, ragged k, half step"),
           KE_NAMES("_vnni4", ", edge tiles, ragged k, half step")}};
#undef KE_NAMES
      const bool mn_ragged = d.m % BLW_BM[tile] != 0 || d.n % BLW_BN[tile] != 0;
      GemmLaunch l = launch(GL_BF16_LW, tile, kedge8_names[mn_ragged][kind / 2][tile], 1, kind);
      l.edge_k8 = true;
      return l;
    }
  }
  // FLAT and VNNI-4 B on the 256x256 tile, if asked for (xsmm_hip_set_dma256_images; brgemm_bf16_dma256.hip entry points _flatb / _vnni4,
  // brgemm_bf16_dma256_images.h): a call planned - not forced - on a flat or VNNI-4 loader-wave tile whose m and n the 256x256 tile divides.
  // Mode 1, the rule: where plan_gemm sends a VNNI-2 descriptor to this tile, pick_bf16_tile(d) == 2 (at least 240 tiles and the fill
  // term); mode 2 (tests, measurements) takes every eligible call. Decided here only - what is queued, grouped, chained or made a quad
  // never sees it -, from the descriptor, the batch count, the pointers' alignment and the CU count: allowed in strict mode. The launcher's
  // own checks: launch_bf16_dma256_image; refused there, the call runs the launch it has with the mode off (launch_gemm).
  // Measured (profiles/dma256_images_ab.txt: one box, 256 CUs, five alternating pairs off / on, us per call, 128x128 image tile -> this one;
  // the VNNI-2 kernel on the same shapes in the same session: 104.14, 132.13, 34.33, 33.28, 35.83, 69.87):
  //   VNNI-4: 4096^3 125.14 -> 104.36, 8192x8192x1024 191.56 -> 130.29, 4096x4096x1024 44.75 -> 34.38, 3840x4096x1024 (240 tiles) 44.86 ->
  //           33.98, 16384x1024x1024 54.39 -> 35.15, 32768x1024x1024 84.85 -> 69.21
  //   flat:   4096^3 130.50 -> 106.84, 8192x8192x1024 201.97 -> 133.68, 4096x4096x1024 44.86 -> 34.61, 3840x4096x1024 42.86 -> 34.29,
  //           16384x1024x1024 56.38 -> 35.54, 32768x1024x1024 93.74 -> 69.77
  // Every pair of every row is faster and both images run at the VNNI-2 kernel's times, so the VNNI-2 rule holds for both as it is and
  // no row needs a gate. (The 32768-row rows: every run on this tile, 68.62 .. 70.17, is below every run off it, 76.02 .. 111.38, but that
  // session's switch-off runs spread wider than the gain, so by the letter of the discipline the row shows no difference there; an earlier
  // session had it faster, VNNI-4 74.52 -> 68.79.) Control, mode 2 on 64 tiles: 2048^3 flat 17.80 -> 42.76, VNNI-4 18.13 -> 41.75 - the fill
  // term of pick_bf16_tile is needed.
  if (env.dma256_images != 0 && d.dtype == DT_BF16 && !d.vnni_c && !d.generic_forced && !d.variant_forced && d.variant >= V_BF16_LWF_32x64 &&
      d.variant <= V_BF16_LW4_128x128 && d.m % 256 == 0 && d.n % 256 == 0 && br >= 1 && al.ab16 && al.c16 && bias_ok8) {
    const int kind = bf16_lw_b_kind(d);
    if ((kind == 2 || kind == 4) && (env.dma256_images == 2 || pick_bf16_tile(d) == 2))
      return launch(GL_BF16_FAST, 2, kind == 2 ? "brgemm_bf16_dma_flatb<256x256>" : "brgemm_bf16_dma_vnni4<256x256>", 1, kind);
  }
  // Small bf16 outputs with a LONG reduction: the 32x32 K-split kernel (fragments straight from global memory, two groups of loads
  // in flight per wave) is latency-bound there - 128 x 1024 x 4096: 15.4 us against 9.8 on 64 loader-wave tiles of 32x64 and 8.1 on
  // 128 tiles of 32x32 + K2 (the same kernel, twice the workgroups pulling panels). Crossovers (profiles/r05_bf16_skinny_small_vs_lw.txt):
  // against the 32x32 + K2 instance - usable when the output is at most one 32x32 tile per CU - at K = 1024 (256 x 1024 x 1024: 4.78
  // against 5.05 us, the reference's bs = 256 bf16 MLP as whole-layer calls 14.3 against 15.7; at K = 768 the K-split kernel still
  // wins by 0.06-0.2 us), against the 32x64 tile between 1024 and 2048. The batch count arrives with the invoke, so this choice is
  // made here and not at dispatch.
  if (v == V_BF16_SMALL32 && d.variant == V_BF16_SMALL32 && !d.generic_forced && d.k % 64 == 0 && d.m % 32 == 0 && d.n % 64 == 0 && al.c16 &&
      bias_ok8 && !d.variant_forced) {
    const bool t32 = (d.m / 32) * (d.n / 32) <= cus;
    const int64_t thr = t32 ? 1024 : 1536;
    GemmDesc e = d;
    e.m = (d.m + 63) / 64 * 64; // (bf16_fast_eligible asks for m % 64; these tiles need m % 32 only)
    if ((int64_t)br * d.k >= thr && bf16_fast_eligible(e))
      return t32 ? launch(GL_BF16_LW, 4, "brgemm_bf16_lw<32x32,k2> (long reduction)") : launch(GL_BF16_LW, 0, "brgemm_bf16_lw<32x64,k2> (long reduction)");
  }
  if (v >= V_BF16_LW_32x64 && v <= V_BF16_LW4_128x128 && br < 1) v = V_GENERIC; // empty batch (C = epilogue of nothing): the loader-wave kernels assume a chunk
  if (v >= V_F32_64x64 && v <= V_F32_64x64K2) return launch(GL_F32_FAST, v);
  if (v == V_F32_LW_64x64 || v == V_F32_LW_128x64) return launch(GL_F32_LW, v == V_F32_LW_64x64 ? 0 : 4);
  if (v == V_F32_LW_64x64K2 || v == V_F32_LW_64x32K2 || v == V_F32_LW_32x32K4) {
    // skinny outputs (fewer tiles than CUs, a long batch-reduce): several workgroups per tile (choose_f32_split)
    static const char *const split_names[4] = {"", "brgemm_f32_lw<64x64,k2>, split", "brgemm_f32_lw<64x32,k4>, split", "brgemm_f32_lw<32x32,k4>, split"};
    const int tile = v == V_F32_LW_32x32K4 ? 3 : v - V_F32_LW_64x64;
    const int bm = tile == 3 ? 32 : 64, bn = tile == 1 ? 64 : 32;
    const long long tiles = (long long)(d.m / bm) * (d.n / bn), chunks = (long long)br * (d.k / BK);
    const int S = choose_f32_split(tile, tiles, chunks, env);
    // more tiles than CUs and a partial last round: its tiles over the CUs it leaves idle, if asked for (choose_f32_tail_split)
    static const char *const tail_names[4] = {"", "brgemm_f32_lw<64x64,k2>, tail split", "brgemm_f32_lw<64x32,k4>, tail split", "brgemm_f32_lw<32x32,k4>, tail split"};
    int tail_tiles = 0;
    const int tail_S = S == 1 ? choose_f32_tail_split(tile, tiles, chunks, env, &tail_tiles) : 1;
    if (tail_S > 1) {
      GemmLaunch l = launch(GL_F32_LW, tile, tail_names[tile], 1);
      l.tail_tiles = tail_tiles, l.tail_split = tail_S;
      return l;
    }
    GemmLaunch l = launch(GL_F32_LW, tile, S > 1 ? split_names[tile] : "", S);
    l.halves = S == 1 && choose_f32_halves(tile, d, tiles, env);
    return l;
  }
  // (the half-width tiles store 16-byte pieces of C and of the bias row: else the generic kernel below)
  if (v == V_F32_LW16_32x16 && al.c16 && (!d.bias || al.d16)) {
    // LONG reductions (K >= 3072): every XCD streams all of A besides its share of B on the half-width tiles and their chunk time
    // rises by 40 % (128 x 1024 x 4096: 14.6 us); the 32x32 tiles with the k range shared between XCD-aligned workgroups fetch every
    // byte once (12.8 us). The batch count arrives with the invoke, so this is decided here. (profiles/r05_lw16_vs_split.txt)
    const long long chunks = (long long)br * (d.k / BK);
    const int S = chunks >= 48 && !d.variant_forced && d.n % 32 == 0 ? choose_f32_split(3, (long long)(d.m / 32) * (d.n / 32), chunks, env) : 1;
    return launch(GL_F32_LW16, 0, S > 1 ? "brgemm_f32_lw<32x32,k4>, split (long reduction)" : "", S);
  }
  if (v >= V_BF16_FAST && v <= V_BF16_DMA256) return launch(GL_BF16_FAST, v - V_BF16_FAST);
  if (v == V_BF16_SMALL32) return launch(GL_BF16_SMALL32);
  if (v >= V_BF16_LW_32x64 && v <= V_BF16_LW_128x128) return launch(GL_BF16_LW, v - V_BF16_LW_32x64);
  if (v >= V_BF16_LWF_32x64 && v <= V_BF16_LWF_128x128) return launch(GL_BF16_LW, v - V_BF16_LWF_32x64, "", 1, 2);
  if (v >= V_BF16_LW4_32x64 && v <= V_BF16_LW4_128x128) {
    // (round 6) skinny outputs with a long reduction: the 32x32 + K2 instance, as for VNNI-2 operands above - at most one 32x32 tile
    // per CU and K >= 1024: twice the workgroups of the 32x64 tile pulling panels (128 x 1024 x 4096: 9.3 -> 7.6 us)
    if (v == V_BF16_LW4_32x64 && !d.variant_forced && !d.generic_forced && d.m % 32 == 0 && d.n % 32 == 0 && (d.m / 32) * (d.n / 32) <= cus &&
        (int64_t)br * d.k >= 1024)
      return launch(GL_BF16_LW, 4, "brgemm_bf16_lw_vnni4<32x32,k2> (long reduction)", 1, 4);
    return launch(GL_BF16_LW, v - V_BF16_LW4_32x64, "", 1, 4);
  }
  // everything else: the kernel of a group of this one invoke. Spelled out rather than plan_gemm_group(n_items = 1): a group of one
  // tries the half-width lw16 tiles first, a single invoke keeps the pair / ragged 32x32 tile it has always run on.
  const GenericOk g = generic_ok(d, al.ab16);
  const bool f32_lw = g.vec && !d.generic_forced && d.m % 32 == 0 && f32_lw_operands_ok(d);
  // edge tiles, if asked for (choose_f32_edge_variant): a call no tile divides. Decided here only - what is queued, grouped, chained or
  // folded never sees it -, from the descriptor, the batch count, the pointers' alignment and the CU count: allowed in strict mode. A
  // forced split count and the tail split do not apply. The launcher's own checks: launch_f32_lw_edge.
  if (f32_edge_mode(env.edge_tiles) != 0 && d.dtype == DT_F32 && !d.vnni_b && !d.vnni_c && !d.generic_forced && d.variant == V_GENERIC && d.k > 0 &&
      d.k % BK == 0 && br >= 1 && f32_lw_operands_ok(d) && d.ldc % 4 == 0 && d.n % 4 == 0 && al.ab16 && al.c16 && (!d.bias || al.d16)) {
    static const char *const edge_names[5] = {"", "brgemm_f32_lw<64x64,k2>, edge tiles", "brgemm_f32_lw<64x32,k4>, edge tiles",
                                              "brgemm_f32_lw<32x32,k4>, edge tiles", "brgemm_f32_lw<128x64,k1>, edge tiles"};
    const int ev = choose_f32_edge_variant(d, f32_edge_mode(env.edge_tiles), cus);
    if (ev >= 0) {
      const int tile = ev == V_F32_LW_128x64 ? 4 : ev == V_F32_LW_32x32K4 ? 3 : ev - V_F32_LW_64x64;
      GemmLaunch l = launch(GL_F32_LW, tile, edge_names[tile]);
      l.edge = true;
      return l;
    }
  }
  // ragged k, if asked for (xsmm_hip_set_edge_k; brgemm_f32_lw_kedge.h): k >= 64 a multiple of 8 but not of 64 - planned on the generic
  // kernel - on a loader-wave tile whose last chunk per batch element is shifted back (brgemm_f32_lw.hip brgemm_f32_lw_kedge). The tile:
  // the forced one (edge_k 6 / 7 / 9 / 10, else a forcing edge-tile mode), else choose_f32_edge_variant's rule - on ceil-divided counts
  // it is the divisible shapes' rule too. A tile that does not divide m and n is taken only with the f32 edge tiles on as well: else
  // the call stays where it is. Decided here only, like the edge tiles; a forced split count and the tail split do not apply.
  if (env.edge_k != 0 && d.dtype == DT_F32 && !d.vnni_b && !d.vnni_c && !d.generic_forced && d.variant == V_GENERIC && kedge_k_ok(d.k) && br >= 1 &&
      f32_lw_operands_ok(d) && d.ldc % 4 == 0 && d.n % 4 == 0 && al.ab16 && al.c16 && (!d.bias || al.d16)) {
    static const char *const kedge_names[2][5] = {
        {"", "brgemm_f32_lw<64x64,k2>, ragged k", "brgemm_f32_lw<64x32,k4>, ragged k", "brgemm_f32_lw<32x32,k4>, ragged k", "brgemm_f32_lw<128x64,k1>, ragged k"},
        {"", "brgemm_f32_lw<64x64,k2>, edge tiles, ragged k", "brgemm_f32_lw<64x32,k4>, edge tiles, ragged k", "brgemm_f32_lw<32x32,k4>, edge tiles, ragged k",
         "brgemm_f32_lw<128x64,k1>, edge tiles, ragged k"}};
    static const int bm[5] = {0, 64, 64, 32, 128}, bn[5] = {0, 64, 32, 32, 64};
    const int em = f32_edge_mode(env.edge_tiles);
    const int ev = choose_f32_edge_variant(d, env.edge_k != 1 ? env.edge_k : em != 0 ? em : 1, cus);
    if (ev >= 0) {
      const int tile = ev == V_F32_LW_128x64 ? 4 : ev == V_F32_LW_32x32K4 ? 3 : ev - V_F32_LW_64x64;
      const bool mn_ragged = d.m % bm[tile] != 0 || d.n % bn[tile] != 0;
      if (!mn_ragged || em != 0) {
        GemmLaunch l = launch(GL_F32_LW, tile, kedge_names[mn_ragged][tile]);
        l.edge_k = true;
        return l;
      }
    }
  }
  // a SINGLE invoke of a 32-k f32 tile with an even batch count: the kernel its group would run on in the tile queue (the
  // loader-wave pair mode, tile chosen as plan_gemm_group does for one item) - queue on and queue off then add in the same order
  if (f32_lw && f32_pairs_ok(d) && br >= 2 && !(br & 1) && d.n % 32 == 0) {
    const int64_t t64 = (d.m % 64 == 0 && d.n % 64 == 0) ? (d.m / 64) * (d.n / 64) : 0;
    const int64_t t6432 = (d.m % 64 == 0) ? (d.m / 64) * (d.n / 32) : 0;
    if (t64 >= cus) return launch(GL_F32_LW_GROUPED, t64 >= 2 * cus ? 0 : 1);
    if (t6432 >= cus) return launch(GL_F32_LW_GROUPED, 2);
    return launch(GL_F32_LW_GROUPED, 3, "", choose_f32_split(3, (d.m / 32) * (d.n / 32), br / 2, env));
  }
  // a SINGLE invoke of a tile whose n ends inside a 32-column block (--tiles=64,48,64): the loader-wave kernel its group runs on
  if (f32_lw && d.k % BK == 0 && br >= 1 && d.n > 32 && d.n % 32 != 0)
    return launch(GL_F32_LW_GROUPED, 3, "", choose_f32_split(3, (d.m / 32) * ((d.n + 31) / 32), (long long)br * (d.k / BK), env));
  return generic(generic_kernel(d, g));
}

GemmLaunch plan_gemm_group(const GemmDesc &d, int n_items, bool vec_ok, bool out_ok, bool pair_ok, int64_t br_hint, const GemmPlanEnv &env) {
  if (d.m <= 0 || d.n <= 0 || n_items <= 0) return launch(GL_NONE);
  if (gemm_on_x6(d)) return launch(GL_INVALID); // the split kernel is never queued or grouped (try_enqueue, gemm_invoke_unqueued)
  const int64_t cus = env.cus;
  // n_dec: the number of items every size-dependent DECISION below is taken for. Normally the group's - the group is what fills the
  // chip. In strict mode 1: a single invoke, the first pass of a queued group and its replays then all run on the same kernel.
  const int64_t n_dec = env.strict ? 1 : n_items;
  if (d.b_trans || d.a_trans) return trans_launch(d, vec_ok, true);
  const GenericOk g = generic_ok(d, vec_ok);
  // f32 tiles with k a multiple of 64 (mlir-gen --tiles=64,64,64, the most common setting of the reference's
  // benchmark configs): the fast tile families in grouped mode, the largest tile that still yields about one
  // workgroup per CU over the whole work list (the same rule as pick_f32_variant)
  // ... and 32-k tiles (--tiles=32,32,32, the reference's MLP benchmark) when every batch count is even: the loader waves build a
  // 64-k chunk from the blocks of two batch elements (brgemm_f32_lw.hip, pair mode)
  const bool k_pairs = pair_ok && f32_pairs_ok(d);
  const bool f32_lw = g.vec && f32_lw_operands_ok(d);
  // (n that is not a multiple of 32 - the reference's --tiles=64,48,64 / 32,48,32 configs: the last 32-column tile of an item is
  // ragged, the loader-wave kernels clamp its loads and mask its stores; needs the 16-byte output pieces of out_ok and ldc % 4)
  // skinny groups - at most one 32x16 tile per CU over the whole work list: the half-width tiles (brgemm_f32_lw16.hip), every CU a
  // workgroup without a hand-off. 64-k tiles, or 32-k tiles whose n is not a multiple of 32 with even batch counts (--tiles=32,48,32);
  // plain 32x32x32 tiles stay on the pair kernel whatever the group size (a single invoke and its group add in the same order:
  // what tools/queue_fuzz.py checks bit for bit)
  {
    const int64_t t16 = (d.m % 32 == 0 && d.n % 16 == 0) ? n_dec * (d.m / 32) * (d.n / 16) : 0;
    const bool k_ok = (d.k % BK == 0 && d.k > 0) || (k_pairs && d.n % 32 != 0);
    if (f32_lw && out_ok && !d.generic_forced && t16 > 0 && t16 <= cus && k_ok && d.ldc % 4 == 0 && n_items <= 65535 &&
        !((d.k == 32 ? br_hint / 2 : br_hint * (d.k / BK)) >= 48 && d.n % 32 == 0 && d.k % BK == 0)) // (long reductions: the split 32x32 tiles below, as plan_gemm_call)
      return launch(GL_F32_LW16, 0, d.k == 32 ? "brgemm_f32_lw16<32x16,k4> grouped, 32-k pairs" : "brgemm_f32_lw16<32x16,k4> grouped");
  }
  const bool n_ragged = d.n % 32 != 0;
  const bool fam_ok = n_ragged ? (!d.generic_forced && d.n > 32 && (d.k % BK == 0 || k_pairs)) // (plan_gemm knows no tile for such an n: variant = generic)
                               : ((d.k % BK == 0 && d.variant != V_GENERIC) || (k_pairs && !d.generic_forced));
  if (f32_lw && d.m % 32 == 0 && fam_ok && n_items <= 65535 * 2) { // (grid.x carries the item index: x split)
    const bool pairs = d.k == 32;
    const int64_t t64 = (d.m % 64 == 0 && d.n % 64 == 0) ? n_dec * (d.m / 64) * (d.n / 64) : 0;
    const int64_t t6432 = (d.m % 64 == 0) ? n_dec * (d.m / 64) * ((d.n + 31) / 32) : 0;
    const int64_t t32 = n_dec * (d.m / 32) * ((d.n + 31) / 32);
    // the loader-wave kernels (brgemm_f32_lw.hip) in grouped mode
    if (t64 >= 2 * cus) return launch(GL_F32_LW_GROUPED, 0, pairs ? "brgemm_f32_lw<64x64> grouped, 32-k pairs" : "brgemm_f32_lw<64x64> grouped");
    if (t64 >= cus) return launch(GL_F32_LW_GROUPED, 1, pairs ? "brgemm_f32_lw<64x64,k2> grouped, 32-k pairs" : "brgemm_f32_lw<64x64,k2> grouped");
    // (rounds of workgroups x per-chunk time, as pick_f32_variant: 1.5 rounds of 64x32 tiles lose to 3 half-rounds of 32x32 tiles)
    if (t6432 >= cus && !f32_32x32_beats_64x32(t32, t6432, cus))
      return launch(GL_F32_LW_GROUPED, 2, pairs ? "brgemm_f32_lw<64x32,k4> grouped, 32-k pairs" : "brgemm_f32_lw<64x32,k4> grouped");
    // skinny groups (fewer 64x32 tiles than CUs): 32x32 tiles, and the batch-reduce range of a tile over several workgroups
    // when the model says so (choose_f32_split: from the descriptor, the first item's batch count and the group's size)
    const int64_t chunks = pairs ? br_hint / 2 : br_hint * (d.k / BK);
    const int S = choose_f32_split(3, t32, chunks, env);
    if (S > 1) return launch(GL_F32_LW_GROUPED, 3, pairs ? "brgemm_f32_lw<32x32,k4> grouped, 32-k pairs, split" : "brgemm_f32_lw<32x32,k4> grouped, split", S);
    return launch(GL_F32_LW_GROUPED, 3, pairs ? "brgemm_f32_lw<32x32,k4> grouped, 32-k pairs" : "brgemm_f32_lw<32x32,k4> grouped");
  }
  // bf16 tile invokes with k a multiple of 64 and n a multiple of 64 (the reference's --tiles=64,64,64 / 32,64,64 bf16 rows): the
  // LOADER-WAVE tiles in grouped mode (round 6, brgemm_bf16_lw.hip launch_bf16_lw_grouped) - what the same layer runs on as one
  // whole-layer call. Tile by the blw_cost model over the group's workgroups: 32x64 + K2 (two workgroups per 64-row item) or 64x64.
  // Against the two older grouped kernels (profiles/r06_bf16_sweep_before.txt, forced-variant rows): the loader-wave tiles win whenever
  // the group fills 3/4 of the chip with 64x64 tiles (1024 x 1024 x 512: 5.1 us against 6.7) or the reduction is long (16 chunks or
  // more: 128 x 4096 x 1024 5.3 against 9.4) or half the chip gets a 32x64 tile of at least 8 chunks (128 x 3072 x 768: 4.9 against
  // 6.3; 1024 x 512 x 256, 4 chunks: 5.6 against 5.1); short reductions of small groups stay on the K-split kernel (128 x 768 x 768:
  // 4.3 against 4.7). (A forced split count: the K-split kernel below.)
  {
    const bool v2 = d.vnni_factor == 2, v4 = d.vnni_factor == 4;
    const bool lw_ok = (v2 || v4) && bf16_lw_items_ok(d, v4) && vec_ok && out_ok && br_hint >= 1 && env.forced_split < 0;
    const int64_t chunks = br_hint * (d.k / BK);
    const int b_kind = v4 ? 4 : 0;
    const bool even = ((d.k / BK) % 2 == 0) || pair_ok;
    // RAGGED n (round 6): items whose n is 16 more than a multiple of 32 - the reference's --tiles=64,48,64 rows (fc / matmul 128x768x2304)
    // - on the 32x32 + K2 instance: ceil(n / 32) column tiles per item, the last moved left to end at column n (it recomputes the 16
    // columns it shares with its neighbour and stores its own 16: brgemm_bf16_lw.hip skip_cols). Skinny groups with a long reduction
    // only, like the instance's other uses; everything else with such an n stays on the K-split kernel below.
    if (lw_ok && d.n % 32 == 16 && d.n >= 48 && n_dec * (d.m / 32) * ((d.n + 31) / 32) <= cus && chunks >= 16) {
      return launch(GL_BF16_LW_GROUPED, 4, v4 ? "brgemm_bf16_lw_vnni4<32x32,k2> grouped, ragged n" : "brgemm_bf16_lw<32x32,k2> grouped, ragged n", 1, b_kind, even);
    }
    const int64_t t64 = d.m % 64 == 0 ? n_dec * (d.m / 64) * (d.n / 64) : 0;
    const int64_t wg0 = n_dec * (d.m / 32) * (d.n / 64);
    if (lw_ok && d.n % 64 == 0 && (t64 * 4 >= 3 * cus || chunks >= 16 || (wg0 * 2 >= cus && chunks >= 8))) {
      const double c0 = blw_cost(0, rounds(wg0, cus), (double)chunks);
      const double c1 = t64 > 0 ? blw_cost(1, rounds(t64, cus), (double)chunks) : 1e30;
      int tile = c1 <= c0 ? 1 : 0;
      // 32x32 + K2 (VNNI-2): twice the workgroups of the 32x64 tile pulling panels - for skinny groups with a long reduction, as
      // plan_gemm_call does for the whole-layer call (one round of workgroups at most, 16 chunks or more)
      if (n_dec * (d.m / 32) * (d.n / 32) <= cus && chunks >= 16 && blw_cost(4, 1, (double)chunks) < (c1 < c0 ? c1 : c0)) tile = 4;
      static const char *const names[2][3] = {
          {"brgemm_bf16_lw<32x64,k2> grouped", "brgemm_bf16_lw<64x64> grouped", "brgemm_bf16_lw<32x32,k2> grouped"},
          {"brgemm_bf16_lw_vnni4<32x64,k2> grouped", "brgemm_bf16_lw_vnni4<64x64> grouped", "brgemm_bf16_lw_vnni4<32x32,k2> grouped"}};
      return launch(GL_BF16_LW_GROUPED, tile, names[v4 ? 1 : 0][tile == 4 ? 2 : tile], 1, b_kind, even);
    }
  }
  // bf16 tiles of 64x64 with k a multiple of 64: the 64x64 bf16 family in grouped mode (it stores 16-byte
  // row pieces and reads the bias 8 bytes at a time: checked per item by the queue through out_ok)
  // (whatever a SINGLE invoke of the handle would run on - a lone 64x64 tile is planned on the 32x32 K-split kernel -, the GROUP is
  // what fills the chip: round 5, the reference's fc / matmul shapes as 64,64,64 tile invokes: 1024 x 2560 x 1024 30.4 us on 32x32
  // tiles against 15 us whole-layer)
  const bool fills64 = n_dec * (d.m / 64) * (d.n / 64) >= (3 * cus) / 4;
  if (g.vec16 && out_ok && d.variant >= V_BF16_FAST && (d.variant != V_BF16_SMALL32 || !d.variant_forced) && !d.generic_forced && bf16_fast_eligible(d) && fills64)
    return launch(GL_BF16_GROUPED64, 0, "brgemm_bf16_fast<64x64> grouped");
  // ... and the same family on a VNNI-4 B operand (--vnni=4 tile invokes: benchmarks/config/*/*_dp4_*; the generic kernel's MFMA path
  // took 30 us for 1024 x 2560 x 1024 against 19.5 on VNNI-2)
  if (g.vec16_4 && out_ok && !d.generic_forced && !d.vnni_c && d.k % BK == 0 && d.m % 64 == 0 && d.n % 64 == 0 && !((d.ldc | d.stride_b) & 7) && d.ldc < (1 << 22) &&
      d.lda < (1 << 22) && d.ldb < (1 << 20) && fills64)
    return launch(GL_BF16_GROUPED64, 0, "brgemm_bf16_fast_vnni4<64x64> grouped");
  // (VNNI-4 tile invokes - the compiler-native 32x32x32 tiles of a --vnni=4 pipeline, small groups of 64x64x64 tiles - on the same
  // kernel: its B fragment is then two 8-byte loads; a single invoke of such a handle stays on the generic kernel's MFMA path.
  // And tiles whose n is a multiple of 4 but not of 32 (--tiles=64,48,64): a masked last column tile instead of the generic kernel.)
  const bool small_base = bf16_small_operands_ok(d) && !d.vnni_c && !d.generic_forced && d.n >= 32 && d.n % 4 == 0;
  const bool small4 = small_base && d.vnni_factor == 4 && !(d.stride_b & 3);
  const bool small_ragged = small_base && d.vnni_factor == 2 && d.n % 32 != 0 && !(d.stride_b & 1);
  if (vec_ok && out_ok && ((d.variant != V_GENERIC && bf16_small_eligible(d)) || small_ragged || small4)) {
    // skinny groups with a long reduction: the K steps of a tile over several workgroups (choose_bf16_small_split)
    const int S = choose_bf16_small_split((long long)n_dec * (d.m / 32) * ((d.n + 31) / 32), (long long)br_hint * (d.k / 16), env);
    const char *unsplit = small4 ? "brgemm_bf16_small32_vnni4 grouped" : "brgemm_bf16_small32 grouped";
    GemmLaunch l = launch(GL_BF16_SMALL32, 0, S > 1 ? (small4 ? "brgemm_bf16_small32_vnni4 grouped, split" : "brgemm_bf16_small32 grouped, split") : unsplit, S);
    l.text_unsplit = unsplit;
    return l;
  }
  static const char *const names[] = {"brgemm_grouped<f32>", "brgemm_grouped<f32>", "brgemm_grouped<bf16,vnni2>", "brgemm_grouped<bf16,vnni2>",
                                      "brgemm_grouped<bf16,vnni4>", "brgemm_grouped<bf16,flat>"};
  return generic(generic_kernel(d, g), names[generic_kernel(d, g)]);
}

bool gemm_quads_pay(const GemmDesc &d, int n_items, int64_t br, const GemmPlanEnv &env) {
  if (env.strict || !quads_shape_ok(d) || br < 1 || n_items < 4 || (n_items & 3) || env.forced_split >= 0) return false;
  const double chunks = (double)(br * (d.k / BK));
  const int64_t cus = env.cus;
  // the 64x64 and 32x64 + K2 tiles - what the grouped path would pick from - against 128x128 blocks of four items
  const double c64 = blw_cost(1, rounds(n_items, cus), chunks), c32 = blw_cost(0, rounds(2 * (int64_t)n_items, cus), chunks);
  const double cq = blw_cost(3, rounds(n_items / 4, cus), chunks);
  return cq * 1.05 < (c64 < c32 ? c64 : c32);
}

GemmLaunch plan_gemm_quads(const GemmDesc &d, int n_quads, int64_t br) {
  if (!quads_shape_ok(d) || br < 1 || n_quads <= 0) return launch(GL_INVALID);
  const bool v4 = d.vnni_factor == 4;
  return launch(GL_BF16_LW_QUADS, 0, v4 ? "brgemm_bf16_lw_vnni4<128x128> quads" : "brgemm_bf16_lw<128x128> quads", 1, v4 ? 4 : 0);
}

} // namespace tpp
