// gemm_plan.h - which GEMM kernel runs a call: the variant a descriptor is planned on at dispatch (plan_gemm), the launch an invoke or a
// tile-queue group gets (plan_gemm_call, plan_gemm_group), the one launch a layer chain gets (plan_chain: the entry of the chain rules below).
// Host-only, every input an argument: the table of choices is checked on a CPU (tests/golden/gemm_plan.txt, chain_dispatch.txt).
// brgemm_f32.hip carries a GemmLaunch out, rt_chain.h try_chain_launch a ChainLaunchPlan.
#pragma once
#include "xsmm_desc.h"

namespace tpp {

enum GemmVariant : int {
  V_F32_64x64 = 0,   // brgemm_f32.hip register-staged tiles: 4 waves 2x2x1
  V_F32_64x32K2 = 1, // 4 waves 2x1x2
  V_F32_32x32K4 = 2, // 4 waves 1x1x4
  V_F32_128x64 = 3,  // 8 waves 4x2x1
  V_F32_64x64K2 = 4, // 8 waves 2x2x2 (two waves per SIMD share every K chunk)
  V_F32_LW_64x64 = 5,     // brgemm_f32_lw.hip: 4 MFMA waves 2x2x1 + 2 loader waves
  V_F32_LW_64x64K2 = 6,   // 8 MFMA waves 2x2x2 + 2 loader waves
  V_F32_LW_64x32K2 = 7,   // 8 MFMA waves 2x1x4 + 2 loader waves (K split over four groups since round 3; the name of the constant stayed)
  V_GENERIC = 8,     // chosen per invoke when the fast preconditions fail
  V_F32_LW_32x32K4 = 9,   // 4 MFMA waves 1x1x4 + 2 loader waves
  V_F32_LW_128x64 = 10,   // 8 MFMA waves 4x2x1 + 2 x 2 loader waves, 3-slot ring (large outputs)
  V_F32_LW16_32x16 = 11,  // brgemm_f32_lw16.hip: 32x16 tiles on v_mfma_f32_16x16x4_f32, 4 MFMA waves (K split) + 3 loader waves: outputs of at most one 32x16 tile per CU
  V_F32_X6_64x64 = 12,    // brgemm_f32_x6.hip: the bf16x6 split on v_mfma_f32_32x32x16_bf16 (f32 descriptors dispatched under xsmm_hip_set_f32_precision(6)
  V_F32_X6_64x32K2 = 13,  //   with this variant forced: plan_gemm); 4 waves, K split over the rest of them; 128x64 with 8 waves
  V_F32_X6_32x32K4 = 14,
  V_F32_X6_128x64 = 15,
  V_BF16_FAST = 16,  // brgemm_bf16.hip: 64x64 register-staged
  V_BF16_DMA128 = 17, // brgemm_bf16.hip: 128x128, LDS-DMA + loader waves
  V_BF16_DMA256 = 18, // brgemm_bf16_dma256.hip: 256x256, LDS-DMA
  V_BF16_SMALL32 = 19, // brgemm_bf16_small.hip: 32x32 tiles, 4 waves split K, fragments straight from global memory
  V_BF16_LW_32x64 = 20,   // brgemm_bf16_lw.hip: loader-wave tiles for mid-size outputs (one workgroup per CU), 32x64 + K2
  V_BF16_LW_64x64 = 21,
  V_BF16_LW_64x128 = 22,
  V_BF16_LW_128x128 = 23,
  V_BF16_LWF_32x64 = 24,  // the same tiles for a FLAT bf16 B operand (no VNNI flag): the pair-row interleave happens in the B loader
  V_BF16_LWF_64x64 = 25,
  V_BF16_LWF_64x128 = 26,
  V_BF16_LWF_128x128 = 27,
  V_BF16_LW4_32x64 = 28,  // the same tiles for a VNNI-4 B operand [k/4][n][4] (xsmm_hip_set_vnni_factor(4)): a fragment is two 8-byte reads
  V_BF16_LW4_64x64 = 29,
  V_BF16_LW4_64x128 = 30,
  V_BF16_LW4_128x128 = 31,
};

// what the decisions read besides the descriptor: the device's compute units, xsmm_hip_set_strict, xsmm_hip_force_split (-1 = the
// split model) and xsmm_hip_set_tail_split (0 = off, 1 = the model, 2 .. 16 = that many workgroups per tail tile) and
// xsmm_hip_set_edge_tiles (0 = off, 1 = the f32 tile rule, 6 / 7 / 9 / 10 = that f32 GemmVariant's tile, 2 = the f32 and the bf16 tile rule, 20 .. 23 =
// that bf16 GemmVariant's tile) and xsmm_hip_set_edge_k (0 = off, 1 = the f32 tile rule, 6 / 7 / 9 / 10 = that GemmVariant's tile) and
// xsmm_hip_set_edge_k_bf16 (0 = off, 1 = the bf16 tile rule, 20 .. 23 = that bf16 GemmVariant's tile) and xsmm_hip_set_f32_halves (0 = off, 1 =
// the rule, 2 = wherever eligible) and xsmm_hip_set_edge_k8_bf16 (the values of edge_k_bf16, for k % 16 == 8) and xsmm_hip_set_dma256_images
// (0 = off, 1 = the rule, 2 = wherever eligible) and xsmm_hip_set_dma256_edge (the same values) and xsmm_hip_set_skinny_bf16 (0 = off, 1 = the
// rule, 16 / 32 / 64 = that column-block width wherever eligible) and xsmm_hip_set_skinny_split (0 = off, 1 = the rule, 2 .. 16 = that many parts
// wherever eligible); mode_switches.h gemm_plan_env_of fills it per call, and the accepted values of each switch stand in its table
struct GemmPlanEnv { int cus; bool strict; int forced_split; int tail_split = 0; int edge_tiles = 0; int edge_k = 0; int edge_k_bf16 = 0; int halves = 0; int edge_k8_bf16 = 0; int dma256_images = 0; int dma256_edge = 0; int skinny_bf16 = 0; int skinny_split = 0; };

// pointer facts of one invoke: A and B 16-byte aligned, C 16- / 8-byte aligned, the bias row D 8- / 16-byte aligned
struct GemmAlign { bool ab16, c16, c8, d8, d16; };

// which launcher runs a call (brgemm_f32.hip run_gemm_launch) and with what
enum GemmLauncher : int {
  GL_NONE,            // nothing to compute (empty output or work list): hipSuccess
  GL_INVALID,         // no kernel takes this call: hipErrorInvalidValue
  GL_F32_FAST,        // brgemm_f32_fast (brgemm_f32.hip): tile = V_F32_64x64 .. V_F32_64x64K2
  GL_F32_LW,          // launch_f32_lw(tile); halves: launch_f32_lw_halves first; split > 1: launch_f32_lw_split(tile, split) first; tail_tiles > 0: launch_f32_lw_tail first; edge: launch_f32_lw_edge(tile); edge_k: launch_f32_lw_kedge(tile)
  GL_F32_LW16,        // launch_f32_lw16(tile); split > 1: launch_f32_lw_split(3, split) first
  GL_F32_LW_GROUPED,  // launch_f32_lw_grouped(tile, split)
  GL_F32_X6,          // launch_f32_x6(tile, vec)
  GL_BF16_FAST,       // launch_gemm_bf16_fast(tile); b_kind 2 / 4 (xsmm_hip_set_dma256_images): launch_bf16_dma256_image(b_kind), tile 2 only; edge (xsmm_hip_set_dma256_edge): launch_bf16_dma256_edge(b_kind), tile 2 only
  GL_BF16_SMALL32,    // launch_bf16_small32(split)
  GL_BF16_GROUPED64,  // launch_bf16_grouped64
  GL_BF16_LW,         // launch_bf16_lw(mode, tile, b_kind); mode (brgemm_bf16_lw_launch.h): BLW_LAYER; edge: BLW_EDGE; edge_k: BLW_KEDGE; edge_k8: BLW_KEDGE8
  GL_BF16_LW_GROUPED, // launch_bf16_lw_grouped(tile, b_kind, even)
  GL_BF16_LW_QUADS,   // launch_bf16_lw_quads(b_kind)
  GL_GENERIC,         // brgemm_grouped<T, VNNI, VEC, VF, FORM>: generic
  GL_BF16_SKINNY,     // launch_bf16_skinny(b_kind, tile): tile = the column-block width BN 16 / 32 / 64 (xsmm_hip_set_skinny_bf16; brgemm_bf16_skinny.hip); split > 1 (xsmm_hip_set_skinny_split): launch_bf16_skinny_split(b_kind, tile, split) first
};
// the instances of the generic kernel brgemm_grouped<T, VNNI, VEC, VF>: <float, false, false / true>, <unsigned short, true, false / true>,
// <unsigned short, true, true, 4>, <unsigned short, false, false>; and the f32 instances whose FORM argument says that an operand is
// read transposed (mode 2 of xsmm_hip_set_fold_transpose): <float, false, true, 2, B transposed>, <float, false, true / false, 2, A transposed>
enum GemmGeneric : int { GG_F32, GG_F32_VEC, GG_BF16_VNNI2, GG_BF16_VNNI2_VEC, GG_BF16_VNNI4_VEC, GG_BF16_FLAT, GG_F32_BT_VEC, GG_F32_AT_VEC, GG_F32_AT };
struct GemmLaunch {
  GemmLauncher launcher;
  int tile;        // the launcher's tile index (GL_BF16_SKINNY: the column-block width BN)
  int split;       // workgroups per output tile (1 = none; GL_BF16_SKINNY: the parts P_eff of a column block)
  int b_kind;      // B image of the bf16 loader-wave tiles and of the 256x256 tile: 0 VNNI-2, 2 flat, 4 VNNI-4
  bool even;       // GL_BF16_LW_GROUPED: every item has an even chunk count
  bool vec;        // GL_F32_X6: A and B 16-byte aligned
  GemmGeneric generic;
  const char *text; // what xsmm_hip_last_refined_kernel (a call) / xsmm_hip_last_grouped_kernel (a group) reports, a static string
  // GL_F32_LW, tail split (xsmm_hip_set_tail_split): the last tail_tiles output tiles - the partial last round of workgroups - run on
  // tail_split workgroups each, the tiles of the full rounds unsplit, all in one launch (0 / 1 = none)
  int tail_tiles = 0;
  int tail_split = 1;
  // GL_F32_LW / GL_BF16_LW, edge tiles (xsmm_hip_set_edge_tiles): m or n is not a multiple of the tile - launch_f32_lw_edge(tile) /
  // launch_bf16_lw(BLW_EDGE, tile, b_kind) on the ceil-divided tile grid; refused by the launcher: the launch the call has with the mode off.
  // GL_BF16_FAST, tile 2 (xsmm_hip_set_dma256_edge): m or n is not a multiple of 256 - launch_bf16_dma256_edge(b_kind), refused the same way
  bool edge = false;
  // GL_F32_LW, ragged k (xsmm_hip_set_edge_k): k is a multiple of 8 but not of 64 - launch_f32_lw_kedge(tile) on the ceil-divided tile
  // grid (m and n may be ragged too); refused by the launcher: the launch the call has with the mode off.
  // GL_BF16_LW (xsmm_hip_set_edge_k_bf16): k is a multiple of 16 but not of 64 - launch_bf16_lw(BLW_KEDGE, tile, b_kind), the same way
  bool edge_k = false;
  // GL_BF16_LW, ragged k in half steps (xsmm_hip_set_edge_k8_bf16): k is a multiple of 8 but not of 16 - launch_bf16_lw(BLW_KEDGE8, tile,
  // b_kind), refused the same way. Never set together with edge_k.
  bool edge_k8 = false;
  // GL_F32_LW, tile 1, halves (xsmm_hip_set_f32_halves): every 64x64 + K2 tile as two 64x32 + K2 workgroups - launch_f32_lw_halves, the
  // same bits; refused by the launcher: launch_f32_lw(1). Variant, kernel name and text are those of the launch with the mode off.
  bool halves = false;
  // GL_BF16_SMALL32 with split > 1: what a group reports when its stream has no scratch block (a 17th stream, a stream being captured
  // into a graph) and launch_bf16_small32 ran the unsplit launch instead
  const char *text_unsplit = nullptr;
};

// fills d.variant / d.name / d.generic_forced / d.variant_forced; returns false if no kernel can run the descriptor
bool plan_gemm(GemmDesc &d, int forced_variant, const GemmPlanEnv &env);
// one invoke of a planned descriptor with batch count br (launch_gemm). The refinements in order of precedence, each with the switches it reads
// besides the descriptor, the call, the CU count and forced_split - pinned under every switch set by tests/test_gemm_call_switches.py: dma256 edge
// {dma256_edge}, bf16 edge tiles {edge_tiles}, bf16 ragged k {edge_k_bf16, edge_tiles}, half-step ragged k {edge_k8_bf16, edge_tiles}, dma256 images
// {dma256_images}, f32 edge tiles {edge_tiles}, f32 ragged k {edge_k, edge_tiles}, tail split {tail_split}, halves {halves}; plan_gemm reads none.
// Skinny-batch bf16 layers {skinny_bf16} stand outside that list: they take bf16 calls with m < 32 planned on the generic kernel, which
// no other refinement takes (each asks for m >= 32), so the partition depends on the descriptor alone (tests/test_gemm_plan_skinny.py).
// The K split across workgroups of such a launch, xsmm_hip_set_skinny_split {skinny_split, skinny_bf16}, is read INSIDE that block only - for
// a call already put on GL_BF16_SKINNY - and sets split and text, nothing else: with skinny_bf16 at 0 it is never read, BN and the m >= 17
// gate do not read it, and no other refinement does (tests/test_gemm_plan_skinny_split.py).
GemmLaunch plan_gemm_call(const GemmDesc &d, int64_t br, const GemmAlign &al, const GemmPlanEnv &env);
// n_items invokes of one descriptor in one launch (launch_gemm_grouped; vec_ok / out_ok / pair_ok / br_hint as there)
GemmLaunch plan_gemm_group(const GemmDesc &d, int n_items, bool vec_ok, bool out_ok, bool pair_ok, int64_t br_hint, const GemmPlanEnv &env);
// n_quads 2 x 2 blocks of 64x64 items on the 128x128 loader-wave tile (launch_gemm_quads)
GemmLaunch plan_gemm_quads(const GemmDesc &d, int n_quads, int64_t br);
// would the group run faster as 2 x 2 blocks (xsmm_desc.h gemm_quads_pay)
bool gemm_quads_pay(const GemmDesc &d, int n_items, int64_t br, const GemmPlanEnv &env);

// planned on the bf16x6 split kernel (brgemm_f32_x6.hip: variants 12 .. 15). Such handles are never queued, grouped, chained or given a
// folded transpose; a bf16x6 descriptor planned on an exact kernel (a shape the split kernel does not take) goes every way a mode-0 one goes
inline bool gemm_on_x6(const GemmDesc &d) { return d.variant >= V_F32_X6_64x64 && d.variant <= V_F32_X6_128x64; }
// which B image of the loader-wave bf16 tiles (brgemm_bf16_lw.hip) a descriptor's B operand needs - 0: VNNI-2, 2: flat [k][ldb],
// 4: VNNI-4 - or -1 if the descriptor cannot run on those tiles (shape / alignment / lane-offset limits of the LDS-DMA panels)
int bf16_lw_b_kind(const GemmDesc &d);
// RAGGED-m CHAINS (xsmm_hip_set_chain_edge; plan_chain, brgemm_bf16_lw.hip launch_bf16_chain, BLW_CHAIN_EDGE). Host-only, no HIP calls:
// tests/golden/gemm_plan_chain_edge.txt is the table of both functions' answers.
// One call of a chain: the B image (0 VNNI-2, 2 flat, 4 VNNI-4) it would run with as a layer of a ragged-m chain - what bf16_lw_b_kind asks of
// leading dimensions, strides and lane offsets without its m and n terms -, or -1 and *why: the switch is off, an f32 call, a VNNI C,
// beta 1, a forced kernel (xsmm_hip_force_variant, the generic kernel included), k not in 64-k chunks, an operand off the LDS-DMA grid.
int chain_edge_b_kind(const GemmDesc &d, int chain_edge, const char **why);
// The tile of the ONE launch: m x n outputs per layer, nlayers layers of k[l] per batch element and br[l] batch elements, cus compute
// units on the stream, forced_tile 0 .. 3 = the tile xsmm_hip_set_edge_tiles(20 .. 23) names (-1: none), strict = xsmm_hip_set_strict.
// A tile FITS when m >= BM, n % BN == 0 and ceil(m / BM) * (n / BN) <= cus (every workgroup resident at once). The forced tile if it
// fits, else the smallest of tiles 0 .. 3 that fits. tile = -1 and why = the NOCHAIN reason: strict mode (the chain tile is no function
// of the descriptor alone), fewer than 2 or more than 8 layers, a k % 64 or an empty batch, no tile fits (m below every tile's rows, n
// not in whole column tiles, more tiles than compute units), or the chosen tile's rows divide m (not a ragged chain: the divisible
// chain's rules decide).
struct ChainEdgePlan { int tile; const char *why; };
ChainEdgePlan plan_chain_edge(int64_t m, int64_t n, int nlayers, const int64_t *k, const int64_t *br, int64_t cus, int forced_tile, bool strict);
// RAGGED-WIDTH CHAINS (xsmm_hip_set_chain_ragged; plan_chain, brgemm_bf16_lw_chain_ragged.hip launch_bf16_chain_ragged,
// BLW_CHAIN_RAGGED, schedule in brgemm_bf16_lw_chain_ragged.h). Host-only, no HIP calls: tests/golden/gemm_plan_chain_ragged.txt is the table of
// both functions' answers.
// One call of a chain: the B image (0 VNNI-2, 2 flat, 4 VNNI-4) it would run with as a layer of a ragged-width chain - what chain_edge_b_kind
// asks, with the k term replaced by "k >= 64 and k % 8 == 0" (whole, a multiple of 16, or a multiple of 8 per layer) -, or -1 and *why: the
// switch is off, an f32 call, a VNNI C, beta 1, a forced kernel (the generic kernel included), such a k, an operand off the LDS-DMA grid.
int chain_ragged_b_kind(const GemmDesc &d, int chain_ragged, const char **why);
// The tile of the ONE launch: arguments as plan_chain_edge's + mode = the switch's value and b_kind = the B image every call has. A tile
// FITS when its instance exists (blw_chain_ragged_instance_exists: not 64x128 with VNNI-2), m >= BM, n >= BN and ceil(m / BM) * ceil(n / BN)
// <= cus. The forced tile if it fits, else the smallest of tiles 0 .. 3 that fits. tile = -1 and why = the reason: the switch off, strict
// mode, fewer than 2 or more than 8 layers, a k below 64 or not a multiple of 8, an empty batch, n % 8 != 0, no tile fits (m or n below
// every tile, more tiles than compute units - the multi-round switch never combines with this one), or nothing is ragged in width on the
// chosen tile - n % BN == 0 and every k % 64 == 0: a chain ragged in m alone is plan_chain_edge's, a divisible one the plain chain's.
// THE GATE (measured, profiles/chain_ragged_ab.txt): a chain whose tile by the rule would be 64x128 but whose B image has no instance of it
// (VNNI-2) and that would land on 128x128 stays call by call - 2000 rows x 1000 ran 13 % slower as one launch there; and a chain with a whole-k layer of an even chunk count on the
// 32x64 or 64x64 tile stays call by call too - that layer runs two chunks per barrier as a single call, one in this mode: 1024 rows x [1024,
// 1000, 1000] ran 3.5 % slower. Under a forcing edge-tile mode (forced_tile >= 0: tests, measurements) nothing is gated.
struct ChainRaggedPlan { int tile; const char *why; };
ChainRaggedPlan plan_chain_ragged(int64_t m, int64_t n, int nlayers, const int64_t *k, const int64_t *br, int64_t cus, int forced_tile, int b_kind, int mode, bool strict);
// MULTI-ROUND CHAINS (xsmm_hip_set_chain_rounds; plan_chain, brgemm_bf16_lw.hip launch_bf16_chain, BLW_CHAIN_ROUNDS, step maps in
// brgemm_bf16_lw_chain_rounds.h). Host-only, no HIP calls: tests/golden/gemm_plan_chain_rounds.txt is the table of the function's answers.
// A bf16 chain that meets every condition of the divisible chain but has MORE output tiles than compute units runs as one launch on
// G x tiles_n resident workgroups, G row groups walking R = ceil(tiles_m / G) rounds of row blocks. m x n outputs per layer, nlayers layers
// of k[l] per batch element and br[l] batch elements, cus compute units on the stream, planned_tile 0 .. 3 = the loader-wave tile ALL calls
// were planned on (-1: they do not share one, -2: a call is not bf16 - chain_rounds_planned_tile), mode = the switch's value, strict =
// xsmm_hip_set_strict.
//   tile:   the planned tile; without one, refused in strict mode, else the largest tile whose rows divide m and whose columns divide n.
//           (Strict mode may take the rule on the planned tile: the tile is the descriptors' own, and G changes no bit.)
//   groups: Gmax = cus / tiles_n rounded down. mode 1 applies only where tiles_m > Gmax (a chain that fits is the divisible chain's):
//           R = ceil(tiles_m / Gmax), G = ceil(tiles_m / R) - as few rounds as fit, balanced. mode 1000 + G: that G if 1 <= G < tiles_m and
//           G * tiles_n <= cus.
// tile = -1, groups = 0 and why = the reason: the switch off, an f32 call, fewer than 2 or more than 8 layers, a k % 64 or an empty batch, strict
// mode without a shared tile, m or n not in whole tiles, a row of tiles wider than the compute units, a chain that fits in one round
// (mode 1), a forced G that does not fit.
// THE GATE (mode 1 only; measured, profiles/chain_rounds_ab.txt: three 1024-wide VNNI-2 layers on 256 CUs, call by call -> one launch:
// 4224 rows R = 2 62.45 -> 49.35 us, 8192 rows R = 2 60.34 -> 53.81, but 16384 rows R = 4 99.61 -> 104.23 and 32768 rows R = 8
// 193.09 -> 217.89 - the calls of such batches run on the 256x256 tile, which the chain has no form of): a chain of MORE THAN TWO
// rounds stays call by call. The answer then still names the rule's tile and groups, with gated = true and why = the gate: the caller
// does not launch. A forced G is not gated.
struct ChainRoundsPlan { int tile; int groups; const char *why; bool gated; };
constexpr int CHAIN_ROUNDS_GATE = 2; // most rounds mode 1 takes
inline bool chain_rounds_mode_forced(int mode) { return mode > 1000; }
// the loader-wave tile 0 .. 3 all n calls of a chain were planned on (variants 20 .. 23 VNNI-2, 24 .. 27 flat B, 28 .. 31 VNNI-4: the same
// four tiles, one B image); -1: they do not share one; -2: a call is not bf16
int chain_rounds_planned_tile(int n, const GemmDesc *const *d);
// One call of a chain under a FORCED G, which is asked in front of the one-round rules: the B image (0 VNNI-2, 2 flat, 4 VNNI-4) of the
// call as a layer of the multi-round launch - what bf16_lw_b_kind asks of leading dimensions, strides and lane offsets WITHOUT its m and n
// terms (the rule itself asks for m and n in whole tiles: 5 x 32 rows of VNNI-2 run on the 32x64 tile) - or -1: an f32 call, a VNNI C,
// beta 1, the generic kernel, k not in 64-k chunks, an operand off the LDS-DMA grid.
int chain_rounds_b_kind(const GemmDesc &d);
ChainRoundsPlan plan_chain_rounds(int64_t m, int64_t n, int nlayers, const int64_t *k, const int64_t *br, int64_t cus, int planned_tile, int mode, bool strict);
// MIXED-WIDTH CHAINS (xsmm_hip_set_chain_widths; plan_chain, brgemm_bf16_lw_chain_widths.hip launch_bf16_chain_widths,
// BLW_CHAIN_WIDTHS, schedule in brgemm_bf16_lw_chain_widths.h). Host-only, no HIP calls: tests/golden/gemm_plan_chain_widths.txt is the table
// of the function's answers. A bf16 chain of 2 .. 8 calls with the same m whose n differ runs as one launch on m / BM x max_l(n[l] / BN)
// workgroups. n[l], k[l], br[l]: layer l's columns, k per batch element and batch count; cus: compute units on the stream; planned_tile
// 0 .. 3 = the loader-wave tile ALL calls were dispatched on (-1: they do not share one, -2: a call is not bf16 - chain_rounds_planned_tile);
// b_kind = the B image every call has by bf16_lw_b_kind (-1: none, or not one); mode = the switch's value; strict = xsmm_hip_set_strict.
// A tile FITS when BM divides m, BN divides every n[l] and m / BM * max_l(n[l] / BN) <= cus. The tile: the planned one if it fits (the
// launch then has the calls' bits: strict mode takes it too); without one, refused in strict mode, else the smallest tile that fits.
// tile = -1 and why = the reason: the switch off, an f32 call, fewer than 2 or more than 8 layers, no shared B image, a k not in 64-k
// chunks or an empty batch, every n equal (the plain chain's), strict mode without a planned tile that fits, m or an n no tile divides
// (ragged shapes never combine with different widths), more tiles than compute units (nor do several rounds).
// THE GATE (measured, profiles/chain_widths_ab.txt): where the tile is the smallest that fits - not one all calls were dispatched on - and
// some layer ALONE (m x n[l]) fits a smaller tile, the chain stays call by call: that layer's separate call covers the chip with more,
// smaller tiles, in the launch it keeps a fraction of the grid busy on the widest layer's tile. 1024 and 256 rows x [1024, 4096, 1024],
// 2048 rows x [1024, 2048, 1024] and 1024 rows x [1024, 2048, 1024, 2048, 1024] ran 32 %, 18 %, 4 % and 9 % slower as one launch; the
// funnel [1024, 512, 256, 128], on the smallest tile, 28 % faster.
struct ChainWidthsPlan { int tile; const char *why; };
ChainWidthsPlan plan_chain_widths(int64_t m, int nlayers, const int64_t *n, const int64_t *k, const int64_t *br, int64_t cus, int planned_tile, int b_kind, int mode, bool strict);
// MIXED-WIDTH CHAINS IN COLUMN ROUNDS (xsmm_hip_set_chain_width_rounds; plan_chain, brgemm_bf16_lw_chain_wrounds.hip
// launch_bf16_chain_wrounds, BLW_CHAIN_WROUNDS, schedule in brgemm_bf16_lw_chain_wrounds.h). Host-only, no HIP calls:
// tests/golden/gemm_plan_chain_width_rounds.txt is the table of the function's answers. The mixed-width chain above on m / BM x W resident
// workgroups, 1 <= W < max_l(n[l] / BN): a workgroup walks several column tiles of a wide layer and one (or none) of a narrow one. The
// arguments are plan_chain_widths'. A tile FITS with W when BM divides m, BN divides every n[l], 1 <= W < max_l T_l (T_l = n[l] / BN) and
// m / BM * W <= cus. The tile's BALANCED W: Wfit = min(max T - 1, cus / (m / BM)), R = ceil(max T / Wfit), W = ceil(max T / R).
//   mode 1:        the planned tile if it fits with its balanced W (the launch then has the calls' bits: strict mode takes it too); else,
//                  never in strict mode, of the tiles 0 .. 3 that fit with their balanced W the one with the smallest
//                  sum_l ceil(T_l / W) * BLW_B[tile] * br[l] * k[l] / 64 - the K-loop time by the fitted per-chunk rates -, ties to the
//                  larger tile. A chain whose widest layer would fit in one round is offered too (R = 2).
//   mode 1000 + W: that W on the planned tile, without one on the smallest tile that fits with it. Never gated. A W that does not fit is a
//                  refusal: the caller decides as with the switch off.
// tile = -1, groups = 0 and why = the reason: the switch off, an f32 call, fewer than 2 or more than 8 layers, no shared B image, a k not
// in 64-k chunks, an empty batch, every n equal, strict mode without a planned tile (or with one that does not fit), m or an n no tile
// divides (ragged shapes never combine with this mode), more row blocks than compute units (no W >= 1 fits), nothing to round (no W < max T
// fits), a forced W that does not fit.
// THE GATE (mode 1 only; measured, profiles/chain_width_rounds_ab.txt: VNNI-2 on 256 CUs, call by call -> one launch in column rounds, us
// per step; n[] as the rule sees it - the block 1024 -> 4096 -> 1024 is the two calls n = [4096, 1024]). On a tile of the rule's OWN
// choice - not one all calls were dispatched on - no chain gained: n = [4096, 1024] at 256 rows 16.85 -> 21.60 (32x64, 8 x 32, two rounds
// of the wide layer), at 1024 rows 25.61 -> 34.04 (64x64, 16 x 16, four), at 2048 rows 44.19 -> 48.29 (128x128, 16 x 16, two), at 4096 rows
// 64.20 -> 68.65 (128x128, 32 x 8, four); 2048 rows x [2048, 1024] 22.68 -> 25.69 (64x128, 32 x 8); 1024 rows x [2048, 1024, 2048, 1024]
// 33.97 -> 37.98 (64x64, 16 x 16) - slower in every pair; the funnel 1024 rows x [512, 256, 128] (32x64, 32 x 4) ran 15.96 -> 16.24 in one
// session, slower in every pair, and 17.30 -> 16.56 in the next, faster in every pair (the launch took about the same time, the separate
// calls did not). The separate calls run every layer on the tile that suits it; the launch pins all of them to one, and every step pays a seam
// of about 2.4 us (the A panels of a step are requested behind its predecessor's epilogue) where a saved launch is worth about the
// tile's fixed cost (3.6 .. 6.1 us). So: WITHOUT A TILE ALL CALLS WERE DISPATCHED ON THE CHAIN STAYS CALL BY CALL. On such a tile the
// separate calls run on that tile too, and the launch gained in both sessions: 1024 rows x [4096, 1024] on 64x64 at the rule's W = 16
// 34.85 -> 34.08, 35.96 -> 35.18 and 36.23 -> 35.84 in three sessions (every pair); not gated. (W = 8 on the same tile: 35.92 -> 64.17 - fewer, longer
// walks cost more than they save; the rule takes the largest W that fits.) A gated answer still names the rule's tile and groups, with
// gated = true and why = the gate: the caller does not launch. A forced W is not gated.
struct ChainWidthRoundsPlan { int tile; int groups; const char *why; bool gated; };
inline bool chain_width_rounds_mode_forced(int mode) { return mode > 1000; }
ChainWidthRoundsPlan plan_chain_width_rounds(int64_t m, int nlayers, const int64_t *n, const int64_t *k, const int64_t *br, int64_t cus, int planned_tile, int b_kind, int mode, bool strict);
// RAGGED MIXED-WIDTH CHAINS (xsmm_hip_set_chain_widths_ragged; plan_chain, brgemm_bf16_lw_chain_wragged.hip
// launch_bf16_chain_wragged, BLW_CHAIN_WRAGGED, schedule in brgemm_bf16_lw_chain_wragged.h). Host-only, no HIP calls:
// tests/golden/gemm_plan_chain_widths_ragged.txt is the table of both functions' answers.
// One call of a chain: chain_ragged_b_kind's question under this switch - the B image (0 VNNI-2, 2 flat, 4 VNNI-4) the call would run with
// as a layer, or -1 and *why: the switch is off, an f32 call, a VNNI C, beta 1, a forced kernel (the generic kernel included), k below 64
// or not a multiple of 8, an operand off the LDS-DMA grid of the edge tiles.
int chain_widths_ragged_b_kind(const GemmDesc &d, int mode, const char **why);
// The tile of the ONE launch on ceil(m / BM) x max_l ceil(n[l] / BN) workgroups: arguments as plan_chain_widths', with forced_tile 0 .. 3 =
// the tile xsmm_hip_set_edge_tiles(20 .. 23) names (-1: none) in place of the planned tile, and b_kind = the B image every call has by
// chain_widths_ragged_b_kind. Takes 2 .. 8 layers with at least two different n, every k >= 64 and k % 8 == 0, every batch >= 1, every
// n[l] % 8 == 0, not in strict mode. THE PARTITION: a chain SOME tile divides entirely (BM | m, BN | every n[l], every k[l] % 64 == 0) is
// never this rule's - it is plan_chain_widths' / plan_chain_width_rounds', or call by call with those off -, and equal widths are the other
// three chain switches'. A tile FITS when m >= BM, every n[l] >= BN, its instance exists (blw_chain_wragged_instance_exists: not 64x128
// with VNNI-2, which would need scratch - that tile is passed over) and ceil(m / BM) * max_l ceil(n[l] / BN) <= cus. The forced tile if it
// fits, else the smallest that fits. tile = -1 and why = the reason: the switch off, strict mode, the layer count, no shared B image, such a
// k or an empty batch, an n % 8, every n equal, a chain some tile divides entirely, m or an n below every tile, more tiles than compute units.
// THE GATE (structural, plan_chain_widths': a chain in which some layer ALONE fits a smaller tile than the launch's stays call by call,
// unless an edge-tile mode forces the tile). Measured here too (profiles/chain_widths_ragged_ab.txt: VNNI-2 on 256 CUs, us per step): the
// widening chain 1000 rows x n = [2000, 1000] would launch on 128x128 (8 x 16; 64x128 has no VNNI-2 instance) while n = 1000 alone fits
// 64x64 - forced onto 128x128 the launch takes 29.79 against 30.93 for calls pinned to that tile, but the calls on the planner's own tiles
// take 21.79: +36.7 % as one launch. Gated, it runs 21.79 / 21.80 with the switch off / on. The six ungated rows - the funnels n = [512, 256,
// 128] at 1024 and 1000 rows with k0 = 784 and 1024, 512 rows x [256, 64, 256, 784], 1000 rows x [504, 248], 200 rows x [136, 72, 200], all
// on 32x64 - gained 15.9 .. 32.2 % in every pair: no further gate. A gated answer still names the rule's tile, with gated = true and
// why = the gate: the caller does not launch.
struct ChainWidthsRaggedPlan { int tile; const char *why; bool gated; };
ChainWidthsRaggedPlan plan_chain_widths_ragged(int64_t m, int nlayers, const int64_t *n, const int64_t *k, const int64_t *br, int64_t cus, int forced_tile, int b_kind, int mode, bool strict);
// LAYER CHAINS ON THE 256x256 TILE (xsmm_hip_set_chain_dma256; plan_chain, brgemm_bf16_dma256_chain.hip launch_bf16_dma256_chain,
// maps in brgemm_bf16_dma256_chain.h). Host-only, no HIP calls: tests/golden/gemm_plan_chain_dma256.txt is the table of the answers.
// One call of a chain: the B image (0 VNNI-2, 2 flat, 4 VNNI-4) it would have as a layer of this launch - bf16, beta 0, no VNNI C, not the
// forced generic kernel, k in 32-k chunks, leading dimensions, strides and lane offsets on the tile's grid - or -1; -2: an f32 call.
int chain_dma256_b_kind(const GemmDesc &d);
// Does the call run on the 256x256 tile as a single call TODAY? VNNI-2: it was dispatched on V_BF16_DMA256 (by plan_gemm's rule, or forced).
// Flat / VNNI-4: xsmm_hip_set_dma256_images (dma256_images, the only other mode this rule reads) is non-zero and plan_gemm_call's block
// takes the call - planned, not forced, on a loader-wave tile of its image, 256 divides m and n, mode 2 or pick_bf16_tile's rule.
bool chain_dma256_on_tile(const GemmDesc &d, int dma256_images);
// The launch: m x n outputs per layer, nlayers layers of k[l] per batch element and br[l] batch elements, cus compute units on the stream,
// all_on_tile = chain_dma256_on_tile of EVERY call, b_kind = the image every call has by chain_dma256_b_kind (-1: none or not one, -2: an
// f32 call), mode = the switch's value, strict = xsmm_hip_set_strict. tiles_m = m / 256, tiles_n = n / 256.
//   mode 1:        only where all_on_tile. Within the compute units: one round, groups = tiles_m. Otherwise Gmax = cus / tiles_n,
//                  R = ceil(tiles_m / Gmax), G = ceil(tiles_m / R) (chain_rounds_groups).
//   mode 2:        every eligible chain, groups as mode 1 (tests, measurements).
//   mode 1000 + G: G row groups, also on a chain that fits: 1 <= G <= tiles_m and G * tiles_n <= cus.
// take = false, groups = 0 and why = the reason: the switch off, an f32 call, fewer than 2 or more than 8 layers, no shared B image, 256
// not dividing m or n, a k not in 32-k chunks or an empty batch, a row of tiles wider than the compute units, strict mode unless
// all_on_tile (the launch then has the separate calls' bits: strict mode takes it), mode 1 without all_on_tile, a forced G that does not fit.
// THE GATE (mode 1 only; measured, profiles/chain_dma256_ab.txt: three layers on 256 CUs, call by call -> one launch, us per step: 1024-wide
// layers at 16384 rows 109.65 -> 108.56, at 32768 rows (R = 2) 214.65 -> 203.22, flat 110.19 -> 109.41, VNNI-4 109.20 -> 108.29; but 4096
// rows x 4096-wide layers, 16 x 16 tiles, 334.03 -> 337.64 in every pair): a chain of MORE THAN EIGHT column tiles (n > 2048) stays call by
// call. The answer then still names the plan, with gated = true and why = the gate: the caller does not launch. Modes 2 and 1000 + G
// are never gated.
struct ChainDma256Plan { bool take; int groups; const char *why; bool gated; };
constexpr int CHAIN_DMA256_GATE_TILES_N = 8; // most column tiles mode 1 takes
inline bool chain_dma256_mode_forced(int mode) { return mode > 1000; }
ChainDma256Plan plan_chain_dma256(int64_t m, int64_t n, int nlayers, const int64_t *k, const int64_t *br, int64_t cus, bool all_on_tile, int b_kind, int mode, bool strict);
// SKINNY-BATCH LAYER CHAINS (xsmm_hip_set_chain_skinny; plan_chain, brgemm_bf16_skinny_chain.hip launch_bf16_skinny_chain, schedule in
// brgemm_bf16_skinny_chain.h). Host-only, no HIP calls: tests/golden/gemm_plan_chain_skinny.txt is the table of both functions' answers.
// One call of a chain: the B image (0 VNNI-2, 2 flat, 4 VNNI-4) it would have as a layer of this launch - bf16, beta 0, no VNNI C, no forced
// generic kernel and no forced variant, lda / ldb / ldc / stride_a / stride_b multiples of 8 elements and not negative, lda >= k, ldb >= n,
// ldc >= n, lda and ldc below 2^24 (the leading-dimension and stride part of bf16_skinny_args_ok, and the launch's buffer offsets) - or
// -1 with *why set.
int chain_skinny_b_kind(const GemmDesc &d, const char **why);
// The ONE launch: m = the rows every call has, n / k / br per layer, cus = the stream's compute units, b_kind = the image every call has by
// chain_skinny_b_kind, mode = the switch's value, strict = xsmm_hip_set_strict. THE PARTITION: m <= 31 is this rule's alone - every other
// chain form asks for m >= 32 - and it takes nothing else. Takes 2 .. 8 layers with 1 <= m <= 31, every batch >= 1, per layer
// skn_shape_ok(m, n_l, k_l, br_l, BN) - n_l >= BN, n_l % 8 == 0, k_l >= 8, k_l % 8 == 0 - and an instance of (image, BN); widths may differ.
//   BN:  modes 16 / 32 / 64 and 1000 * G + BN: that BN. Mode 1: the smallest BN with an instance (16; flat 32) - measured the fastest on
//        every row that gained. No instance (flat with 16) or a layer narrower than BN: a refusal.
//   G:   min(max_l skn_blocks(n_l, BN), cus); a forced G as given if G <= cus, else a refusal.
// Strict mode refuses: the launch has the bits of the calls under xsmm_hip_set_skinny_bf16(BN), not of the calls as the descriptors were planned.
// THE GATE (mode 1 only; measured, profiles/chain_skinny_ab.txt: three layers on 256 CUs against the calls one by one under xsmm_hip_set_skinny_bf16(1)
// + xsmm_hip_set_skinny_split(1), us per step: 1024 -> [1024] * 3 at m 1 / 8 / 16 / 31 16.92 / 17.38 / 17.50 / 18.24 -> 11.77 / 12.92 / 13.62 / 17.71 on BN
// 16, the funnel 784 -> 512 -> 256 -> 128 15.41 .. 15.37 -> 10.58 .. 13.37 in every round; 4096 -> [4096] * 3 27.83 / 29.92 / 30.04 / 37.60 -> 31.87 / 34.12 /
// 36.03 / 45.12 on its best BN, flat and VNNI-4 likewise slower in every round): a chain with a layer of more than 2 MiB of B, and a chain
// with a flat or a VNNI-4 B - none of whose measured rows gained -, stays call by call; the rows and what was not measured stand at the
// rule in gemm_plan.cpp. The answer then names the plan with gated = true and why = the gate, and the caller does not launch. Forced
// modes are never gated. There is no m >= 17 gate: m = 31 gained in every round wherever m <= 16 did.
struct ChainSkinnyPlan { int bn; int groups; const char *why; bool gated; };
inline bool chain_skinny_mode_forced_g(int mode) { return mode >= 1000; }
ChainSkinnyPlan plan_chain_skinny(int64_t m, int nlayers, const int64_t *n, const int64_t *k, const int64_t *br, int64_t cus, int b_kind, int mode, bool strict);
// THE LAYER-CHAIN LAUNCH DECISION (rt_chain.h try_chain_launch carries the answer out): which of the ten launch forms runs n calls that
// the chain contract admits, on which tile, B image and group count - or that they run call by call, and which rule refused. Host-only:
// no HIP call, no global; the descriptors, the batch counts, the switches and a way to ask for the stream's compute units are arguments.
// tests/test_chain_dispatch.py pins the answers through the C-ABI under every switch set (tests/golden/chain_dispatch.txt).
// plan_chain composes the rules above. Each is asked at most once, in ONE order of precedence; behind each rule, the modes it reads:
//   0. skinny batches         plan_chain_skinny        {skinny}   asked in front of everything, and only with the switch non-zero, a bf16 first call
//      and m <= 31: no other form takes such a chain, and this rule takes no other. Where it refuses or gates, everything below is what it is
//      without this switch (call by call today).
//   1. the 256x256 tile      plan_chain_dma256        {dma256; dma256_images in mode 1}   asked first; where it takes the chain nothing else is read
//      (an f32 chain - every call on the K-split loader-wave tile of the first, within the compute units - reads no switch)
//   2. a forced G / a forced W  plan_chain_rounds {rounds = 1000 + G}, plan_chain_width_rounds {width_rounds = 1000 + W}: in front of the one-round rules
//   3. the plain chain on the loader-wave tile all calls were planned on, if it fits the compute units
//   4. mixed widths            plan_chain_widths        {widths}, then column rounds by rule plan_chain_width_rounds {width_rounds = 1}
//   5. one round on edge rows  plan_chain_edge          {edge; edge_tiles 20 .. 23} in front of several rounds plan_chain_rounds {rounds = 1};
//      several rounds on the PLANNED tile in front of the plain chain on another tile (the smallest that fits), on another tile behind both
//   6. ragged width            plan_chain_ragged        {ragged; edge_tiles}, then ragged mixed widths plan_chain_widths_ragged {widths_ragged; edge_tiles},
//      where the others refuse
// Calls that differ in n are rules 4 and 6's (ragged mixed widths) alone, equal widths everyone else's; strict is read by every rule.
constexpr int CHAIN_PLAN_MAXL = 8; // (= CH_MAXL, chain_args.h)
enum ChainForm : int { CF_CALLS, CF_F32, CF_PLAIN, CF_EDGE, CF_ROUNDS, CF_RAGGED, CF_WIDTHS, CF_WROUNDS, CF_WRAGGED, CF_DMA256, CF_SKINNY, CF_FORMS };
// xsmm_hip_set_strict, the seven chain switches of the tiles (xsmm_hip_set_chain_*), xsmm_hip_set_edge_tiles and xsmm_hip_set_dma256_images, and
// xsmm_hip_set_chain_skinny; mode_switches.h chain_plan_env_of fills it per invoke (rt_core.h chain_plan_env)
struct ChainPlanEnv { bool strict; int edge, rounds, ragged, widths, width_rounds, widths_ragged, dma256; int edge_tiles, dma256_images; int skinny = 0; };
// The compute units a launch on the invoke's stream can use - the one input that costs runtime calls (rt_chain.h stream_cus: three). Asked
// lazily and at most once per invoke: a decision that ends in front of every rule that reads them never pays for them.
struct ChainCus {
  int64_t (*ask)(void *);
  void *arg;
  int64_t known = -1;
  int64_t get() { return known >= 0 ? known : (known = ask(arg)); }
};
struct ChainLaunchPlan {
  ChainForm form;     // CF_CALLS: call by call, `why` names a rule that refused
  int tile;           // the launcher's tile: loader-wave tile 0 .. 3, f32 chain tile 1 / 2, 3 for CF_DMA256 (whose launcher takes none), the column-block width BN for CF_SKINNY
  int b_kind;         // the B image of the launch: 0 VNNI-2, 2 flat, 4 VNNI-4 (0 for CF_F32)
  int groups;         // ChainArgs::groups: row groups G (CF_ROUNDS, CF_DMA256), workgroup columns W (CF_WROUNDS), resident workgroups G (CF_SKINNY), 0 otherwise
  int bm, bn;         // the tile's rows and columns (256 x 256 for CF_DMA256; CF_SKINNY: all m rows x BN)
                      // CF_SKINNY: tiles_m = 1 and tiles_n = G - the counter-block key and the arrivals per counter (brgemm_bf16_skinny_chain.h) -,
                      // mixed = false (the target is epoch x G) although ChainLayer::pad carries each layer's n
  int tiles_m, tiles_n; // the counter-block key and the grid: ceil-divided where the form has edge tiles (m: CF_EDGE, CF_RAGGED, CF_WRAGGED; n: the
                      // latter two), the widest layer's column tiles in the width forms
  int tiles_l[CHAIN_PLAN_MAXL]; // the width forms: column tiles per layer, part of the key (what a launch adds to layer l's counters); zero otherwise
  int args_n;         // ChainArgs::n: the widest layer's n
  bool mixed;         // a width form (CF_WIDTHS, CF_WROUNDS, CF_WRAGGED): ChainLayer::pad carries each layer's n, and the hand-off target is the
                      // block's epoch - the kernel multiplies by the producing layer's column tiles; otherwise epoch x tiles_n
  const char *why;    // CF_CALLS: the refusal, a static string ("" for a launch)
  // rules that were asked in front of the answer and refused: "no <rule> (<why>)" under TPP_HIP_TRACE
  struct Note { const char *rule, *why; } notes[4];
  int n_notes;
};
ChainLaunchPlan plan_chain(int n, const GemmDesc *const *d, const int64_t *br, const ChainPlanEnv &env, ChainCus &cus);
// 1 / 2 = the f32 chain tile (brgemm_f32_lw.hip launch_f32_chain) the descriptor was planned on, -1 = none
int f32_chain_tile(const GemmDesc &d);
// tile: 0 = 32x64 (K split over two wave groups), 1 = 64x64, 2 = 64x128, 3 = 128x128 (brgemm_bf16_lw.hip; BLW_TILES, brgemm_bf16_lw_launch.h)
void blw_tile_dims(int tile, int *bm, int *bn);
// the GemmVariant of loader-wave tile 0 .. 3 with B image b_kind (20 + t VNNI-2, 24 + t flat, 28 + t VNNI-4), and the tile of such a variant
inline int blw_variant(int tile, int b_kind) { return (b_kind == 4 ? V_BF16_LW4_32x64 : b_kind == 2 ? V_BF16_LWF_32x64 : V_BF16_LW_32x64) + tile; }
inline int blw_variant_tile(int variant, int b_kind) { return variant - blw_variant(0, b_kind); }
// f32 chain tiles as in launch_f32_lw: 1 = 64x64 + K2, 2 = 64x32 + K4 (K-split tiles: 16-byte stores; 32x32 + K4 measured slower than three launches)
bool f32_chain_tile_dims(int tile, int *bm, int *bn);

} // namespace tpp
