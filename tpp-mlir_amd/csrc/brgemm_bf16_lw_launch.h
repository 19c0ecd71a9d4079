// brgemm_bf16_lw_launch.h - the launch table of brgemm_bf16_lw<WM, WN, WK, TM, TN, NSLOT, NLA, NLB, SUP, MULTI, FLATB, GRP> (brgemm_bf16_lw.hip),
// written once as plain constexpr functions: the launch modes (the values of GRP) and what follows from one, the tiles, which instances
// exist and what each mode's launcher refuses. The kernel, its loader, its launchers, the planner (gemm_plan.cpp) and a CPU test
// (tests/test_blw_launch_table.py) all include this file. Nothing here needs a device: it compiles with any C++17 host compiler.
#pragma once
#include "brgemm_bf16_lw_kedge.h"
#include "brgemm_bf16_lw_chain_ragged.h"
#include "brgemm_bf16_lw_chain_widths.h"
#include "brgemm_bf16_lw_chain_wrounds.h"
#include "brgemm_bf16_lw_chain_wragged.h"

namespace tpp {

// LAUNCH MODES: the kernel's template parameter GRP (an int, so that the kernels keep their names). Each is described where the kernel
// and the loader treat it.
constexpr int BLW_LAYER = 0;        // one whole layer (MULTI false) or a chain of layers on co-resident tiles (MULTI true)
constexpr int BLW_ITEMS = 1;        // tile invokes of one descriptor: operands and batch count from a WorkItem
constexpr int BLW_QUADS = 2;        // 2 x 2 blocks of 64x64 items on the 128x128 tile: operands from a QuadItem
constexpr int BLW_EDGE = 3;         // a layer whose m or n the tile does not divide (xsmm_hip_set_edge_tiles)
constexpr int BLW_KEDGE = 4;        // BLW_EDGE + a k that is a multiple of 16 but not of 64 (xsmm_hip_set_edge_k_bf16)
constexpr int BLW_CHAIN_EDGE = 5;   // a chain whose m the tile's rows do not divide (xsmm_hip_set_chain_edge)
constexpr int BLW_KEDGE8 = 6;       // BLW_KEDGE in half steps: k a multiple of 8 but not of 16 (xsmm_hip_set_edge_k8_bf16)
constexpr int BLW_CHAIN_ROUNDS = 7; // a chain on fewer resident workgroups than output tiles (xsmm_hip_set_chain_rounds)
constexpr int BLW_MODES = 8;
// A ragged-WIDTH chain (xsmm_hip_set_chain_ragged): a mode BESIDE the table - blw_instance_exists and blw_launch_ok go on refusing it, its
// instances live in a translation unit of their own (brgemm_bf16_lw_chain_ragged.hip) and have their own predicates at the end of this file
constexpr int BLW_CHAIN_RAGGED = 8; // a chain with a ragged n and / or a k that is a multiple of 8 but not of 64 in some layer
// A MIXED-WIDTH chain (xsmm_hip_set_chain_widths): beside the table in the same way (brgemm_bf16_lw_chain_widths.hip, predicates at the end)
constexpr int BLW_CHAIN_WIDTHS = 9; // a chain whose layers differ in n: a workgroup sits out the layers that have no column tile for it
// A mixed-width chain in COLUMN ROUNDS (xsmm_hip_set_chain_width_rounds): beside the table too (brgemm_bf16_lw_chain_wrounds.hip, predicates at the end)
constexpr int BLW_CHAIN_WROUNDS = 10; // BLW_CHAIN_WIDTHS on fewer resident workgroup columns than the widest layer has column tiles
// A RAGGED mixed-width chain (xsmm_hip_set_chain_widths_ragged): beside the table too (brgemm_bf16_lw_chain_wragged.hip, predicates at the end)
constexpr int BLW_CHAIN_WRAGGED = 11; // BLW_CHAIN_WIDTHS with BLW_CHAIN_RAGGED's layers: any m >= BM, per layer any n(l) >= BN and k >= 64 in multiples of 8

// what follows from a mode
constexpr bool blw_items(int g) { return g == BLW_ITEMS || g == BLW_QUADS; }      // operands and batch count come from an item
constexpr bool blw_ragged_k(int g) { return g == BLW_KEDGE || g == BLW_KEDGE8; }  // the last chunk of a batch element is shifted back
constexpr bool blw_chain_ragged(int g) { return g == BLW_CHAIN_RAGGED; }         // every layer its own k class, tested in half steps
constexpr bool blw_chain_widths(int g) { return g == BLW_CHAIN_WIDTHS; }         // per-layer n in the argument block, skipped layers
constexpr bool blw_chain_wrounds(int g) { return g == BLW_CHAIN_WROUNDS; }       // ... and a workgroup walks several column tiles of a layer
constexpr bool blw_chain_wragged(int g) { return g == BLW_CHAIN_WRAGGED; }       // per-layer n AND per-layer column shifts, k classes and a carried ring
constexpr bool blw_half_steps(int g) { return g == BLW_KEDGE8; }                  // ... and its overlap ends in the middle of a k-step
// the last row block is shifted back to end at row m and stores its own rows only
constexpr bool blw_edge_rows(int g) { return g == BLW_EDGE || blw_ragged_k(g) || g == BLW_CHAIN_EDGE || blw_chain_ragged(g) || blw_chain_wragged(g); }
// the last column tile is shifted back to end at column n (a ragged-m chain's columns are whole tiles, a ragged-width chain's are not)
constexpr bool blw_edge_cols(int g) { return g == BLW_ITEMS || g == BLW_EDGE || blw_ragged_k(g) || blw_chain_ragged(g) || blw_chain_wragged(g); }
constexpr bool blw_chain(int g) { return g == BLW_CHAIN_EDGE || g == BLW_CHAIN_ROUNDS; } // a chain by itself (BLW_LAYER: either)
constexpr bool blw_one_chunk(int g) { return blw_ragged_k(g) || blw_chain(g) || blw_chain_ragged(g) || blw_chain_wragged(g); }   // one chunk per barrier only (SUP = 1)
// the combinations of mode, MULTI and SUP the kernel and the loader are written for
constexpr bool blw_mode_ok(int g, bool multi, int sup) {
  return g >= 0 && g < BLW_MODES && (multi ? g == BLW_LAYER || blw_chain(g) : !blw_chain(g)) && (!blw_one_chunk(g) || sup == 1);
}
template <int GRP, bool MULTI, int SUP> struct BlwModeCheck {
  static_assert((GRP >= 0 && GRP < BLW_MODES) || blw_chain_ragged(GRP) || blw_chain_widths(GRP) || blw_chain_wrounds(GRP) || blw_chain_wragged(GRP), "0: a layer / chain, 1: items, 2: quads, 3: a layer on edge tiles, 4: edge tiles + a ragged k, 5: a chain on edge row tiles, 6: 4 in half steps, 7: a chain in several rounds, 8: a ragged-width chain, 9: a mixed-width chain, 10: a mixed-width chain in column rounds, 11: a ragged mixed-width chain");
  static_assert(!MULTI || GRP == BLW_LAYER || blw_chain(GRP) || blw_chain_ragged(GRP) || blw_chain_widths(GRP) || blw_chain_wrounds(GRP) || blw_chain_wragged(GRP), "a grouped launch is a set of single layers");
  static_assert(!blw_ragged_k(GRP) || (SUP == 1 && !MULTI), "ragged k: one layer, one chunk per barrier");
  static_assert(!blw_chain(GRP) || (SUP == 1 && MULTI), "a ragged / multi-round chain: a chain, one chunk per barrier");
  static_assert(!blw_chain_ragged(GRP) || (SUP == 1 && MULTI), "a ragged-width chain: a chain, one chunk per barrier");
  static_assert(!blw_chain_widths(GRP) || (MULTI && (SUP == 1 || SUP == 2)), "a mixed-width chain: a chain, one or two chunks per barrier");
  static_assert(!blw_chain_wrounds(GRP) || (SUP == 1 && MULTI), "a mixed-width chain in column rounds: a chain, one chunk per barrier");
  static_assert(!blw_chain_wragged(GRP) || (SUP == 1 && MULTI), "a ragged mixed-width chain: a chain, one chunk per barrier");
  static constexpr bool ok = blw_chain_ragged(GRP) || blw_chain_wrounds(GRP) || blw_chain_wragged(GRP) ? MULTI && SUP == 1 : blw_chain_widths(GRP) ? MULTI && (SUP == 1 || SUP == 2) : blw_mode_ok(GRP, MULTI, SUP);
};

// THE TILES. 0 = 32x64 + K2, 1 = 64x64, 2 = 64x128, 3 = 128x128, 4 = 32x32 + K2. Loader waves per tile (NLA + NLB), same-box A/B
// (profiles/r03_blw_loader_split.txt): 32x64 1 + 2 (1 + 1: +2 %, 2 + 2: +5 %), 64x64 1 + 1 (1 + 2: +2 %, 2 + 2: +7 %), 64x128 1 + 2
// (1 + 1: same, 2 + 4: +5 %), 128x128 1 + 1 (2 + 2, 1 + 2: same). Ring depths: 8 / 8 / 6 / 4 slots; a 5-slot ring with 2 + 2 loaders for the
// 128x128 tile and 4 against 6 slots for 64x128 measured the same (same box, +-0.5 %); FOUR chunks per barrier on a 12-slot ring for the
// 32x64 tile measured 9 % slower than two on 8 slots (the prologue must request 8 chunks before the first barrier).
// Tile 4 (round 5, single layers and items only, no flat B): two MFMA waves, one loader wave per panel. For SMALL outputs with a LONG
// reduction (the reference's M = 128 / 256 shapes at K >= 1536): twice the workgroups of the 32x64 tile, each streaming 8 KiB per chunk -
// the layer is bound by how many CUs pull panels, not by the matrix pipes.
struct BlwTile {
  int wm, wn, wk, tm, tn, nslot, nla, nlb;
  constexpr int bm() const { return 32 * wm * tm; }
  constexpr int bn() const { return 32 * wn * tn; }
};
constexpr int BLW_NTILES = 5;
constexpr BlwTile BLW_TILES[BLW_NTILES] = {{1, 2, 2, 1, 1, 8, 1, 2}, {2, 2, 1, 1, 1, 8, 1, 1}, {2, 2, 1, 1, 2, 6, 1, 2}, {2, 2, 1, 2, 2, 4, 1, 1}, {1, 1, 2, 1, 1, 8, 1, 1}};
// SUP = 2 (one workgroup barrier per TWO chunks): the tiles with one accumulator per wave, when every chunk count is even
constexpr bool blw_tile_sup2(int tile) { return tile == 0 || tile == 1 || tile == 4; }
constexpr bool blw_b_kind_ok(int b_kind) { return b_kind == 0 || b_kind == 2 || b_kind == 4; } // B image: VNNI-2, flat, VNNI-4

// THE INSTANCES: is brgemm_bf16_lw<BLW_TILES[tile]..., sup, multi, b_kind, mode> compiled? (120 are; the launchers instantiate nothing else)
constexpr bool blw_instance_exists(int mode, bool multi, int tile, int b_kind, int sup) {
  if (tile < 0 || tile >= BLW_NTILES || !blw_b_kind_ok(b_kind) || !(sup == 1 || (sup == 2 && blw_tile_sup2(tile))) || !blw_mode_ok(mode, multi, sup)) return false;
  if (mode == BLW_LAYER) return tile <= 3 || (!multi && b_kind != 2);
  if (mode == BLW_ITEMS) return blw_tile_sup2(tile) && b_kind != 2;
  if (mode == BLW_QUADS) return tile == 3 && b_kind != 2;
  return tile <= 3; // edge tiles, both ragged k, both chains
}

// THE REFUSALS: does the launcher of `mode` take this launch? What it asks of a launch's arguments, copied out of the argument block.
constexpr int BLW_MAXL = 8; // (= CH_MAXL, chain_args.h)
struct BlwShape {
  bool chain;      // BLW_LAYER: a chain (launch_bf16_chain), not one layer
  int m, n, nlayers, groups;
  int k[BLW_MAXL], br[BLW_MAXL]; // per layer: k per batch element, batch count (the first min(nlayers, BLW_MAXL), at least one)
};
// every layer of a ragged / multi-round chain: a batch of at least one element in whole chunks
constexpr bool blw_chain_layers_ok(const BlwShape &a) {
  if (a.nlayers < 2 || a.nlayers > BLW_MAXL) return false;
  for (int l = 0; l < a.nlayers; ++l)
    if (a.br[l] < 1 || a.k[l] < BKEDGE_BK || a.k[l] % BKEDGE_BK != 0) return false;
  return true;
}
constexpr bool blw_launch_ok(int mode, int tile, int b_kind, const BlwShape &a) {
  if (tile < 0 || tile >= BLW_NTILES || !blw_b_kind_ok(b_kind)) return false;
  const int bm = BLW_TILES[tile].bm(), bn = BLW_TILES[tile].bn();
  const bool whole_k = a.k[0] >= BKEDGE_BK && a.k[0] % BKEDGE_BK == 0;
  // one layer on tile 0 .. 3 that holds at least one tile and one batch element
  const bool edge_layer = tile <= 3 && a.nlayers == 1 && a.m >= bm && a.n >= bn && a.br[0] >= 1;
  const bool edge_chain = tile <= 3 && blw_chain_layers_ok(a) && a.m >= bm && a.n >= bn && a.n % bn == 0;
  switch (mode) {
  case BLW_LAYER: return a.chain ? tile <= 3 : a.br[0] >= 1 && a.k[0] >= BKEDGE_BK && (tile <= 3 || b_kind != 2);
  case BLW_ITEMS: return whole_k && blw_tile_sup2(tile) && b_kind != 2;
  case BLW_QUADS: return whole_k && a.m == 128 && a.n == 128 && b_kind != 2;
  case BLW_EDGE: return edge_layer && whole_k;
  case BLW_KEDGE: return edge_layer && a.n % 8 == 0 && bkedge_k_ok(a.k[0]);
  case BLW_KEDGE8: return edge_layer && a.n % 8 == 0 && bkedge8_k_ok(a.k[0]);
  case BLW_CHAIN_EDGE: return edge_chain;
  case BLW_CHAIN_ROUNDS: return edge_chain && a.m % bm == 0 && a.groups >= 1 && a.groups <= a.m / bm;
  default: return false;
  }
}

// THE RAGGED-WIDTH CHAIN (BLW_CHAIN_RAGGED, brgemm_bf16_lw_chain_ragged.hip): MULTI, one chunk per barrier. Is the instance of (tile, b_kind)
// compiled? Tiles 0 .. 3 with the three B images, less ONE: the 64x128 tile with the VNNI-2 image needs 76 bytes of scratch per lane in
// this mode (its plain chain instance is at 256 VGPRs already; the body for a layer that starts at an odd ring slot tips it over), so it
// does not exist - eleven instances, none with scratch. The planner (gemm_plan.cpp plan_chain_ragged) never names it.
constexpr bool blw_chain_ragged_instance_exists(int tile, int b_kind) { return tile >= 0 && tile <= 3 && blw_b_kind_ok(b_kind) && !(tile == 2 && b_kind == 0); }
// ... and what its launcher refuses: 2 .. 8 layers, every one a batch of at least one element with k >= 64 and k % 8 == 0; m >= BM, n >= BN,
// n % 8 == 0; ragged in n or in some layer's k (a chain ragged in m alone is BLW_CHAIN_EDGE's, a divisible one BLW_LAYER's)
constexpr bool blw_chain_ragged_launch_ok(int tile, int b_kind, const BlwShape &a) {
  if (!blw_chain_ragged_instance_exists(tile, b_kind) || a.nlayers < 2 || a.nlayers > BLW_MAXL) return false;
  const int bm = BLW_TILES[tile].bm(), bn = BLW_TILES[tile].bn();
  bool ragged = a.n % bn != 0;
  for (int l = 0; l < a.nlayers; ++l) {
    if (a.br[l] < 1 || !chain_ragged_k_ok(a.k[l])) return false;
    if (a.k[l] % BKEDGE_BK != 0) ragged = true;
  }
  return ragged && a.m >= bm && a.n >= bn && a.n % 8 == 0;
}

// THE MIXED-WIDTH CHAIN (BLW_CHAIN_WIDTHS, brgemm_bf16_lw_chain_widths.hip; schedule in brgemm_bf16_lw_chain_widths.h): MULTI. Is the instance of
// (tile, b_kind, sup) compiled? Tiles 0 .. 3 with the three B images at one chunk per barrier, tiles 0 and 1 at two as well - the plain
// chain's eighteen, none with scratch.
constexpr bool blw_chain_widths_instance_exists(int tile, int b_kind, int sup) {
  return tile >= 0 && tile <= 3 && blw_b_kind_ok(b_kind) && (sup == 1 || (sup == 2 && blw_tile_sup2(tile)));
}
// ... and what its launcher refuses, over a shape with per-layer widths: 2 .. 8 layers, every one a batch of at least one element in whole
// 64-k chunks and n(l) >= BN columns in whole column tiles; m in whole row blocks; at least two layers differ in n (an equal-width chain is
// BLW_LAYER's)
struct BlwWidthsShape {
  int m, nlayers;
  int n[BLW_MAXL], k[BLW_MAXL], br[BLW_MAXL]; // per layer (the first min(nlayers, BLW_MAXL))
};
constexpr bool blw_chain_widths_launch_ok(int tile, int b_kind, const BlwWidthsShape &a) {
  if (!blw_chain_widths_instance_exists(tile, b_kind, 1) || a.nlayers < 2 || a.nlayers > BLW_MAXL) return false;
  const int bm = BLW_TILES[tile].bm(), bn = BLW_TILES[tile].bn();
  bool differ = false;
  for (int l = 0; l < a.nlayers; ++l) {
    if (a.br[l] < 1 || a.k[l] < BKEDGE_BK || a.k[l] % BKEDGE_BK != 0) return false;
    if (a.n[l] < bn || a.n[l] % bn != 0) return false;
    if (a.n[l] != a.n[0]) differ = true;
  }
  return differ && a.m >= bm && a.m % bm == 0;
}

// THE MIXED-WIDTH CHAIN IN COLUMN ROUNDS (BLW_CHAIN_WROUNDS, brgemm_bf16_lw_chain_wrounds.hip; schedule in brgemm_bf16_lw_chain_wrounds.h): MULTI,
// one chunk per barrier. Is the instance of (tile, b_kind) compiled? Tiles 0 .. 3 with the three B images - twelve, none with scratch.
constexpr bool blw_chain_wrounds_instance_exists(int tile, int b_kind) { return tile >= 0 && tile <= 3 && blw_b_kind_ok(b_kind); }
// ... and what its launcher refuses: everything the mixed-width chain's does, and a number of column groups that is not
// 1 <= groups < max_l(n(l) / BN) (as many groups as the widest layer has column tiles is BLW_CHAIN_WIDTHS's launch)
constexpr bool blw_chain_wrounds_launch_ok(int tile, int b_kind, const BlwWidthsShape &a, int groups) {
  if (!blw_chain_wrounds_instance_exists(tile, b_kind) || !blw_chain_widths_launch_ok(tile, b_kind, a)) return false;
  int maxT = 0;
  for (int l = 0; l < a.nlayers; ++l)
    if (a.n[l] / BLW_TILES[tile].bn() > maxT) maxT = a.n[l] / BLW_TILES[tile].bn();
  return groups >= 1 && groups < maxT;
}

// THE RAGGED MIXED-WIDTH CHAIN (BLW_CHAIN_WRAGGED, brgemm_bf16_lw_chain_wragged.hip; schedule in brgemm_bf16_lw_chain_wragged.h): MULTI, one chunk
// per barrier. Is the instance of (tile, b_kind) compiled? Tiles 0 .. 3 with the three B images, less ONE: the 64x128 tile with the VNNI-2
// image, which needs 72 bytes of scratch per lane in this mode (17 spilled VGPRs) as it needs 76 in BLW_CHAIN_RAGGED (the body for a layer that
// starts at an odd ring slot tips its 256 VGPRs over), so it does not exist - eleven instances, none with scratch. The planner (gemm_plan.cpp plan_chain_widths_ragged)
// passes that tile over.
constexpr bool blw_chain_wragged_instance_exists(int tile, int b_kind) { return tile >= 0 && tile <= 3 && blw_b_kind_ok(b_kind) && !(tile == 2 && b_kind == 0); }
// ... and what its launcher refuses, over a shape with per-layer widths: 2 .. 8 layers, every one a batch of at least one element with
// k >= 64 and k % 8 == 0 and n(l) >= BN columns, n(l) % 8 == 0; m >= BM; at least two layers differ in n (an equal-width chain is
// BLW_CHAIN_RAGGED's, BLW_CHAIN_EDGE's or BLW_LAYER's); and something ragged on this tile - BM does not divide m, BN does not divide some
// n(l), or some k(l) % 64 != 0 (a chain the tile divides entirely is BLW_CHAIN_WIDTHS')
constexpr bool blw_chain_wragged_launch_ok(int tile, int b_kind, const BlwWidthsShape &a) {
  if (!blw_chain_wragged_instance_exists(tile, b_kind) || a.nlayers < 2 || a.nlayers > BLW_MAXL) return false;
  const int bm = BLW_TILES[tile].bm(), bn = BLW_TILES[tile].bn();
  bool differ = false, ragged = a.m % bm != 0;
  for (int l = 0; l < a.nlayers; ++l) {
    if (a.br[l] < 1 || !chain_ragged_k_ok(a.k[l])) return false;
    if (a.n[l] < bn || a.n[l] % 8 != 0) return false;
    if (a.n[l] != a.n[0]) differ = true;
    if (a.n[l] % bn != 0 || a.k[l] % BKEDGE_BK != 0) ragged = true;
  }
  return differ && ragged && a.m >= bm;
}

} // namespace tpp
