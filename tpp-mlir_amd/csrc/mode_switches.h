// mode_switches.h - the opt-in MODE SWITCHES of the C-ABI (include/tpp_xsmm_abi.h xsmm_hip_set_<name> / xsmm_hip_<name>_stats), declared
// once: a switch is an environment variable TPP_HIP_<NAME> read when the library is loaded, a default, a set of accepted values and a
// block of counters. What the values MEAN stands at the declarations in the public header and at the planner rule that reads them
// (gemm_plan.h); this file only keeps them. Host-only, no HIP call. The modes and the counters are INLINE variables: the ABI layer
// (runtime.cpp) sets and reads them, the launch code (brgemm_f32.hip launch_gemm, rt_chain.h try_chain_launch) reads the modes per invoke
// and counts - and the host-only builds of runtime.cpp (tests/tsan, tests/chain_dispatch) link without any kernel file.
// Not here: the settings of rt_core.h Config, xsmm_hip_force_variant and xsmm_hip_force_split, which have side conditions of their own.
#pragma once
#include "gemm_plan.h" // GemmPlanEnv, ChainPlanEnv
#include <assert.h>
#include <stdint.h>
#include <stdlib.h>
#include <atomic>
#include <initializer_list>

namespace tpp {

enum ModeSwitch : int {
  MS_TAIL_SPLIT, MS_EDGE_TILES, MS_EDGE_K, MS_EDGE_K_BF16, MS_EDGE_K8_BF16, MS_DMA256_IMAGES, MS_DMA256_EDGE, MS_SKINNY_BF16, MS_SKINNY_SPLIT,
  MS_F32_HALVES, MS_CHAIN_EDGE, MS_CHAIN_ROUNDS, MS_CHAIN_RAGGED, MS_CHAIN_WIDTHS, MS_CHAIN_WIDTH_ROUNDS, MS_CHAIN_WIDTHS_RAGGED, MS_CHAIN_DMA256,
  MS_CHAIN_SKINNY, MS_COUNT
};

// the values a setter accepts (every other value: -1, nothing changed; in the environment: the default)
constexpr bool tail_split_mode_ok(int v) { return v >= 0 && v <= 16; }
constexpr bool edge_tiles_mode_ok(int v) { return v == 0 || v == 1 || v == 2 || v == 6 || v == 7 || v == 9 || v == 10 || (v >= 20 && v <= 23); }
constexpr bool edge_k_mode_ok(int v) { return v == 0 || v == 1 || v == 6 || v == 7 || v == 9 || v == 10; }
constexpr bool edge_k_bf16_mode_ok(int v) { return v == 0 || v == 1 || (v >= 20 && v <= 23); } // (the half-step switch takes the same values)
constexpr bool dma256_images_mode_ok(int v) { return v >= 0 && v <= 2; }
constexpr bool dma256_edge_mode_ok(int v) { return v >= 0 && v <= 2; }
constexpr bool skinny_bf16_mode_ok(int v) { return v == 0 || v == 1 || v == 16 || v == 32 || v == 64; }
constexpr bool skinny_split_mode_ok(int v) { return v >= 0 && v <= 16; }
constexpr bool f32_halves_mode_ok(int v) { return v >= 0 && v <= 2; }
constexpr bool chain_edge_mode_ok(int v) { return v == 0 || v == 1; }
constexpr bool chain_rounds_mode_ok(int v) { return v == 0 || v == 1 || (v > 1000 && v <= 1000 + 0x10000); }
constexpr bool chain_ragged_mode_ok(int v) { return v == 0 || v == 1; }
constexpr bool chain_widths_mode_ok(int v) { return v == 0 || v == 1; }
constexpr bool chain_width_rounds_mode_ok(int v) { return v == 0 || v == 1 || (v > 1000 && v <= 1000 + 0x10000); }
constexpr bool chain_widths_ragged_mode_ok(int v) { return v == 0 || v == 1; }
constexpr bool chain_dma256_mode_ok(int v) { return v == 0 || v == 1 || v == 2 || (v > 1000 && v <= 1000 + 0x10000); }
constexpr bool chain_skinny_mode_ok(int v) {
  const int bn = v >= 1000 ? v % 1000 : v, g = v >= 1000 ? v / 1000 : 1;
  return v == 0 || v == 1 || ((bn == 16 || bn == 32 || bn == 64) && g >= 1 && g <= 512);
}

constexpr int MODE_STATS_MAX = 5; // words of the largest counter block
struct ModeSwitchRow {
  ModeSwitch id;     // the row's own index (checked below)
  const char *env;   // read once, at load, with atoi; unset or refused: dflt
  int dflt;
  bool (*ok)(int);
  int counters;      // words of xsmm_hip_<name>_stats: [0] counts launches, the others describe the latest one
};
// One row per switch; behind each: who plans it (gemm_plan.cpp), who launches it, and the words [1 ..] of its counter block.
inline constexpr ModeSwitchRow MODE_SWITCHES[MS_COUNT] = {
    // choose_f32_tail_split; brgemm_f32_lw.hip launch_f32_lw_tail: tail tiles, workgroups per tail tile, body tiles
    {MS_TAIL_SPLIT, "TPP_HIP_TAIL_SPLIT", 0, tail_split_mode_ok, 4},
    // choose_f32_edge_variant, choose_bf16_edge_tile; launch_f32_lw_edge, launch_bf16_lw(BLW_EDGE): tile rows, tile columns, GemmVariant of the tile
    {MS_EDGE_TILES, "TPP_HIP_EDGE_TILES", 0, edge_tiles_mode_ok, 4},
    // plan_gemm_call; brgemm_f32_lw_kedge.h: chunks per batch element, overlap o, GemmVariant of the tile
    {MS_EDGE_K, "TPP_HIP_EDGE_K", 0, edge_k_mode_ok, 4},
    // plan_gemm_call; brgemm_bf16_lw_kedge.h: chunks per batch element, overlap o, GemmVariant of the tile with its B image
    {MS_EDGE_K_BF16, "TPP_HIP_EDGE_K_BF16", 0, edge_k_bf16_mode_ok, 4},
    // plan_gemm_call; brgemm_bf16_lw_kedge.h bkedge8_*: the same words
    {MS_EDGE_K8_BF16, "TPP_HIP_EDGE_K8_BF16", 0, edge_k_bf16_mode_ok, 4},
    // plan_gemm_call; brgemm_bf16_dma256.hip launch_bf16_dma256_image: tile rows, tile columns (256x256), B image (2 flat, 4 VNNI-4)
    {MS_DMA256_IMAGES, "TPP_HIP_DMA256_IMAGES", 0, dma256_images_mode_ok, 4},
    // plan_gemm_call, dma256_edge_rule; brgemm_bf16_dma256_edge.hip: tile rows, tile columns (ceil-divided), B image (0 VNNI-2, 2 flat, 4 VNNI-4)
    {MS_DMA256_EDGE, "TPP_HIP_DMA256_EDGE", 0, dma256_edge_mode_ok, 4},
    // plan_gemm_call, skinny_bf16_bn; brgemm_bf16_skinny.hip: workgroups, waves per workgroup, BN, B image
    {MS_SKINNY_BF16, "TPP_HIP_SKINNY_BF16", 0, skinny_bf16_mode_ok, 5},
    // plan_gemm_call, skinny_split_parts - read only for a call already on the skinny kernel; brgemm_bf16_skinny_split.hip: parts P_eff, workgroups
    {MS_SKINNY_SPLIT, "TPP_HIP_SKINNY_SPLIT", 0, skinny_split_mode_ok, 3},
    // choose_f32_halves; brgemm_f32_lw.hip launch_f32_lw_halves: tile rows, tile columns (64x64), 0. The one switch that is on by default
    {MS_F32_HALVES, "TPP_HIP_F32_HALVES", 1, f32_halves_mode_ok, 4},
    // The chain switches: plan_chain asks the rule named here, rt_chain.h try_chain_launch launches and counts - row blocks, column tiles and
    // the GemmVariant of the tile with its B image, unless the row says otherwise.
    {MS_CHAIN_EDGE, "TPP_HIP_CHAIN_EDGE", 0, chain_edge_mode_ok, 4},                   // plan_chain_edge
    {MS_CHAIN_ROUNDS, "TPP_HIP_CHAIN_ROUNDS", 0, chain_rounds_mode_ok, 4},             // plan_chain_rounds: row groups G, rounds R, GemmVariant
    {MS_CHAIN_RAGGED, "TPP_HIP_CHAIN_RAGGED", 0, chain_ragged_mode_ok, 4},             // plan_chain_ragged
    {MS_CHAIN_WIDTHS, "TPP_HIP_CHAIN_WIDTHS", 0, chain_widths_mode_ok, 4},             // plan_chain_widths
    {MS_CHAIN_WIDTH_ROUNDS, "TPP_HIP_CHAIN_WIDTH_ROUNDS", 0, chain_width_rounds_mode_ok, 4}, // plan_chain_width_rounds: row blocks, workgroup columns W, GemmVariant
    {MS_CHAIN_WIDTHS_RAGGED, "TPP_HIP_CHAIN_WIDTHS_RAGGED", 0, chain_widths_ragged_mode_ok, 4}, // plan_chain_widths_ragged
    {MS_CHAIN_DMA256, "TPP_HIP_CHAIN_DMA256", 0, chain_dma256_mode_ok, 4},             // plan_chain_dma256: row groups G, rounds R, B image
    {MS_CHAIN_SKINNY, "TPP_HIP_CHAIN_SKINNY", 0, chain_skinny_mode_ok, 4},             // plan_chain_skinny: resident workgroups G, BN, B image
};
constexpr bool mode_switch_table_ok() {
  for (int i = 0; i < MS_COUNT; ++i)
    if (MODE_SWITCHES[i].id != i || !MODE_SWITCHES[i].ok(MODE_SWITCHES[i].dflt) || MODE_SWITCHES[i].counters < 1 || MODE_SWITCHES[i].counters > MODE_STATS_MAX)
      return false;
  return true;
}
static_assert(mode_switch_table_ok(), "a row of MODE_SWITCHES stands at another index than its switch, or its default or counter count is out of range");

struct ModeSwitchState {
  std::atomic<int> mode[MS_COUNT];
  alignas(64) std::atomic<int64_t> stats[MS_COUNT][MODE_STATS_MAX] = {}; // (a line of their own: counting never takes the modes' line from the invoking threads)
  ModeSwitchState() {
    for (int i = 0; i < MS_COUNT; ++i) {
      const ModeSwitchRow &r = MODE_SWITCHES[i];
      const char *e = getenv(r.env);
      const int v = e ? atoi(e) : r.dflt;
      mode[i].store(r.ok(v) ? v : r.dflt, std::memory_order_relaxed);
    }
  }
};
inline ModeSwitchState g_mode_switches;

inline int mode_of(ModeSwitch s) { return g_mode_switches.mode[s].load(std::memory_order_relaxed); }
// returns the previous mode, -1 (nothing changed) for a value the switch refuses
inline int set_mode(ModeSwitch s, int v) { return MODE_SWITCHES[s].ok(v) ? g_mode_switches.mode[s].exchange(v) : -1; }
// out: the switch's own count of words (ModeSwitchRow::counters)
inline void mode_stats(ModeSwitch s, int64_t *out) {
  for (int i = 0; i < MODE_SWITCHES[s].counters; ++i) out[i] = g_mode_switches.stats[s][i].load(std::memory_order_relaxed);
}
// one launch under the switch: the words [1 ..] that describe it first, then the launch count - a reader that sees the count move
// between two reads has words no older than that launch. At most counters - 1 words (asserted; the store is bounded all the same); a
// word the caller does not name keeps its value - f32_halves names two and its word 3 stays 0
inline void count_mode_launch(ModeSwitch s, std::initializer_list<int64_t> words) {
  assert((int)words.size() < MODE_SWITCHES[s].counters);
  int i = 1;
  for (int64_t w : words)
    if (i < MODE_SWITCHES[s].counters) g_mode_switches.stats[s][i++].store(w, std::memory_order_relaxed);
  g_mode_switches.stats[s][0].fetch_add(1, std::memory_order_relaxed);
}

// The ONLY two places that map switches to planner inputs (field order and names: gemm_plan.h). Relaxed loads, no lock, per invoke.
inline GemmPlanEnv gemm_plan_env_of(int cus, bool strict, int forced_split) {
  GemmPlanEnv e{cus, strict, forced_split};
  e.tail_split = mode_of(MS_TAIL_SPLIT);
  e.edge_tiles = mode_of(MS_EDGE_TILES);
  e.edge_k = mode_of(MS_EDGE_K);
  e.edge_k_bf16 = mode_of(MS_EDGE_K_BF16);
  e.halves = mode_of(MS_F32_HALVES);
  e.edge_k8_bf16 = mode_of(MS_EDGE_K8_BF16);
  e.dma256_images = mode_of(MS_DMA256_IMAGES);
  e.dma256_edge = mode_of(MS_DMA256_EDGE);
  e.skinny_bf16 = mode_of(MS_SKINNY_BF16);
  e.skinny_split = mode_of(MS_SKINNY_SPLIT);
  return e;
}
inline ChainPlanEnv chain_plan_env_of(bool strict) {
  ChainPlanEnv e{};
  e.strict = strict;
  e.edge = mode_of(MS_CHAIN_EDGE);
  e.rounds = mode_of(MS_CHAIN_ROUNDS);
  e.ragged = mode_of(MS_CHAIN_RAGGED);
  e.widths = mode_of(MS_CHAIN_WIDTHS);
  e.width_rounds = mode_of(MS_CHAIN_WIDTH_ROUNDS);
  e.widths_ragged = mode_of(MS_CHAIN_WIDTHS_RAGGED);
  e.dma256 = mode_of(MS_CHAIN_DMA256);
  e.edge_tiles = mode_of(MS_EDGE_TILES);
  e.dma256_images = mode_of(MS_DMA256_IMAGES);
  e.skinny = mode_of(MS_CHAIN_SKINNY);
  return e;
}

} // namespace tpp
