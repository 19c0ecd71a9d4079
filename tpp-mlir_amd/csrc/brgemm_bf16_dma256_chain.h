// brgemm_bf16_dma256_chain.h - the maps of a LAYER CHAIN on the 256x256 bf16 tile (brgemm_bf16_dma256_chain.hip, opt-in: xsmm_hip_set_chain_dma256),
// written once as plain functions: the kernel, its launcher, the planner (gemm_plan.cpp) and a CPU test (tests/test_chain_dma256_schedule.py)
// all include this file. Nothing here needs a device: it compiles with any C++14 host compiler.
//
// A chain of L layers on tiles_m x tiles_n output tiles of 256 x 256 runs on G x tiles_n RESIDENT workgroups, a one-dimensional grid: G row
// GROUPS, G = tiles_m in a chain of one round. Workgroup wg is (g, tn) by the map below and computes tile (tm, tn) of every layer for the
// row blocks tm = g, g + G, .. < tiles_m of its group, LAYER-MAJOR - the walk of brgemm_bf16_lw_chain_rounds.h (chain_rounds_next /
// chain_rounds_more), unchanged. A step of layer l > 0 waits until cnt[l - 1][tm] has received the tiles_n arrivals of this launch; a step
// of a layer l < L - 1 adds one to cnt[l][tm] when its tile is stored. The progress argument is the one written in that header: a step
// waits only for steps that lie earlier in their workgroups' own order, and every workgroup is resident.
//
// THE MAP. Consecutive workgroup ids go to the 8 XCDs in turn. Where 4 divides G and 2 divides tiles_n the grid is XCD-BLOCKED as the
// single-call kernel's dim3(8, tiles_n / 2, tiles_m / 4) is: XCD x = wg % 8 holds the groups [(x >> 1) * G / 4, + G / 4) and the columns
// [(x & 1) * tiles_n / 2, + tiles_n / 2) - an eighth of the A panels and half of the B panels pass through each L2 instead of all of the
// one and an eighth of the other. Otherwise the map is linear, tn fastest.
#pragma once
#include "brgemm_bf16_lw_chain_rounds.h"

namespace tpp {

constexpr int D256C_BM = 256, D256C_BN = 256, D256C_BK = 32; // the tile and its k chunk (D256_BM, D256_BN, D256_BK of brgemm_bf16_dma256_images.h)

// resident workgroups of the launch
constexpr long long d256c_grid(int G, int tiles_n) { return (long long)G * tiles_n; }
constexpr bool d256c_blocked(int G, int tiles_n) { return G > 0 && tiles_n > 0 && (G & 3) == 0 && (tiles_n & 1) == 0; }
// workgroup wg of the grid -> its row group and its column tile
constexpr int d256c_group(int wg, int G, int tiles_n) {
  return d256c_blocked(G, tiles_n) ? ((wg & 7) >> 1) * (G >> 2) + (wg >> 3) / (tiles_n >> 1) : wg / tiles_n;
}
constexpr int d256c_col(int wg, int G, int tiles_n) {
  return d256c_blocked(G, tiles_n) ? (wg & 1) * (tiles_n >> 1) + (wg >> 3) % (tiles_n >> 1) : wg % tiles_n;
}
// the counter of row block tm in the hand-off from layer l to l + 1, in words (stride: CHAIN_CNT_STRIDE)
constexpr long long d256c_counter(int l, int tm, int tiles_m, int stride) { return ((long long)l * tiles_m + tm) * stride; }
// what the launcher asks of the shape: whole tiles, 2 .. max_layers layers, 1 <= G <= tiles_m
constexpr bool d256c_shape_ok(long long m, long long n, int nlayers, int max_layers, int G) {
  return m >= D256C_BM && n >= D256C_BN && m % D256C_BM == 0 && n % D256C_BN == 0 && m / D256C_BM <= 0x7fffffff / 64 && n / D256C_BN <= 0x7fffffff / 64 &&
         nlayers >= 2 && nlayers <= max_layers && G >= 1 && G <= m / D256C_BM && d256c_grid(G, (int)(n / D256C_BN)) <= 0x7fffffff;
}
constexpr bool d256c_k_ok(long long k, long long br) { return k >= D256C_BK && k % D256C_BK == 0 && k <= 0x7fffffff && br >= 1 && br * (k / D256C_BK) <= 0x7fffffff; }

} // namespace tpp
