// driver.cpp - TEST INFRASTRUCTURE for tests/test_chain_dma256_schedule.py, never part of the product library.
//
// Walks the maps of a layer chain on the 256x256 tile (tpp-mlir_amd/csrc/brgemm_bf16_dma256_chain.h + brgemm_bf16_lw_chain_rounds.h) as the kernel
// does, for  driver <tiles_m> <tiles_n> <G> <L> <order: 0 identity, 1 reversed>  and prints the facts the test asserts:
//   map       <workgroups> bijection <0|1> groups_seen <n> cols_seen <n> blocked <0|1>
//   tiles     once <n> never <n> more <n>          (over L * tiles_m * tiles_n (layer, tm, tn))
//   arrivals  exact <n> other <n>                  (counters cnt[l][tm], l < L - 1: exactly tiles_n arrivals)
//   run       done <0|1> steps <n> sweeps <n>      (simulated execution: every workgroup resident, a step runs when its counter is at target)
#include "brgemm_bf16_dma256_chain.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

using namespace tpp;

int main(int argc, char **argv) {
  if (argc != 6) return 2;
  const int tiles_m = atoi(argv[1]), tiles_n = atoi(argv[2]), G = atoi(argv[3]), L = atoi(argv[4]), order = atoi(argv[5]);
  if (!d256c_shape_ok(256ll * tiles_m, 256ll * tiles_n, L, 8, G)) return 3;
  const int W = (int)d256c_grid(G, tiles_n);
  // the map: workgroup -> (group, column), a bijection onto G x tiles_n
  std::vector<int> hit((size_t)W, 0), wg_g((size_t)W), wg_tn((size_t)W);
  bool bij = true;
  std::vector<char> gs((size_t)G, 0), cs((size_t)tiles_n, 0);
  for (int wg = 0; wg < W; ++wg) {
    const int g = d256c_group(wg, G, tiles_n), tn = d256c_col(wg, G, tiles_n);
    if (g < 0 || g >= G || tn < 0 || tn >= tiles_n) { bij = false; continue; }
    if (hit[(size_t)g * tiles_n + tn]++) bij = false;
    wg_g[wg] = g, wg_tn[wg] = tn, gs[g] = 1, cs[tn] = 1;
  }
  int gseen = 0, cseen = 0;
  for (char c : gs) gseen += c;
  for (char c : cs) cseen += c;
  printf("map %d bijection %d groups_seen %d cols_seen %d blocked %d\n", W, (int)bij, gseen, cseen, (int)d256c_blocked(G, tiles_n));
  if (!bij) return 0;
  // simulated execution: per workgroup the walk's state; a step of layer l > 0 needs cnt[l-1][tm] == tiles_n (one launch, epoch 1)
  std::vector<int> tm((size_t)W), l((size_t)W, 0);
  for (int wg = 0; wg < W; ++wg) tm[wg] = wg_g[wg];
  std::vector<int> computed((size_t)L * tiles_m * tiles_n, 0), cnt((size_t)(L > 1 ? L - 1 : 1) * tiles_m, 0);
  long steps = 0, sweeps = 0;
  bool progress = true, all_done = false;
  while (progress && !all_done) {
    progress = false, all_done = true, ++sweeps;
    for (int i = 0; i < W; ++i) {
      const int wg = order ? W - 1 - i : i;
      if (l[wg] >= L) continue;
      all_done = false;
      // ONE step per sweep and workgroup: the interleaving is the sweep order
      if (l[wg] > 0 && cnt[(size_t)d256c_counter(l[wg] - 1, tm[wg], tiles_m, 1)] < tiles_n) continue; // waits
      ++computed[((size_t)l[wg] * tiles_m + tm[wg]) * tiles_n + wg_tn[wg]];
      if (l[wg] + 1 < L) ++cnt[(size_t)d256c_counter(l[wg], tm[wg], tiles_m, 1)];
      // (the kernel ends its walk behind the last layer's last block: chain_rounds_next then moves l to L)
      chain_rounds_next(tm[wg], l[wg], G, tiles_m);
      ++steps, progress = true;
    }
  }
  long once = 0, never = 0, more = 0, exact = 0, other = 0;
  for (int c : computed) (c == 1 ? once : c == 0 ? never : more)++;
  for (int c = 0; c < (L - 1) * tiles_m; ++c) (cnt[c] == tiles_n ? exact : other)++;
  printf("tiles once %ld never %ld more %ld\n", once, never, more);
  printf("arrivals exact %ld other %ld\n", exact, other);
  printf("run done %d steps %ld sweeps %ld\n", (int)all_done, steps, sweeps);
  return 0;
}
