// driver.cpp - TEST INFRASTRUCTURE for tests/test_chain_rounds_steps.py, never part of the product library.
//
// Walks tpp-mlir_amd/csrc/brgemm_bf16_lw_chain_rounds.h - the header the multi-round chain kernel includes - as plain host C++: for every
// tiles_m in 1 .. 40 and every G in 1 .. tiles_m, three layers, one line per group
//   <tiles_m> <G> <g> n<steps per layer> R<rounds> : <layer>.<row block>.<wait layer>.<wait row block> ...
// the steps in the order the kernel's walk (chain_rounds_next from tm = g, l = 0) makes them; a step of layer 0 waits for nothing (-1.-1),
// a later one for the counter of the row block it loads, in the layer before - as blw_loader computes it from the walk's tm.
// Then, per tile and a list of (tiles_m, tiles_n, cus): "rule <tiles_m> <tiles_n> <cus> gmax<Gmax> G<groups> R<rounds>".
#include "brgemm_bf16_lw_chain_rounds.h"
#include <initializer_list>
#include <stdio.h>

using namespace tpp;

static_assert(chain_rounds_steps(0, 2, 5) == 3 && chain_rounds_steps(1, 2, 5) == 2, "five row blocks on two groups: 3 and 2");
static_assert(chain_rounds_groups(64, 32) == 32 && chain_rounds_rounds(64, 32) == 2, "8192 rows of 128: G = 32, R = 2");
static_assert(chain_rounds_groups(33, 32) == 17 && chain_rounds_rounds(33, 17) == 2, "4224 rows of 128: G = 17, R = 2");
static_assert(chain_rounds_max_groups(8, 256) == 32 && chain_rounds_max_groups(300, 256) == 0, "groups that fit");

int main() {
  const int L = 3;
  for (int tiles_m = 1; tiles_m <= 40; ++tiles_m)
    for (int G = 1; G <= tiles_m; ++G)
      for (int g = 0; g < G; ++g) {
        printf("%d %d %d n%d R%d :", tiles_m, G, g, chain_rounds_steps(g, G, tiles_m), chain_rounds_rounds(tiles_m, G));
        int tm = g, l = 0, guard = 0;
        while (l < L && guard++ < 1000) {
          printf(" %d.%d.%d.%d", l, tm, l > 0 ? l - 1 : -1, l > 0 ? tm : -1);
          chain_rounds_next(tm, l, G, tiles_m);
        }
        printf("\n");
      }
  for (int tiles_n : {1, 2, 8, 16, 300})
    for (int cus : {256, 64, 304})
      for (int tiles_m = 1; tiles_m <= 300; tiles_m += (tiles_m < 70 ? 1 : 31)) { // (.. 69, 70, 101, .., 256, 287)
        const int gmax = chain_rounds_max_groups(tiles_n, cus);
        if (gmax < 1) printf("rule %d %d %d gmax0 G0 R0\n", tiles_m, tiles_n, cus);
        else printf("rule %d %d %d gmax%d G%d R%d\n", tiles_m, tiles_n, cus, gmax, chain_rounds_groups(tiles_m, gmax), chain_rounds_rounds(tiles_m, chain_rounds_groups(tiles_m, gmax)));
      }
  return 0;
}
