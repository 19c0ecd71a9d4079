// Walks the schedule of a mixed-width layer chain in column rounds (tpp-mlir_amd/csrc/brgemm_bf16_lw_chain_wrounds.h) for
// tests/test_chain_width_rounds_schedule.py and tests/test_chain_width_rounds_launch.py: for every loader-wave tile 0 .. 3, a list of width
// vectors (in column tiles) and every W from 1 to max T (max T itself: the one-round walk, for comparison), the events of every column
// group's LOADER role and MFMA role, written from the header's functions the way brgemm_bf16_lw.hip's blw_loader and MFMA loop use them.
//   case <tile> <nslot> <wk> <nla> <L> <W> <tiles of layer 0> .. <chunks of layer 0> ..
//   wg <c> steps <steps in layer 0> ..
//   L <events>          M <events>
// events: s<l>:<tn>:<slot> a step of layer l on column tile tn starts at ring slot, W<l> a bounded wait for cnt[l - 1][tm] in front of it,
// P:<l> m:<l> (one per further chunk) R1:<l> S1:<l> barriers, A<l> one arrival at cnt[l][tm], I<l>:<tn> the B loaders' run-ahead loads the
// state of that step.
// With the argument "launch": blw_chain_wrounds_launch_ok's answers ("ok <what> <answer>"), the instances ("inst <tile>:<b_kind> ..") and
// the launch table's view of the mode ("table ..").
#include "brgemm_bf16_lw_launch.h"
#include <cstdio>
#include <cstring>
#include <vector>

using namespace tpp;

static int launch_part() {
  const BlwWidthsShape good{128, 3, {256, 64, 128}, {192, 256, 64}, {1, 1, 1}};
  auto say = [](const char *what, int tile, int b_kind, BlwWidthsShape a, int groups) { printf("ok %s %d\n", what, (int)blw_chain_wrounds_launch_ok(tile, b_kind, a, groups)); };
  say("accepted", 1, 0, good, 2);
  say("accepted-one-group", 1, 0, good, 1);
  say("tile-4", 4, 0, good, 2);
  say("b-kind-1", 1, 1, good, 2);
  { BlwWidthsShape a = good; a.nlayers = 1; say("one-layer", 1, 0, a, 2); }
  { BlwWidthsShape a = good; a.nlayers = 9; say("nine-layers", 1, 0, a, 2); }
  { BlwWidthsShape a = good; a.br[1] = 0; say("empty-batch", 1, 0, a, 2); }
  { BlwWidthsShape a = good; a.k[0] = 32; say("k-below-64", 1, 0, a, 2); }
  { BlwWidthsShape a = good; a.k[0] = 200; say("k-not-in-chunks", 1, 0, a, 2); }
  { BlwWidthsShape a = good; a.n[1] = 0; say("n-below-bn", 1, 0, a, 2); }
  { BlwWidthsShape a = good; a.n[1] = 96; say("n-not-in-tiles", 1, 0, a, 2); }
  { BlwWidthsShape a = good; a.n[0] = a.n[1] = a.n[2] = 128; say("equal-widths", 1, 0, a, 1); }
  { BlwWidthsShape a = good; a.m = 32; say("m-below-bm", 1, 0, a, 2); }
  { BlwWidthsShape a = good; a.m = 160; say("m-not-in-blocks", 1, 0, a, 2); }
  say("groups-zero", 1, 0, good, 0);
  say("groups-negative", 1, 0, good, -1);
  say("groups-widest", 1, 0, good, 4);
  say("groups-above-widest", 1, 0, good, 5);
  printf("inst");
  for (int tile = -1; tile <= 4; ++tile)
    for (int b_kind = 0; b_kind <= 4; ++b_kind)
      if (blw_chain_wrounds_instance_exists(tile, b_kind)) printf(" %d:%d", tile, b_kind);
  printf("\n");
  // the modes beside the table stay outside it
  printf("table %d %d %d %d\n", BLW_MODES, BLW_CHAIN_WROUNDS, (int)blw_instance_exists(BLW_CHAIN_WROUNDS, true, 1, 0, 1),
         (int)blw_launch_ok(BLW_CHAIN_WROUNDS, 1, 0, BlwShape{true, 128, 128, 3, 2, {192, 128, 128}, {1, 1, 1}}));
  return 0;
}

int main(int argc, char **argv) {
  if (argc > 1 && !strcmp(argv[1], "launch")) return launch_part();
  const std::vector<std::vector<int>> vectors = {{4, 1, 2}, {1, 3, 1}, {2, 1, 2, 1, 2, 1, 2, 1}, {2, 2, 1}, {3, 1}, {4, 2}, {1, 4, 1}, {8, 4, 2, 1}, {5, 2, 7, 3}, {1, 2, 4}};
  for (int tile = 0; tile < 4; ++tile) {
    const BlwTile t = BLW_TILES[tile];
    const int bn = t.bn();
    for (const auto &v : vectors) {
      const int L = (int)v.size();
      std::vector<int> n(L), T(L), K(L);
      for (int l = 0; l < L; ++l) n[l] = v[l] * bn, K[l] = n[l] / bn, T[l] = l == 0 ? 9 : n[l - 1] / 64; // (layer 0: k = 576; later layers read their predecessor)
      auto n_of = [&](int l) { return n[l]; };
      bool ahead = true;
      for (int l = 0; l < L; ++l)
        if (T[l] < t.nslot) ahead = false;
      const int maxT = chain_widths_grid(L, bn, n_of);
      for (int W = 1; W <= maxT; ++W) {
        printf("case %d %d %d %d %d %d", tile, t.nslot, t.wk, t.nla, L, W);
        for (int l = 0; l < L; ++l) printf(" %d", K[l]);
        for (int l = 0; l < L; ++l) printf(" %d", T[l]);
        printf("\n");
        for (int c = 0; c < W; ++c) {
          printf("wg %d steps", c);
          for (int l = 0; l < L; ++l) printf(" %d", chain_wrounds_steps(c, W, K[l]));
          // the loader role (blw_loader: the A loader that polls; the B loaders differ by the run-ahead alone)
          printf("\nL");
          int s0 = 0, tn = c;
          for (int lc = 0; lc < L; chain_wrounds_next(tn, lc, W, K[lc])) {
            if (!chain_widths_active(tn, n[lc], bn)) continue;
            printf(" s%d:%d:%d", lc, tn, s0);
            if (chain_widths_waits(lc)) printf(" W%d", lc);
            printf(" P:%d", lc);
            for (int i = 0; i + 1 < T[lc]; ++i) printf(" m:%d", lc);
            const bool more = chain_wrounds_more(tn, W, K[lc]);
            const int ntn = more ? tn + W : chain_wrounds_group(tn, W);
            const int nxt = more ? lc : chain_widths_next(ntn, lc, L, bn, n_of);
            if (ahead && nxt < L) printf(" I%d:%d", nxt, ntn);
            if (lc + 1 == L && !more) break;
            if (t.wk > 1) printf(" R1:%d", lc);
            printf(" S1:%d", lc);
            s0 = chain_widths_next_s0(s0, T[lc], t.nslot);
          }
          printf("\nM");
          s0 = 0, tn = c;
          for (int l = 0; l < L; chain_wrounds_next(tn, l, W, K[l])) {
            if (!chain_widths_active(tn, n[l], bn)) continue;
            printf(" s%d:%d:%d", l, tn, s0);
            printf(" P:%d", l);
            for (int i = 0; i + 1 < T[l]; ++i) printf(" m:%d", l);
            s0 = chain_widths_next_s0(s0, T[l], t.nslot);
            if (t.wk > 1) printf(" R1:%d", l);
            if (!chain_widths_signals(l, L)) {
              if (!chain_wrounds_more(tn, W, K[l])) break;
              printf(" S1:%d", l);
              continue;
            }
            printf(" S1:%d A%d", l, l);
          }
          printf("\n");
        }
      }
    }
  }
  // the rule's W: "groups <maxT> <tiles_m> <cus> <wfit> <W or 0>"
  const int probes[][3] = {{64, 16, 256}, {32, 32, 256}, {32, 16, 256}, {10, 32, 256}, {10, 32, 304}, {4, 2, 256}, {2, 300, 256}, {1, 4, 256}, {7, 3, 16}};
  for (const auto &p : probes) {
    const int wfit = chain_wrounds_max_groups(p[0], p[1], p[2]);
    printf("groups %d %d %d %d %d\n", p[0], p[1], p[2], wfit, wfit >= 1 ? chain_wrounds_groups(p[0], wfit) : 0);
  }
  return 0;
}
