// Walks the schedule of a mixed-width layer chain (tpp-mlir_amd/csrc/brgemm_bf16_lw_chain_widths.h) for tests/test_chain_widths_schedule.py: for
// every loader-wave tile 0 .. 3 and a list of width vectors (in column tiles), the events of every workgroup's LOADER role and MFMA role,
// written from the header's functions the way brgemm_bf16_lw.hip's blw_loader and MFMA loop use them. One line per role:
//   case <tile> <nslot> <wk> <nla> <L> <tiles of layer 0> .. <chunks of layer 0> ..
//   wg <tn> first <l> last <l>
//   L <events>          M <events>
// events: s<l>:<slot> the layer starts at ring slot, W<l>:<counter layer> a bounded wait in front of layer l, S2:<l> P:<l> m:<l> (one per further
// chunk) R1:<l> S1:<l> barriers, A<l> one arrival at cnt[l][tm], I<l>:<layer> the B loaders' run-ahead loads that layer's state.
//   target <l> <epoch> <value>     chain_widths_target for epochs 1, 2, 3, 0x80000000 and 0xffffffff
#include "brgemm_bf16_lw_launch.h"
#include <cstdio>
#include <vector>

using namespace tpp;

int main() {
  const std::vector<std::vector<int>> vectors = {{1, 4, 1}, {1, 2, 4}, {8, 4, 2, 1}, {2, 1, 2, 1, 2, 1, 2, 1}, {2, 2, 2}, {3, 1, 2}, {1, 3, 1}, {3, 1, 3}, {1, 3, 3}, {4, 1}, {4, 2, 4}};
  for (int tile = 0; tile < 4; ++tile) {
    const BlwTile t = BLW_TILES[tile];
    const int bn = t.bn();
    for (const auto &v : vectors) {
      const int L = (int)v.size();
      std::vector<int> n(L), T(L);
      for (int l = 0; l < L; ++l) n[l] = v[l] * bn, T[l] = l == 0 ? 9 : n[l - 1] / 64; // (layer 0: k = 576, an odd count no ring is short of; later layers read their predecessor)
      auto n_of = [&](int l) { return n[l]; };
      printf("case %d %d %d %d %d", tile, t.nslot, t.wk, t.nla, L);
      for (int l = 0; l < L; ++l) printf(" %d", chain_widths_tiles(n[l], bn));
      for (int l = 0; l < L; ++l) printf(" %d", T[l]);
      printf("\n");
      bool ahead = true;
      for (int l = 0; l < L; ++l)
        if (T[l] < t.nslot) ahead = false;
      const int grid = chain_widths_grid(L, bn, n_of);
      for (int tn = 0; tn < grid; ++tn) {
        printf("wg %d first %d last %d\n", tn, chain_widths_first(tn, L, bn, n_of), chain_widths_last(tn, L, bn, n_of));
        // the loader role (blw_loader: the A loader that polls; the B loaders differ by the run-ahead alone)
        printf("L");
        int s0 = 0;
        for (int lc = 0; lc < L; ++lc) {
          if (!chain_widths_active(tn, n[lc], bn)) continue;
          printf(" s%d:%d", lc, s0);
          if (chain_widths_waits(lc)) printf(" W%d:%d", lc, lc - 1);
          if (t.nla > 1 && lc > 0) printf(" S2:%d", lc);
          printf(" P:%d", lc);
          for (int c = 0; c + 1 < T[lc]; ++c) printf(" m:%d", lc);
          const int nxt = chain_widths_next(tn, lc, L, bn, n_of);
          if (ahead && nxt < L) printf(" I%d:%d", lc, nxt);
          if (lc + 1 == L) break;
          if (t.wk > 1) printf(" R1:%d", lc);
          printf(" S1:%d", lc);
          s0 = chain_widths_next_s0(s0, T[lc], t.nslot);
        }
        printf("\nM");
        s0 = 0;
        for (int l = 0; l < L; ++l) {
          if (!chain_widths_active(tn, n[l], bn)) continue;
          printf(" s%d:%d", l, s0);
          if (t.nla > 1 && l > 0) printf(" S2:%d", l);
          printf(" P:%d", l);
          for (int c = 0; c + 1 < T[l]; ++c) printf(" m:%d", l);
          s0 = chain_widths_next_s0(s0, T[l], t.nslot);
          if (t.wk > 1) printf(" R1:%d", l);
          if (!chain_widths_signals(l, L)) break;
          printf(" S1:%d A%d", l, l);
        }
        printf("\n");
      }
      const unsigned epochs[5] = {1u, 2u, 3u, 0x80000000u, 0xffffffffu};
      for (int l = 0; l < L; ++l)
        for (unsigned e : epochs) printf("target %d %u %u\n", l, e, chain_widths_target(e, n[l], bn));
    }
  }
  // blw_chain_widths_launch_ok: one accepted launch and one refusal per term ("ok <what> <answer>")
  {
    const BlwWidthsShape good{128, 3, {192, 64, 128}, {192, 192, 64}, {1, 1, 1}};
    auto say = [](const char *what, int tile, int b_kind, BlwWidthsShape a) { printf("ok %s %d\n", what, (int)blw_chain_widths_launch_ok(tile, b_kind, a)); };
    say("accepted", 1, 0, good);
    say("tile-4", 4, 0, good);
    say("b-kind-1", 1, 1, good);
    { BlwWidthsShape a = good; a.nlayers = 1; say("one-layer", 1, 0, a); }
    { BlwWidthsShape a = good; a.nlayers = 9; say("nine-layers", 1, 0, a); }
    { BlwWidthsShape a = good; a.br[1] = 0; say("empty-batch", 1, 0, a); }
    { BlwWidthsShape a = good; a.k[0] = 32; say("k-below-64", 1, 0, a); }
    { BlwWidthsShape a = good; a.k[0] = 200; say("k-not-in-chunks", 1, 0, a); }
    { BlwWidthsShape a = good; a.n[1] = 0; say("n-below-bn", 1, 0, a); }
    { BlwWidthsShape a = good; a.n[1] = 96; say("n-not-in-tiles", 1, 0, a); }
    { BlwWidthsShape a = good; a.n[0] = a.n[1] = a.n[2] = 128; say("equal-widths", 1, 0, a); }
    { BlwWidthsShape a = good; a.m = 32; say("m-below-bm", 1, 0, a); }
    { BlwWidthsShape a = good; a.m = 160; say("m-not-in-blocks", 1, 0, a); }
    say("n-not-in-tiles-of-128", 3, 0, good);
    printf("inst");
    for (int tile = -1; tile <= 4; ++tile)
      for (int b_kind = 0; b_kind <= 4; ++b_kind)
        for (int sup = 1; sup <= 2; ++sup)
          if (blw_chain_widths_instance_exists(tile, b_kind, sup)) printf(" %d:%d:%d", tile, b_kind, sup);
    printf("\n");
    // the modes beside the table stay outside it
    printf("table %d %d %d %d\n", BLW_MODES, BLW_CHAIN_WIDTHS, (int)blw_instance_exists(BLW_CHAIN_WIDTHS, true, 1, 0, 1), (int)blw_launch_ok(BLW_CHAIN_WIDTHS, 1, 0, BlwShape{true, 128, 128, 3, 0, {192, 128, 128}, {1, 1, 1}}));
  }
  return 0;
}
