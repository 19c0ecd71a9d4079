// Walks the schedule of a ragged mixed-width layer chain (tpp-mlir_amd/csrc/brgemm_bf16_lw_chain_wragged.h and the headers it builds on) for
// tests/test_chain_wragged_schedule.py: for every loader-wave tile 0 .. 3 and a list of shapes (m, per layer n, k, batch count, in units of
// the tile), every workgroup's loader role and MFMA role, written from the headers' functions the way brgemm_bf16_lw.hip's blw_loader and
// MFMA loop use them in launch mode 11. The checks are made here; the output is
//   case <tile> <shape> <m> <L> n .. k .. br ..        one per (tile, shape)
//   fail <tile> <shape> <what>                        a property that does not hold (none expected)
//   arrivals <tile> <shape> <l> <tm> <count> <want>   per counter and launch
//   seen <what> <count>                               features the shape list exercised, summed over all cases
//   ok <what> <answer> / inst .. / table ..           blw_chain_wragged_launch_ok, _instance_exists, and the launch table's refusal
#include "brgemm_bf16_lw_launch.h"
#include <cstdio>
#include <map>
#include <string>
#include <vector>

using namespace tpp;

struct Shape {
  const char *name;
  int m_bm, m_add;                 // m = m_bm * BM + m_add
  std::vector<int> n_bn, n_add;    // n(l) = n_bn * BN + n_add
  int k0, br0;                     // layer 0 (later layers read their predecessor: k = n(l - 1), one batch element, unless brs says otherwise)
  int br_later;                    // batch elements of every later layer (k = n(l - 1) / br_later; must stay a multiple of 8 and >= 64)
};

static std::map<std::string, long> seen;
static int g_tile;
static const char *g_shape;
static void fail(const char *what) { printf("fail %d %s %s\n", g_tile, g_shape, what); }

int main() {
  const std::vector<Shape> shapes = {
      {"sitout-resume", 1, 8, {3, 1, 2}, {8, 8, 24}, 192, 1, 1},
      {"sitout-resume-3bm-3", 3, -3, {3, 1, 2}, {8, 8, 24}, 192, 1, 1},
      {"first-active-later", 1, 8, {1, 3, 1}, {8, 0, 16}, 128, 1, 1},
      {"first-active-later-3bm-3", 3, -3, {1, 3, 1}, {8, 0, 16}, 128, 1, 1},
      {"2bn-next-to-2bn+8", 2, 0, {2, 2, 1}, {0, 8, 0}, 72, 1, 1},
      {"2bn+8-next-to-2bn", 1, 8, {2, 2, 1}, {8, 0, 8}, 64, 2, 1},
      {"k72", 1, 8, {4, 2, 1}, {0, 0, 0}, 72, 1, 1},
      {"k80", 1, 8, {4, 2, 1}, {0, 0, 0}, 80, 1, 1},
      {"k88", 3, -3, {4, 2, 1}, {0, 0, 0}, 88, 1, 1},
      {"k96", 3, -3, {4, 2, 1}, {0, 0, 0}, 96, 1, 1},
      {"k104", 1, 8, {4, 2, 1}, {0, 0, 0}, 104, 1, 1},
      {"k112", 2, 0, {4, 2, 1}, {0, 0, 0}, 112, 1, 1},
      {"k120", 1, 8, {4, 2, 1}, {0, 0, 0}, 120, 1, 1},
      {"k200", 3, -3, {4, 2, 1}, {0, 0, 0}, 200, 1, 1},
      {"ragged-m-only", 3, -3, {3, 1, 2}, {0, 0, 0}, 192, 1, 1},
      {"twelve-chunks", 1, 8, {2, 1}, {0, 0}, 200, 3, 1},
      {"eight-layers", 1, 8, {2, 1, 2, 1, 2, 1, 2, 1}, {8, 8, 8, 8, 8, 8, 8, 8}, 136, 1, 1},
      {"two-batch-elements", 3, -3, {2, 2, 1}, {16, 16, 8}, 144, 2, 2},
  };
  for (int tile = 0; tile < 4; ++tile) {
    const BlwTile t = BLW_TILES[tile];
    const int bm = t.bm(), bn = t.bn(), nslot = t.nslot;
    for (const Shape &sh : shapes) {
      g_tile = tile, g_shape = sh.name;
      const int L = (int)sh.n_bn.size(), m = sh.m_bm * bm + sh.m_add;
      std::vector<int> n(L), k(L), br(L);
      for (int l = 0; l < L; ++l) {
        n[l] = sh.n_bn[l] * bn + sh.n_add[l];
        br[l] = l == 0 ? sh.br0 : sh.br_later;
        k[l] = l == 0 ? sh.k0 : n[l - 1] / br[l];
        if (!chain_ragged_k_ok(k[l]) || n[l] % 8 != 0 || n[l] < bn) fail("the shape list names a layer the mode does not take");
      }
      auto n_of = [&](int l) { return n[l]; };
      printf("case %d %s %d %d", tile, sh.name, m, L);
      for (int l = 0; l < L; ++l) printf(" %d", n[l]);
      for (int l = 0; l < L; ++l) printf(" %d", k[l]);
      for (int l = 0; l < L; ++l) printf(" %d", br[l]);
      printf("\n");
      {
        BlwWidthsShape a{m, L, {}, {}, {}};
        for (int l = 0; l < L; ++l) a.n[l] = n[l], a.k[l] = k[l], a.br[l] = br[l];
        if (!blw_chain_wragged_launch_ok(tile, 2, a)) fail("blw_chain_wragged_launch_ok refuses the shape");
      }
      const int tiles_m = chain_edge_tiles_m(m, bm), grid = chain_wragged_grid(L, bn, n_of);
      // ---- rows: loads inside [0, m), every row stored by exactly one row block
      {
        std::vector<int> rows(m, 0);
        for (int tm = 0; tm < tiles_m; ++tm) {
          const int r0 = chain_edge_row0(tm, tiles_m, m, bm);
          if (r0 < 0 || r0 + bm > m) fail("a row block loads outside [0, m)");
          if (r0 + chain_edge_own_row(tm, tiles_m, m, bm) != chain_edge_store_begin(tm, tiles_m, m, bm)) fail("own_row and store_begin disagree");
          for (int r = chain_edge_store_begin(tm, tiles_m, m, bm); r < chain_edge_store_end(tm, tiles_m, m, bm); ++r) {
            if (r < r0 || r >= r0 + bm) fail("a row block stores a row it did not compute");
            else ++rows[r];
          }
          const int bf = chain_edge_first_block(tm, tiles_m, m, bm), bl = chain_edge_last_block(tm, tiles_m, m, bm);
          if (bf < 0 || bl != tm || bl - bf > 1) fail("a seam waits on other than one or two row blocks");
          for (int r = r0; r < r0 + bm; ++r)
            if (r / bm < bf || r / bm > bl) fail("a row block reads a row whose producer it does not wait for");
          if (bl > bf) ++seen["two-counter-wait"];
        }
        for (int r = 0; r < m; ++r)
          if (rows[r] != 1) fail("a row is not stored exactly once");
        if (m % bm) ++seen["ragged-m"];
      }
      // ---- columns, per layer: loads inside [0, n(l)), every column stored by exactly one ACTIVE workgroup column, none outside the window
      for (int l = 0; l < L; ++l) {
        std::vector<int> cols(n[l], 0);
        int active = 0;
        for (int tn = 0; tn < grid; ++tn) {
          if (!chain_wragged_active(tn, n[l], bn)) {
            if (tn < chain_wragged_tiles(n[l], bn)) fail("a column tile of the layer is not active");
            continue;
          }
          if (tn >= chain_wragged_tiles(n[l], bn)) fail("a workgroup without a column tile is active");
          ++active;
          const int c0 = chain_ragged_col0(tn, n[l], bn), own = chain_ragged_own_col(tn, n[l], bn);
          if (c0 < 0 || c0 + bn > n[l]) fail("a column tile loads outside [0, n(l))");
          if (own < 0 || own >= bn || own % 8 != 0 || c0 % 8 != 0) fail("the own-column offset is not a whole number of 16-byte pieces inside the tile");
          for (int c = c0 + own; c < c0 + bn; ++c) ++cols[c];
          if (own > 0) ++seen["shifted-column-tile"];
        }
        for (int c = 0; c < n[l]; ++c)
          if (cols[c] != 1) fail("a column is not stored exactly once");
        if (active != chain_wragged_tiles(n[l], bn)) fail("active workgroups and column tiles disagree");
      }
      // ---- k, per layer: every k-value of every batch element multiplied exactly once, all reads inside [0, k)
      for (int l = 0; l < L; ++l) {
        const int T = chain_ragged_layer_chunks(k[l], br[l]);
        std::vector<std::vector<int>> mult(br[l], std::vector<int>(k[l], 0));
        int tested = 0;
        for (int c = 0; c < T; ++c) {
          const int b = chain_ragged_batch(k[l], c), k0 = chain_ragged_chunk_k0(k[l], c);
          if (b < 0 || b >= br[l] || k0 < 0 || k0 + BKEDGE_BK > k[l]) fail("a chunk lies outside its batch element");
          const int skip = chain_ragged_skip_halves(k[l], c);
          if (skip) ++seen["skip-" + std::to_string(skip)], ++tested;
          for (int s = 0; s < 4; ++s) {
            const int part = chain_ragged_step_part(k[l], c, s);
            const int lo = part == BKEDGE8_WHOLE ? 0 : part == BKEDGE8_UPPER ? 8 : 16;
            for (int q = lo; q < 16; ++q) ++mult[b][k0 + 16 * s + q];
          }
        }
        for (int b = 0; b < br[l]; ++b)
          for (int q = 0; q < k[l]; ++q)
            if (mult[b][q] != 1) fail("a k-value is not multiplied exactly once");
        // the K loop's test period: the tested chunks are exactly every period-th one
        const int period = chain_ragged_test_period(k[l], T);
        for (int c = 0; c < T; ++c)
          if ((chain_ragged_skip_halves(k[l], c) != 0) != ((c + 1) % period == 0 && period <= T)) fail("the test period misses or invents a tested chunk");
        if (T == 12) ++seen["twelve-chunk-layer"];
        (void)tested;
      }
      // ---- per workgroup column: both roles walk the same layers, count the same ring slots, and no slot is refilled before it was consumed
      for (int tn = 0; tn < grid; ++tn) {
        const int first = chain_widths_first(tn, L, bn, n_of), last = chain_widths_last(tn, L, bn, n_of);
        if (first < 0 || first >= L || last < first) fail("a workgroup without an active layer");
        if (first > 0) ++seen["first-active-layer-later"];
        if (last + 1 < L) ++seen["last-active-layer-not-the-chain-s-last"];
        // the MFMA role: s0 through chain_wragged_s0, slots through chain_ragged_slot
        std::vector<std::vector<int>> mslot(L);
        for (int l = 0; l < L; ++l) {
          if (!chain_wragged_active(tn, n[l], bn)) continue;
          const int s0 = chain_wragged_s0(tn, l, bn, n_of, k.data(), br.data(), nslot);
          for (int c = 0; c < chain_ragged_layer_chunks(k[l], br[l]); ++c) mslot[l].push_back(chain_ragged_slot(s0, c, nslot));
        }
        // the loader role: a running slot, set to s0 at every active layer (no run-ahead), s0 moved by chain_wragged_next_s0
        int s0 = 0, prev_active = -1;
        std::vector<int> owner_layer(nslot, -1), owner_chunk(nslot, -1);
        for (int lc = 0; lc < L; ++lc) {
          const bool act = chain_wragged_active(tn, n[lc], bn);
          if (act) {
            if (prev_active >= 0 && lc > prev_active + 1) ++seen["sit-out-and-resume"];
            if (prev_active >= 0 && (chain_ragged_own_col(tn, n[lc], bn) > 0) != (chain_ragged_own_col(tn, n[prev_active], bn) > 0)) ++seen["shifted-in-one-layer-interior-in-another"];
            prev_active = lc;
            const int T = chain_ragged_layer_chunks(k[lc], br[lc]);
            int slot = s0, issued = 0, consumed = 0; // chunks requested / retired (chunk t - 1 retires at the barrier in chunk t)
            auto issue = [&]() {
              // the slot's previous owner: a chunk of an earlier layer (its seam lies behind: consumed) or chunk issued - nslot of this one
              if (owner_layer[slot] == lc && owner_chunk[slot] >= consumed) fail("a ring slot is refilled before its chunk was consumed");
              if ((int)mslot[lc].size() != T || mslot[lc][issued] != slot) fail("loader and MFMA waves disagree on a chunk's ring slot");
              owner_layer[slot] = lc, owner_chunk[slot] = issued++;
              slot = chain_ragged_next_slot(slot, nslot);
            };
            const int npro = T < nslot - 1 ? T : nslot - 1;
            for (int c = 0; c < npro; ++c) issue();
            for (int tt = 0; tt + nslot - 1 < T; ++tt) {
              consumed = tt; // (the barrier in the middle of chunk tt: chunks < tt are retired)
              issue();
            }
            if (issued != T) fail("the loader does not request every chunk of a layer");
            if (s0 != 0) ++seen["layer-starts-at-a-later-slot"];
            if (s0 & 1) ++seen["layer-starts-at-an-odd-slot"];
          }
          s0 = chain_wragged_next_s0(s0, act, k[lc], br[lc], nslot);
        }
      }
      // ---- counters and progress: all workgroups round-robin, each blocking at its waits; three epochs from a counter state just below
      //      the unsigned wrap of the epoch
      {
        const unsigned e0 = 0xfffffffeu;
        std::vector<std::vector<unsigned>> cnt(L, std::vector<unsigned>(tiles_m));
        for (int l = 0; l < L; ++l)
          for (int tm = 0; tm < tiles_m; ++tm) cnt[l][tm] = chain_wragged_target(e0, n[l], bn);
        for (unsigned step = 1; step <= 3; ++step) {
          const unsigned epoch = e0 + step; // 0xffffffff, 0 (the wrap), 1
          struct Op { bool wait; int l; };
          std::vector<std::vector<Op>> prog(tiles_m * grid);
          std::vector<size_t> pc(tiles_m * grid, 0);
          std::vector<std::vector<unsigned>> before = cnt;
          for (int tm = 0; tm < tiles_m; ++tm)
            for (int tn = 0; tn < grid; ++tn)
              for (int l = 0; l < L; ++l) {
                if (!chain_wragged_active(tn, n[l], bn)) continue;
                if (chain_widths_waits(l)) prog[tm * grid + tn].push_back(Op{true, l});
                if (chain_widths_signals(l, L)) prog[tm * grid + tn].push_back(Op{false, l});
              }
          for (int order = 0; order < 2; ++order) {
            if (order == 1) {
              cnt = before;
              for (auto &p : pc) p = 0;
            }
            bool moved = true, done = false;
            while (moved && !done) {
              moved = false, done = true;
              for (int i0 = 0; i0 < tiles_m * grid; ++i0) {
                const int i = order ? tiles_m * grid - 1 - i0 : i0, tm = i / grid;
                while (pc[i] < prog[i].size()) {
                  const Op op = prog[i][pc[i]];
                  if (op.wait) {
                    const unsigned target = chain_wragged_target(epoch, n[op.l - 1], bn);
                    bool ready = true;
                    for (int b = chain_edge_first_block(tm, tiles_m, m, bm); b <= chain_edge_last_block(tm, tiles_m, m, bm); ++b)
                      if ((int)(cnt[op.l - 1][b] - target) < 0) ready = false; // (the kernel's comparison)
                    if (!ready) break;
                  } else {
                    ++cnt[op.l][tm];
                  }
                  ++pc[i];
                  moved = true;
                }
                if (pc[i] < prog[i].size()) done = false;
              }
            }
            if (!done) fail("the round-robin run of all workgroups does not complete: a cyclic wait");
          }
          for (int l = 0; l < L; ++l)
            for (int tm = 0; tm < tiles_m; ++tm) {
              const unsigned got = cnt[l][tm] - before[l][tm], want = l + 1 < L ? (unsigned)chain_wragged_tiles(n[l], bn) : 0u;
              if (step == 1) printf("arrivals %d %s %d %d %u %u\n", tile, sh.name, l, tm, got, want);
              if (got != want) fail("a counter does not receive ceil(n(l) / BN) arrivals per launch");
              if (l + 1 < L && cnt[l][tm] != chain_wragged_target(epoch, n[l], bn)) fail("a counter is not at its target after the launch");
            }
          if (epoch == 0) ++seen["epoch-wraps"];
        }
      }
      if (L == 8) ++seen["eight-layers"];
    }
  }
  for (const auto &s : seen) printf("seen %s %ld\n", s.first.c_str(), s.second);
  // blw_chain_wragged_launch_ok: one accepted launch and one refusal per term ("ok <what> <answer>")
  {
    const BlwWidthsShape good{136, 3, {200, 72, 128}, {200, 200, 72}, {1, 1, 1}};
    auto say = [](const char *what, int tile, int b_kind, BlwWidthsShape a) { printf("ok %s %d\n", what, (int)blw_chain_wragged_launch_ok(tile, b_kind, a)); };
    say("accepted", 1, 0, good);
    say("tile-4", 4, 0, good);
    say("b-kind-1", 1, 1, good);
    say("no-instance", 2, 0, BlwWidthsShape{136, 2, {264, 136}, {200, 264}, {1, 1}});
    say("its-flat-instance", 2, 2, BlwWidthsShape{136, 2, {264, 136}, {200, 264}, {1, 1}});
    { BlwWidthsShape a = good; a.nlayers = 1; say("one-layer", 1, 0, a); }
    { BlwWidthsShape a = good; a.nlayers = 9; say("nine-layers", 1, 0, a); }
    { BlwWidthsShape a = good; a.br[1] = 0; say("empty-batch", 1, 0, a); }
    { BlwWidthsShape a = good; a.k[0] = 56; say("k-below-64", 1, 0, a); }
    { BlwWidthsShape a = good; a.k[0] = 204; say("k-not-a-multiple-of-8", 1, 0, a); }
    { BlwWidthsShape a = good; a.n[1] = 56; say("n-below-bn", 1, 0, a); }
    { BlwWidthsShape a = good; a.n[1] = 76; say("n-not-a-multiple-of-8", 1, 0, a); }
    { BlwWidthsShape a = good; a.n[0] = a.n[1] = a.n[2] = 200; say("equal-widths", 1, 0, a); }
    { BlwWidthsShape a = good; a.m = 56; say("m-below-bm", 1, 0, a); }
    say("divided-entirely", 1, 0, BlwWidthsShape{128, 3, {192, 64, 128}, {192, 192, 64}, {1, 1, 1}});
    say("ragged-m-alone", 1, 0, BlwWidthsShape{136, 3, {192, 64, 128}, {192, 192, 64}, {1, 1, 1}});
    say("ragged-k-alone", 1, 0, BlwWidthsShape{128, 3, {192, 64, 128}, {200, 192, 64}, {1, 1, 1}});
    say("ragged-n-alone", 1, 0, BlwWidthsShape{128, 3, {192, 72, 128}, {192, 192, 128}, {1, 1, 1}});
    printf("inst");
    for (int tile = -1; tile <= 4; ++tile)
      for (int b_kind = 0; b_kind <= 4; ++b_kind)
        if (blw_chain_wragged_instance_exists(tile, b_kind)) printf(" %d:%d", tile, b_kind);
    printf("\n");
    // the modes beside the table stay outside it
    printf("table %d %d %d %d\n", BLW_MODES, BLW_CHAIN_WRAGGED, (int)blw_instance_exists(BLW_CHAIN_WRAGGED, true, 1, 0, 1),
           (int)blw_launch_ok(BLW_CHAIN_WRAGGED, 1, 0, BlwShape{true, 136, 200, 3, 0, {200, 200, 200}, {1, 1, 1}}));
  }
  return 0;
}
