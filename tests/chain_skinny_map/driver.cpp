// driver.cpp - TEST INFRASTRUCTURE for tests/test_chain_skinny_map.py, never part of the product library.
//
// Walks the schedule of the skinny-batch layer chain (tpp-mlir_amd/csrc/brgemm_bf16_skinny_chain.h, on top of brgemm_bf16_skinny.h) as plain host
// C++: for G = 1 .. 9 resident workgroups, BN = 16 / 32 / 64 and chains of 2 .. 4 layers whose widths give 1 .. 20 column blocks, mixed per
// layer, with and without a shifted last block -
//   a  every (layer, block) is owned by exactly one workgroup, and skc_owner names it
//   b  every workgroup arrives exactly once per seam: a launch adds exactly G to each of nlayers - 1 counters
//   c  per layer the deal over W_l waves is the single call's (skn_wave_first / _count with skn_waves), and waves beyond take nothing
//   d  every column of every layer is stored exactly once, the shifted last block included
//   e  a simulation of the waits terminates under several workgroup orders - ascending, descending, one workgroup run as far as it gets, a
//      shuffled round robin - over three launches on the same monotonic counters (targets epoch * G), and leaves every counter at 3 G
// Prints the counts and "OK"; exit code 1 and FAIL lines otherwise.
#include "../../tpp-mlir_amd/csrc/brgemm_bf16_skinny_chain.h"
#include <cstdint>
#include <cstdio>
#include <vector>

using namespace tpp;

static int g_fail = 0;
#define FAIL(...)                            \
  do {                                       \
    if (g_fail++ < 50) {                     \
      printf("FAIL: " __VA_ARGS__);          \
      printf("\n");                          \
    }                                        \
  } while (0)

static uint32_t g_lcg = 2024;
static uint32_t lcg() { return g_lcg = g_lcg * 1664525u + 1013904223u; }

// one workgroup's program: per layer [wait for seam l - 1] [its blocks] [arrive at seam l]
struct Wg {
  int layer = 0, block_i = 0;
  bool waited = false, done = false;
};

// runs workgroup w until it blocks or ends; returns whether it made progress
static bool run_wg(Wg &s, int w, int G, int bn, const std::vector<int> &ns, std::vector<unsigned> &cnt, unsigned epoch, bool one_step) {
  const int L = (int)ns.size();
  bool progress = false;
  while (!s.done) {
    const int blocks = skn_blocks(ns[s.layer], bn), owned = skc_owned(w, G, blocks);
    if (skc_waits(w, G, s.layer, blocks) && !s.waited) {
      if ((int)(cnt[s.layer - 1] - skc_target(epoch, G)) < 0) return progress; // blocked
      s.waited = true;
    }
    if (s.block_i < owned) {
      ++s.block_i; // (computes and stores block skc_block(w, G, block_i))
    }
    if (s.block_i >= owned) {
      if (skc_signals(s.layer, L)) ++cnt[s.layer]; // behind the last block, or at once
      ++s.layer, s.block_i = 0, s.waited = false;
      if (s.layer == L) s.done = true;
    }
    progress = true;
    if (one_step) return true;
  }
  return progress;
}

static long g_sims = 0;
static void simulate(int G, int bn, const std::vector<int> &ns) {
  const int L = (int)ns.size();
  for (int order = 0; order < 4; ++order) {
    std::vector<unsigned> cnt(L - 1, 0);
    for (unsigned epoch = 1; epoch <= 3; ++epoch) {
      std::vector<Wg> wg(G);
      long guard = 0;
      bool all_done = false;
      while (!all_done && guard++ < 100000) {
        bool any = false;
        all_done = true;
        for (int i = 0; i < G; ++i) {
          int w = order == 0 ? i : order == 1 ? G - 1 - i : order == 2 ? i : (int)(lcg() >> 8) % G;
          any = run_wg(wg[w], w, G, bn, ns, cnt, epoch, order == 3) || any;
        }
        for (int i = 0; i < G && !any; ++i) any = run_wg(wg[i], i, G, bn, ns, cnt, epoch, true); // (a shuffled pass may have missed the one that can move)
        for (int i = 0; i < G; ++i) all_done = all_done && wg[i].done;
        if (!any && !all_done) {
          FAIL("DEADLOCK: G %d BN %d layers %d order %d epoch %u", G, bn, L, order, epoch);
          return;
        }
      }
      if (!all_done) FAIL("simulation did not end: G %d BN %d order %d", G, bn, order);
      for (int l = 0; l + 1 < L; ++l)
        if (cnt[l] != epoch * skc_arrivals(G)) FAIL("seam %d holds %u after launch %u of G %d", l, cnt[l], epoch, G);
    }
    ++g_sims;
  }
}

int main() {
  long owned_checked = 0, columns = 0, deals = 0;
  // c: the deal, for a spread of (br, k)
  for (int br : {1, 2, 3, 7, 16, 100})
    for (int k : {8, 32, 40, 72, 256, 264, 1000, 4096}) {
      const int S = br * skn_steps(k), W = skn_waves(S);
      if (skc_layer_waves(br, k) != W) FAIL("waves of br %d k %d", br, k);
      int next = 0;
      for (int w = 0; w < SKN_WMAX; ++w) {
        const int c = skc_wave_count(w, br, k), f = skc_wave_first(w, br, k);
        if (w < W) {
          if (c != skn_wave_count(w, W, S) || f != skn_wave_first(w, W, S) || f != next || c < 1) FAIL("deal br %d k %d wave %d: first %d count %d", br, k, w, f, c);
          next = f + c;
        } else if (c != 0) FAIL("wave %d beyond W = %d takes %d steps (br %d k %d)", w, W, c, br, k);
      }
      if (next != S) FAIL("deal br %d k %d covers %d of %d steps", br, k, next, S);
      ++deals;
    }
  const int blocks_of[] = {1, 2, 3, 4, 5, 7, 8, 9, 13, 16, 20};
  for (int bn : {16, 32, 64})
    for (int G = 1; G <= 9; ++G)
      for (int L = 2; L <= 4; ++L)
        for (int variant = 0; variant < 24; ++variant) {
          std::vector<int> ns;
          for (int l = 0; l < L; ++l) {
            const int b = blocks_of[(variant * 7 + l * 5 + G) % 11];
            const bool shifted = b > 1 && ((variant + l) & 1);
            ns.push_back(shifted ? (b - 1) * bn + 8 : b * bn);
          }
          for (int l = 0; l < L; ++l) {
            const int n = ns[l], blocks = skn_blocks(n, bn);
            // a: ownership
            std::vector<int> owner(blocks, -1);
            for (int w = 0; w < G; ++w) {
              const int owned = skc_owned(w, G, blocks);
              if (skc_arrive_after(w, G, blocks) != owned - 1) FAIL("arrival point of workgroup %d", w);
              for (int i = 0; i < owned; ++i) {
                const int b = skc_block(w, G, i);
                if (b < 0 || b >= blocks || owner[b] != -1) FAIL("block %d of layer %d (n %d BN %d G %d) owned twice or out of range", b, l, n, bn, G);
                else owner[b] = w;
                ++owned_checked;
              }
              if (w + owned * G < blocks) FAIL("workgroup %d of %d stops short of block %d", w, G, w + owned * G);
            }
            for (int b = 0; b < blocks; ++b)
              if (owner[b] != skc_owner(b, G)) FAIL("block %d of layer %d has owner %d, skc_owner says %d", b, l, owner[b], skc_owner(b, G));
            // d: columns
            std::vector<int> stored(n, 0);
            for (int b = 0; b < blocks; ++b) {
              const int n0 = skn_origin(b, n, bn);
              if (n0 < 0 || n0 + bn > n) FAIL("block %d of n %d BN %d reaches outside", b, n, bn);
              for (int c = skn_skip(b, n, bn); c < bn; ++c) {
                ++stored[n0 + c];
                if (!skn_owns(b, n, bn, n0 + c)) FAIL("block %d stores column %d it does not own", b, n0 + c);
              }
            }
            for (int c = 0; c < n; ++c) {
              if (stored[c] != 1) FAIL("column %d of layer %d (n %d BN %d) stored %d times", c, l, n, bn, stored[c]);
              ++columns;
            }
          }
          // b: arrivals per seam
          for (int l = 0; l + 1 < L; ++l) {
            unsigned arr = 0;
            for (int w = 0; w < G; ++w) arr += skc_signals(l, L) ? 1 : 0;
            if (arr != skc_arrivals(G)) FAIL("seam %d receives %u arrivals of G %d", l, arr, G);
          }
          if (skc_signals(L - 1, L)) FAIL("the last layer signals");
          simulate(G, bn, ns); // b and e
        }
  if (skc_key_tiles_m() != 1 || skc_key_tiles_n(7) != 7 || skc_target(5, 7) != 35) FAIL("the counter-block key or the target");
  if (skc_groups(20, 256) != 20 || skc_groups(300, 256) != 256) FAIL("skc_groups");
  printf("ownership %ld, columns %ld, deals %ld, simulations %ld\n", owned_checked, columns, deals, g_sims);
  if (g_fail) {
    printf("%d checks FAILED\n", g_fail);
    return 1;
  }
  printf("OK\n");
  return 0;
}
