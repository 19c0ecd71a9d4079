// driver.cpp - TEST INFRASTRUCTURE for tests/test_chain_skinny_split_cpu.py, never part of the product library. Linked with the real gemm_plan.cpp.
//   driver walk <bn> <m> <G> <P> <n,n,..> <k,k,..> <br,br,..>   walks the schedule of tpp-mlir_amd/csrc/brgemm_bf16_skinny_chain_split.h as the
//                 kernel does and prints: units owned once, units in all, arrivals per seam (min and max), waves, scratch floats, counters, bad
//   driver plan <mode> <split> <strict> <m> <image> <n,n,..> <k,k,..> <br,br,..>   plan_chain_skinny at 256 CUs, with and without the argument
#include "brgemm_bf16_skinny_chain_split.h"
#include "gemm_plan.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

using namespace tpp;

static std::vector<int> ints(const char *s) {
  std::vector<int> v;
  for (const char *p = s; *p; p = strchr(p, ',') ? strchr(p, ',') + 1 : p + strlen(p)) v.push_back(atoi(p));
  return v;
}

static int walk(int bn, int m, int G, int P, const std::vector<int> &n, const std::vector<int> &k, const std::vector<int> &br) {
  const int L = (int)n.size(), mb = skn_mb(m), regs = (mb / 16) * skn_cols(bn);
  long once = 0, all = 0, bad = 0;
  long long floats = 0, counters = 0; // what the launcher asks the scratch block for
  int waves = 1, arr_min = 1 << 30, arr_max = 0;
  for (int l = 0; l < L; ++l) {
    floats = std::max(floats, skcs_layer_floats(n[l], bn, mb, P, br[l], k[l]));
    counters = std::max(counters, skcs_layer_counters(n[l], bn, P, br[l], k[l]));
    waves = std::max(waves, skcs_layer_waves(P, br[l], k[l]));
  }
  for (int l = 0; l < L; ++l) {
    const int blocks = skn_blocks(n[l], bn), S = skcs_steps(br[l], k[l]), P_l = skcs_layer_parts(P, br[l], k[l]), units = skcs_units(n[l], bn, P, br[l], k[l]);
    bad += P_l != (P < S ? P : S) || units != blocks * P_l || (S == 1 && P_l != 1);
    std::vector<int> seen(units, 0), parts_of(blocks, 0);
    int arrivals = 0;
    for (int w = 0; w < G; ++w) { // the kernel's loop: sit out and arrive at once, or walk w, w + G, .. and arrive behind the last unit
      if (w >= units) {
        bad += skcs_owned(w, G, units) != 0;
        arrivals += skc_signals(l, L);
        continue;
      }
      int walked = 0;
      for (int u = w;; u += G) {
        const int prt = skcs_unit_part(u, blocks), blk = u - prt * blocks;
        bad += skcs_unit(w, G, walked) != u || blk != skcs_unit_block(u, blocks) || prt < 0 || prt >= P_l || blk < 0 || blk >= blocks;
        ++seen[u], ++walked, ++parts_of[blk];
        // the deal inside the unit: the part's waves cover its run once and in order, within the waves of the launch
        int next = sks_part_first(prt, P_l, S);
        for (int wv = 0; wv < SKN_WMAX; ++wv) {
          const int c = sks_wave_count(wv, prt, P_l, S), f = sks_wave_first(wv, prt, P_l, S);
          bad += (c > 0 && f != next) || (c > 0 && wv >= waves) || (wv < skn_waves(sks_part_count(prt, P_l, S))) != (c > 0);
          next += c;
        }
        bad += next != sks_part_first(prt, P_l, S) + sks_part_count(prt, P_l, S);
        if (P_l >= 2) // the highest float the unit parks, and its counter
          bad += sks_float_index(blk, prt, P_l, mb, bn, regs - 1, 63, 3) >= floats || blk >= counters;
        if (u + G >= units) {
          bad += skc_arrive_after(w, G, units) != walked - 1;
          arrivals += skc_signals(l, L);
          break;
        }
      }
      bad += walked != skcs_owned(w, G, units);
    }
    for (int v : seen) once += v == 1, ++all;
    for (int v : parts_of) bad += v != P_l;
    // the parts of a block: contiguous runs that cover the layer's steps once and in order
    int next = 0;
    for (int q = 0; q < P_l; ++q) {
      bad += sks_part_first(q, P_l, S) != next || sks_part_count(q, P_l, S) < 1;
      next += sks_part_count(q, P_l, S);
    }
    bad += next != S;
    if (skc_signals(l, L)) {
      bad += (unsigned)arrivals != skc_arrivals(G);
      arr_min = std::min(arr_min, arrivals), arr_max = std::max(arr_max, arrivals);
    }
  }
  printf("once %ld of %ld arrivals %d..%d waves %d floats %lld counters %lld bad %ld\n", once, all, arr_min, arr_max, waves, floats, counters, bad);
  return 0;
}

static void show(const ChainSkinnyPlan &p, int L, const std::vector<int> &k, const int64_t *br) {
  printf("bn %d groups %d gated %d parts %d why '%s' layer parts", p.bn, p.groups, (int)p.gated, p.parts, p.why);
  for (int l = 0; l < L; ++l) printf(" %d", p.parts ? skcs_layer_parts(p.parts, br[l], k[l]) : 1);
  printf("\n");
}

static int plan(int mode, int split, bool strict, int m, int image, const std::vector<int> &n, const std::vector<int> &k, const std::vector<int> &brs) {
  const int L = (int)n.size();
  int64_t n64[SKC_MAXL], k64[SKC_MAXL], br[SKC_MAXL];
  for (int l = 0; l < L; ++l) n64[l] = n[l], k64[l] = k[l], br[l] = brs[l];
  show(plan_chain_skinny(m, L, n64, k64, br, 256, image, mode, strict, split), L, k, br);
  if (split == 0) show(plan_chain_skinny(m, L, n64, k64, br, 256, image, mode, strict), L, k, br); // the call as every caller made it before
  return 0;
}

int main(int argc, char **argv) {
  const std::string a = argc >= 2 ? argv[1] : "";
  if (a == "walk" && argc == 9) return walk(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), ints(argv[6]), ints(argv[7]), ints(argv[8]));
  if (a == "plan" && argc == 10) return plan(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]) != 0, atoi(argv[5]), atoi(argv[6]), ints(argv[7]), ints(argv[8]), ints(argv[9]));
  return 2;
}
