// driver.cpp - TEST INFRASTRUCTURE for tests/test_chain_skinny_f32_split_cpu.py, never part of the product library. Linked with the real gemm_plan.cpp.
//   driver walk <bn> <m> <G> <P> <n,n,..> <k,k,..> <br,br,..>   walks the schedule of tpp-mlir_amd/csrc/brgemm_f32_skinny_chain_split.h as the
//                 kernel does and prints: units owned once, units in all, arrivals per seam (min and max), waves, scratch floats, counters, bad
//   driver plan <mode> <split> <strict> <m> <n,n,..> <k,k,..> <br,br,..>   the chain through plan_chain at 256 CUs
#include "brgemm_f32_skinny_chain_split.h"
#include "gemm_plan.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

using namespace tpp;

static std::vector<int> ints(const char *s) {
  std::vector<int> v;
  for (const char *p = s; *p; p = strchr(p, ',') ? strchr(p, ',') + 1 : p + strlen(p)) v.push_back(atoi(p));
  return v;
}

static int walk(int bn, int m, int G, int P, const std::vector<int> &n, const std::vector<int> &k, const std::vector<int> &br) {
  const int L = (int)n.size(), mb = skf_mb(m), regs = (mb / 16) * skf_cols(bn);
  long once = 0, all = 0, bad = 0;
  long long floats = 0, counters = 0; // what the launcher asks the scratch block for
  int waves = 1, arr_min = 1 << 30, arr_max = 0;
  for (int l = 0; l < L; ++l) {
    floats = std::max(floats, skfcs_layer_floats(n[l], bn, mb, P, br[l], k[l]));
    counters = std::max(counters, skfcs_layer_counters(n[l], bn, P, br[l], k[l]));
    waves = std::max(waves, skfcs_layer_waves(P, br[l], k[l]));
  }
  for (int l = 0; l < L; ++l) {
    const int blocks = skf_blocks(n[l], bn), S = skfcs_steps(br[l], k[l]), P_l = skfcs_layer_parts(P, br[l], k[l]), units = skfcs_units(n[l], bn, P, br[l], k[l]);
    bad += P_l != (P < S ? P : S) || units != blocks * P_l;
    std::vector<int> seen(units, 0), parts_of(blocks, 0);
    int arrivals = 0;
    for (int w = 0; w < G; ++w) { // the kernel's loop: sit out and arrive at once, or walk w, w + G, .. and arrive behind the last unit
      if (w >= units) {
        bad += skfcs_owned(w, G, units) != 0;
        arrivals += skc_signals(l, L);
        continue;
      }
      int walked = 0;
      for (int u = w;; u += G) {
        const int prt = skfcs_unit_part(u, blocks), blk = u - prt * blocks;
        bad += skfcs_unit(w, G, walked) != u || blk != skfcs_unit_block(u, blocks) || prt < 0 || prt >= P_l || blk < 0 || blk >= blocks;
        ++seen[u], ++walked, ++parts_of[blk];
        // the deal inside the unit: the part's waves cover its run once and in order, within the waves of the launch
        int next = skfs_part_first(prt, P_l, S);
        for (int wv = 0; wv < SKF_WMAX; ++wv) {
          const int c = skfs_wave_count(wv, prt, P_l, S), f = skfs_wave_first(wv, prt, P_l, S);
          bad += (c > 0 && f != next) || (c > 0 && wv >= waves) || (wv < skfs_part_waves(prt, P_l, S)) != (c > 0);
          next += c;
        }
        bad += next != skfs_part_first(prt, P_l, S) + skfs_part_count(prt, P_l, S);
        if (P_l >= 2) // the highest float the unit parks, and its counter
          bad += skfs_float_index(blk, prt, P_l, mb, bn, regs - 1, 63, 3) >= floats || blk >= counters;
        if (u + G >= units) {
          bad += skc_arrive_after(w, G, units) != walked - 1;
          arrivals += skc_signals(l, L);
          break;
        }
      }
      bad += walked != skfcs_owned(w, G, units);
    }
    for (int v : seen) once += v == 1, ++all;
    for (int v : parts_of) bad += v != P_l;
    // the parts of a block: contiguous runs that cover the layer's steps once and in order
    int next = 0;
    for (int q = 0; q < P_l; ++q) {
      bad += skfs_part_first(q, P_l, S) != next || skfs_part_count(q, P_l, S) < 1;
      next += skfs_part_count(q, P_l, S);
    }
    bad += next != S;
    if (skc_signals(l, L)) {
      bad += (unsigned)arrivals != skc_arrivals(G);
      arr_min = arrivals < arr_min ? arrivals : arr_min, arr_max = arrivals > arr_max ? arrivals : arr_max;
    }
  }
  printf("once %ld of %ld arrivals %d..%d waves %d floats %lld counters %lld bad %ld\n", once, all, arr_min, arr_max, waves, floats, counters, bad);
  return 0;
}

static int plan(int mode, int split, bool strict, int m, const std::vector<int> &n, const std::vector<int> &k, const std::vector<int> &brs) {
  const int L = (int)n.size();
  std::vector<GemmDesc> d(L);
  const GemmDesc *dp[CHAIN_PLAN_MAXL];
  int64_t br[CHAIN_PLAN_MAXL];
  for (int l = 0; l < L; ++l) {
    GemmDesc &g = d[l];
    memset(&g, 0, sizeof(g));
    g.kind = KIND_GEMM, g.has_batch = 1, g.dtype = DT_F32, g.m = m, g.n = n[l], g.k = k[l];
    g.lda = l == 0 ? k[0] * brs[0] : n[l - 1], g.ldb = g.ldc = n[l], g.stride_a = k[l], g.stride_b = (int64_t)k[l] * n[l];
    g.beta0 = g.bias = g.relu = g.fused = 1, g.vnni_factor = 2;
    plan_gemm(g, -1, GemmPlanEnv{256, strict, -1});
    dp[l] = &g, br[l] = brs[l];
  }
  ChainPlanEnv env{};
  env.strict = strict, env.skinny_f32 = mode, env.skinny_f32_split = split;
  ChainCus cus{[](void *) { return (int64_t)256; }, nullptr};
  const ChainLaunchPlan p = plan_chain(L, dp, br, env, cus);
  if (p.form == CF_CALLS) return printf("calls : %s\n", p.why), 0;
  printf("form %d tile %d groups %d key %d %d pad %d parts %d layer parts", (int)p.form, p.tile, p.groups, p.tiles_m, p.tiles_n, (int)p.mixed, p.parts);
  for (int l = 0; l < L; ++l) printf(" %d", p.parts ? skfcs_layer_parts(p.parts, br[l], k[l]) : 1);
  printf("\n");
  return 0;
}

int main(int argc, char **argv) {
  const std::string a = argc >= 2 ? argv[1] : "";
  if (a == "walk" && argc == 9) return walk(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), ints(argv[6]), ints(argv[7]), ints(argv[8]));
  if (a == "plan" && argc == 9) return plan(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]) != 0, atoi(argv[5]), ints(argv[6]), ints(argv[7]), ints(argv[8]));
  return 2;
}
