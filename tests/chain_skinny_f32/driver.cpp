// driver.cpp - TEST INFRASTRUCTURE for tests/test_chain_skinny_f32_cpu.py, never part of the product library. Linked with the real gemm_plan.cpp.
//   driver walk <bn> <G> <n,n,..> <k,k,..> <br,br,..>   walks the schedule of tpp-mlir_amd/csrc/brgemm_f32_skinny_chain.h as the kernel does
//                 and prints: blocks owned once, blocks in all, arrivals per seam (min and max over the workgroups' sum), waves of the launch, bad
//   driver plan   a written list of chains through plan_chain at 256 CUs: form / tile / groups / tiles_m / tiles_n, or form 0 and the refusal
#include "brgemm_f32_skinny_chain.h"
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

static int walk(int bn, int G, const std::vector<int> &n, const std::vector<int> &k, const std::vector<int> &br) {
  const int L = (int)n.size();
  long once = 0, all = 0, bad = 0;
  int waves = 1, arr_min = 1 << 30, arr_max = 0;
  for (int l = 0; l < L; ++l) {
    const int blocks = skf_blocks(n[l], bn), S = br[l] * skf_steps(k[l]), W = skfc_layer_waves(br[l], k[l]);
    std::vector<int> seen(blocks, 0);
    int arrivals = 0;
    for (int w = 0; w < G; ++w) { // the kernel's loop: sit out and arrive at once, or walk w, w + G, .. and arrive behind the last block
      if (w >= blocks) {
        bad += skc_owned(w, G, blocks) != 0 || skc_waits(w, G, l, blocks);
        arrivals += skc_signals(l, L);
        continue;
      }
      int walked = 0;
      for (int blk = w;; blk += G) {
        bad += skc_block(w, G, walked) != blk || skc_owner(blk, G) != w;
        ++seen[blk], ++walked;
        if (blk + G >= blocks) {
          bad += skc_arrive_after(w, G, blocks) != walked - 1;
          arrivals += skc_signals(l, L);
          break;
        }
      }
      bad += walked != skc_owned(w, G, blocks) || skc_waits(w, G, l, blocks) != (l > 0);
    }
    for (int v : seen) once += v == 1, ++all;
    if (skc_signals(l, L)) {
      bad += (unsigned)arrivals != skc_arrivals(G) || skc_target(3, G) != 3u * G;
      arr_min = arrivals < arr_min ? arrivals : arr_min, arr_max = arrivals > arr_max ? arrivals : arr_max;
    }
    // the waves and their runs: the single call's deal over W waves, nothing for a wave at or beyond W
    bad += W != skf_waves(S);
    int next = 0;
    for (int w = 0; w < SKF_WMAX; ++w) {
      const int c = skfc_wave_count(w, br[l], k[l]), f = skfc_wave_first(w, br[l], k[l]);
      bad += w < W ? (c != skf_wave_count(w, W, S) || f != skf_wave_first(w, W, S) || f != next || c < 1) : (c != 0 || f != 0);
      next += c;
    }
    bad += next != S;
    waves = W > waves ? W : waves;
  }
  printf("once %ld of %ld arrivals %d..%d waves %d bad %ld\n", once, all, arr_min, arr_max, waves, bad);
  return 0;
}

struct Row {
  const char *what;
  int mode, dtype, m;
  std::vector<int> n, k;
  bool strict, beta0;
};

static int plan() {
  const std::vector<int> N{72, 64}, K{64, 72};
  const Row rows[] = {{"forced 16", 16, DT_F32, 16, N, K, false, true}, {"forced 32", 32, DT_F32, 16, N, K, false, true}, {"forced 64", 64, DT_F32, 16, N, K, false, true},
                      {"forced G 2 BN 32", 2032, DT_F32, 31, N, K, false, true}, {"three layers 16", 16, DT_F32, 1, {144, 96, 64}, {40, 144, 96}, false, true},
                      {"strict", 32, DT_F32, 16, N, K, true, true}, {"n % 4 != 0", 32, DT_F32, 16, {70, 64}, {64, 68}, false, true},
                      {"k % 4 != 0", 32, DT_F32, 16, N, {66, 72}, false, true}, {"n_l < BN", 64, DT_F32, 16, {72, 32, 64}, {64, 72, 32}, false, true},
                      {"m = 32", 32, DT_F32, 32, N, K, false, true}, {"bf16", 32, DT_BF16, 16, N, K, false, true}, {"beta 1", 32, DT_F32, 16, N, K, false, false},
                      {"forced G above the CUs", 300032, DT_F32, 16, N, K, false, true}, {"mode 1, funnel m 16", 1, DT_F32, 16, {512, 256, 128}, {784, 512, 256}, false, true},
                      {"mode 1, funnel m 17", 1, DT_F32, 17, {512, 256, 128}, {784, 512, 256}, false, true}, {"mode 1, 1024 m 1", 1, DT_F32, 1, {1024, 1024}, {1024, 1024}, false, true},
                      {"mode 1, 1024 m 2", 1, DT_F32, 2, {1024, 1024}, {1024, 1024}, false, true}, {"mode 1, 1028 m 1", 1, DT_F32, 1, {1024, 1024}, {1028, 1024}, false, true},
                      {"switch 0, m 16", 0, DT_F32, 16, N, K, false, true}, {"switch 0, m 512", 0, DT_F32, 512, {1024, 1024}, {1024, 1024}, false, true},
                      {"forced 32, m 512", 32, DT_F32, 512, {1024, 1024}, {1024, 1024}, false, true}};
  for (const Row &r : rows) {
    const int L = (int)r.n.size();
    std::vector<GemmDesc> d(L);
    const GemmDesc *dp[CHAIN_PLAN_MAXL];
    int64_t br[CHAIN_PLAN_MAXL];
    for (int l = 0; l < L; ++l) {
      GemmDesc &g = d[l];
      memset(&g, 0, sizeof(g));
      g.kind = KIND_GEMM, g.has_batch = 1, g.dtype = r.dtype, g.m = r.m, g.n = r.n[l], g.k = r.k[l];
      g.lda = l == 0 ? r.k[0] : r.n[l - 1], g.ldb = g.ldc = r.n[l], g.stride_a = r.k[l], g.stride_b = (int64_t)r.k[l] * r.n[l];
      g.beta0 = r.beta0 || l == 0, g.bias = g.relu = g.fused = 1, g.vnni_b = r.dtype == DT_BF16, g.vnni_factor = 2;
      plan_gemm(g, -1, GemmPlanEnv{256, r.strict, -1});
      dp[l] = &g, br[l] = 1;
    }
    ChainPlanEnv env{};
    env.strict = r.strict, env.skinny_f32 = r.mode;
    ChainCus cus{[](void *) { return (int64_t)256; }, nullptr};
    const ChainLaunchPlan p = plan_chain(L, dp, br, env, cus);
    if (p.form == CF_CALLS) printf("%s : calls : %s\n", r.what, p.why);
    else printf("%s : form %d tile %d groups %d key %d %d pad %d\n", r.what, (int)p.form, p.tile, p.groups, p.tiles_m, p.tiles_n, (int)p.mixed);
  }
  // skfc_ld_ok: the multiple of 4, the cover, the sign, and the bound 2^24 on lda and ldc (not on ldb)
  printf("ld_ok %d %d %d %d %d %d %d\n", skfc_ld_ok(72, 72, 72, 64, 64 * 72, 72, 64), skfc_ld_ok(72, 74, 72, 64, 0, 72, 64), skfc_ld_ok(60, 72, 72, 64, 0, 72, 64),
         skfc_ld_ok(72, 72, 72, -4, 0, 72, 64), skfc_ld_ok((1 << 24) - 4, 1 << 25, (1 << 24) - 4, 0, 0, 72, 64), skfc_ld_ok(1 << 24, 72, 72, 0, 0, 72, 64),
         skfc_ld_ok(72, 72, 1 << 24, 0, 0, 72, 64));
  return 0;
}

int main(int argc, char **argv) {
  const std::string a = argc >= 2 ? argv[1] : "";
  if (a == "walk" && argc == 7) return walk(atoi(argv[2]), atoi(argv[3]), ints(argv[4]), ints(argv[5]), ints(argv[6]));
  return a == "plan" ? plan() : 2;
}
