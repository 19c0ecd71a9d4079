// driver.cpp - TEST INFRASTRUCTURE for tests/test_skinny_f32_split_cpu.py, never part of the product library. Linked with the real gemm_plan.cpp.
//   driver maps   walks the maps of tpp-mlir_amd/csrc/brgemm_f32_skinny_split.h by brute force and prints counts
//   driver plan   a written list of calls through plan_gemm_call at 256 CUs: per call the cell of (skinny_f32, skinny_f32_split) =
//                 (16, 0) (16, 4) (32, 16) (0, 3) (1, 1) (1, 0) - "-" = the launch with both switches off, else kernel text / BN / P_eff
#include "brgemm_f32_skinny_split.h"
#include "gemm_plan.h"
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

using namespace tpp;

static int maps() {
  for (int S : {1, 2, 3, 9, 32, 63})
    for (int P : {2, 3, 4, 16}) {
      const int pe = skfs_parts(P, S), bw = skfs_block_waves(pe, S);
      std::vector<int> seen(S, 0);
      int bad = bw != skf_waves(skfs_part_count(0, pe, S)), next = 0, once = 0;
      for (int p = 0; p < pe; ++p) {
        bad += skfs_part_first(p, pe, S) != next || skfs_part_count(p, pe, S) < 1 || skfs_part_waves(p, pe, S) > bw || skfs_part_waves(p, pe, S) < bw - 1;
        for (int w = 0; w < bw; ++w) { // every wave of the workgroup, the idle one included: its run is empty and starts inside the call
          const int f = skfs_wave_first(w, p, pe, S), c = skfs_wave_count(w, p, pe, S);
          bad += f < 0 || f + c > S || (c > 0 && f != next) || (c == 0) != (w >= skfs_part_waves(p, pe, S));
          for (int t = f; t < f + c; ++t) ++seen[t];
          next += c;
        }
      }
      for (int v : seen) once += v == 1;
      printf("deal steps %d P %d parts %d once %d bad %d\n", S, P, pe, once, bad);
    }
  // the scratch: every (block, part, register, lane, element) at its own float, all below skfs_floats; the grid is part-major
  for (int bn : {16, 64})
    for (int mb : {16, 32}) {
      const int blocks = 3, pe = 5, regs = (mb / 16) * (bn / 16);
      std::vector<int> seen(skfs_floats(blocks, pe, mb, bn), 0);
      long bad = 0, once = 0;
      for (int b = 0; b < blocks; ++b)
        for (int p = 0; p < pe; ++p) {
          const int bid = p * blocks + b;
          bad += skfs_grid_part(bid, blocks) != p || skfs_grid_block(bid, blocks) != b || bid >= skfs_grid(blocks, pe);
          for (int r = 0; r < regs; ++r)
            for (int l = 0; l < 64; ++l)
              for (int e = 0; e < 4; ++e) {
                const long long i = skfs_float_index(b, p, pe, mb, bn, r, l, e);
                if (i < 0 || i >= (long long)seen.size()) ++bad;
                else ++seen[i];
              }
        }
      for (int v : seen) once += v == 1;
      printf("scratch bn %d mb %d floats %ld once %ld bad %ld\n", bn, mb, (long)seen.size(), once, bad);
    }
  // the three limits: 4096 counters, 16 parts, 8 Mi floats (64 x 32 slots of 2048 floats: 4096 slots fit, 4097 do not)
  printf("fits %d %d %d %d %d %d %d\n", skfs_launch_fits(4096, 2, 16, 16, 4096, 16, 8 << 20), skfs_launch_fits(4097, 2, 16, 16, 4096, 16, 8 << 20),
         skfs_launch_fits(8, 16, 16, 16, 4096, 16, 8 << 20), skfs_launch_fits(8, 17, 16, 16, 4096, 16, 8 << 20), skfs_launch_fits(256, 16, 32, 64, 4096, 16, 8 << 20),
         skfs_launch_fits(257, 16, 32, 64, 4096, 16, 8 << 20), skfs_launch_fits(8, 1, 16, 16, 4096, 16, 8 << 20));
  return 0;
}

static std::string cell(const GemmDesc &d, int64_t br, int skinny, int split) {
  GemmPlanEnv e{256, false, -1}, off{256, false, -1};
  e.skinny_f32 = skinny, e.skinny_f32_split = split;
  const GemmLaunch l = plan_gemm_call(d, br, GemmAlign{true, true, true, true, true}, e), o = plan_gemm_call(d, br, GemmAlign{true, true, true, true, true}, off);
  if (l.launcher != GL_F32_SKINNY) return l.launcher == o.launcher && l.tile == o.tile && l.split == o.split && !strcmp(l.text, o.text) ? "-" : "?";
  return std::string(l.text) + "/" + std::to_string(l.tile) + "/" + std::to_string(l.split);
}

static int plan() {
  const auto row = [](const char *what, int64_t m, int64_t n, int64_t k, int64_t br) {
    GemmDesc d;
    memset(&d, 0, sizeof(d));
    d.kind = KIND_GEMM, d.has_batch = 1, d.dtype = DT_F32, d.m = m, d.n = n, d.k = k, d.lda = k * br, d.ldb = n, d.ldc = n, d.stride_a = k, d.stride_b = k * n;
    d.beta0 = d.bias = d.relu = d.fused = 1;
    plan_gemm(d, -1, GemmPlanEnv{256, false, -1});
    printf("plan %s :", what);
    for (auto ms : {std::pair<int, int>{16, 0}, {16, 4}, {32, 16}, {0, 3}, {1, 1}, {1, 0}}) printf(" %s", cell(d, br, ms.first, ms.second).c_str());
    printf("\n");
  };
  for (int m : {1, 16, 31}) {
    row(("m" + std::to_string(m) + " n1024 K1024").c_str(), m, 1024, 64, 16);
    row(("m" + std::to_string(m) + " n1024 K4096").c_str(), m, 1024, 64, 64);
    row(("m" + std::to_string(m) + " n4096 K4096").c_str(), m, 4096, 64, 64);
  }
  row("m8 n64 k36 br1", 8, 64, 36, 1);
  row("m8 n64 k16 br1", 8, 64, 16, 1);
  row("m32", 32, 1024, 64, 16);
  return 0;
}

int main(int argc, char **argv) {
  const std::string a = argc == 2 ? argv[1] : "";
  return a == "maps" ? maps() : a == "plan" ? plan() : 2;
}
