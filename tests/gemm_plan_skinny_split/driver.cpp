// driver.cpp - TEST INFRASTRUCTURE for tests/test_gemm_plan_skinny_split.py, never part of the product library.
//
// Steps whole-layer calls through the kernel planner (tpp-mlir_amd/csrc/gemm_plan.h) under the modes 0, 1 and 32 of xsmm_hip_set_skinny_bf16
// and 0, 1, 3 and 16 of xsmm_hip_set_skinny_split at 64, 256 and 304 compute units, strict mode off and on, and prints one line per
// descriptor (the format of tests/gemm_plan_skinny/driver.cpp)
//   <form> <m>x<n>x<k> e<epilogue> f<forced> : <variant> <name>
// and under it one line per call
//   c br<batch> : <launch, both modes 0> | 0: <group> / <group> / <group> / <group> | 1: <group> / ... | 32: <group> / ...
// one block per skinny mode, in it one group per split mode 0, 1, 3, 16, in a group one cell per compute-unit count. The mode-0 launch
// comes from a GemmPlanEnv that names neither field. A cell of split mode 0 is that of the skinny driver: "-" (the launch of skinny mode 0,
// field by field) or S<MB>x<BN>. A cell of another split mode is "-" (the launch of split mode 0 under the same skinny mode, field by field)
// or P<split>: launcher skinny, the tile, the B image and every other field of the split-mode-0 launch, split > 1, and its text with
// "_split" behind "brgemm_bf16_skinny"; anything else prints with a "!". A line carries a "!" too when split mode 0 differs from an
// environment without the field, when strict mode changes any cell, when a forcing mode's cell depends on the compute units, or when
// another switch changes what this one does.
#include "gemm_plan.h"
#include <stdio.h>
#include <string.h>
#include <string>

using namespace tpp;

namespace {

const int CUS[3] = {64, 256, 304};

struct Form {
  const char *name;
  int64_t dtype;
  int vnni_b, vf, vnni_c;
};
const Form V2{"v2", DT_BF16, 1, 2, 0}, V4{"v4", DT_BF16, 1, 4, 0}, FLAT{"flat", DT_BF16, 0, 0, 0}, F32{"f32", DT_F32, 0, 0, 0};

GemmDesc desc(const Form &f, int64_t m, int64_t n, int64_t k, const char *ep = "bBr", int forced = -1) {
  GemmDesc d;
  memset(&d, 0, sizeof(d));
  d.kind = KIND_GEMM;
  d.has_batch = 1;
  d.dtype = f.dtype;
  d.m = m, d.n = n, d.k = k;
  d.lda = 16 * k;
  d.ldb = n;
  d.ldc = n;
  d.stride_a = k;
  d.stride_b = k * d.ldb;
  d.beta0 = strchr(ep, 'b') != nullptr;
  d.bias = strchr(ep, 'B') != nullptr;
  d.relu = strchr(ep, 'r') != nullptr;
  d.fused = d.bias || d.relu;
  d.vnni_b = f.vnni_b;
  d.vnni_factor = f.vf;
  d.vnni_c = f.vnni_c;
  const bool ok = plan_gemm(d, forced, GemmPlanEnv{256, false, -1});
  printf("%s %ldx%ldx%ld e%s f%d : %s%d %s\n", f.name, (long)m, (long)n, (long)k, *ep ? ep : "-", forced, ok ? "" : "!", d.variant, d.name);
  return d;
}

std::string launch_text(const GemmLaunch &l) {
  char buf[256];
  snprintf(buf, sizeof buf, "L%d t%d s%d b%d g%d%s%s%s%s%s", (int)l.launcher, l.tile, l.split, l.b_kind, (int)l.generic, l.edge ? " edge" : "", l.edge_k ? " edge_k" : "",
           l.edge_k8 ? " edge_k8" : "", l.halves ? " halves" : "", l.tail_tiles ? " tail" : "");
  std::string s = buf;
  if (l.text && *l.text) s += std::string(" \"") + l.text + "\"";
  return s;
}

// split mode 0: "-", S<MB>x<BN>, or the launch with a "!" (tests/gemm_plan_skinny/driver.cpp cell)
std::string skinny_cell(const GemmDesc &d, const GemmLaunch &l, const std::string &off) {
  if (l.launcher != GL_BF16_SKINNY) return launch_text(l) == off ? "-" : "!" + launch_text(l);
  const int kind = !d.vnni_b ? 2 : d.vnni_factor == 4 ? 4 : 0, mb = d.m <= 16 ? 16 : 32;
  char want[96], out[32];
  snprintf(want, sizeof want, "brgemm_bf16_skinny%s<%dx%d>", kind == 2 ? "_flatb" : kind == 4 ? "_vnni4" : "", mb, l.tile);
  snprintf(out, sizeof out, "S%dx%d", mb, l.tile);
  const bool ok = l.b_kind == kind && l.split == 1 && !l.edge && !l.edge_k && !l.edge_k8 && !l.halves && !l.tail_tiles && l.text && !strcmp(l.text, want);
  return ok ? out : "!" + launch_text(l);
}

// another split mode against the launch `base` of split mode 0 under the same skinny mode: "-", P<split>, or the launch with a "!"
std::string split_cell(const GemmLaunch &l, const GemmLaunch &base) {
  if (launch_text(l) == launch_text(base)) return "-";
  bool ok = base.launcher == GL_BF16_SKINNY && l.split > 1 && l.text && base.text;
  if (ok) {
    std::string want = base.text;
    want.insert(strlen("brgemm_bf16_skinny"), "_split");
    GemmLaunch same = l;
    same.split = base.split, same.text = base.text;
    ok = want == l.text && launch_text(same) == launch_text(base);
  }
  return ok ? "P" + std::to_string(l.split) : "!" + launch_text(l);
}

void call(const GemmDesc &d, int64_t br) {
  static const int skinny[3] = {0, 1, 32}, split[4] = {0, 1, 3, 16};
  const GemmAlign al{true, true, true, true, true};
  std::string flags, offs[3][2]; // both modes 0 per compute-unit count and strict mode: from an environment that names neither field
  for (int strict = 0; strict < 2; ++strict)
    for (int cu = 0; cu < 3; ++cu) offs[cu][strict] = launch_text(plan_gemm_call(d, br, al, GemmPlanEnv{CUS[cu], strict != 0, -1}));
  printf(" c br%ld : %s", (long)br, offs[1][0].c_str());
  for (int sm : skinny) {
    printf(" | %d:", sm);
    GemmLaunch base[3][2];
    for (int pi = 0; pi < 4; ++pi) {
      std::string cells[3];
      for (int cu = 0; cu < 3; ++cu) {
        for (int strict = 0; strict < 2; ++strict) {
          GemmPlanEnv e{CUS[cu], strict != 0, -1};
          e.skinny_bf16 = sm;
          if (split[pi] == 0) { // an environment that does not name the new field, and one that sets it to 0
            base[cu][strict] = plan_gemm_call(d, br, al, e);
            e.skinny_split = 0;
            if (launch_text(plan_gemm_call(d, br, al, e)) != launch_text(base[cu][strict])) flags += " !split mode 0 differs from an environment without the field";
          }
          e.skinny_split = split[pi];
          const GemmLaunch l = plan_gemm_call(d, br, al, e);
          const std::string c = split[pi] == 0 ? skinny_cell(d, l, offs[cu][strict]) : split_cell(l, base[cu][strict]);
          if (strict == 0) cells[cu] = c;
          else if (c != cells[cu]) flags += " !strict mode changes the answer";
          if (strict) continue;
          // every other switch, one at a time and all together, and a forced split
          for (int which = 0; which < 8; ++which) {
            GemmPlanEnv o = e;
            if (which == 0 || which == 7) o.edge_tiles = 2;
            if (which == 1) o.edge_tiles = V_BF16_LW_32x64;
            if (which == 2 || which == 7) o.edge_k_bf16 = 1, o.edge_k8_bf16 = 1;
            if (which == 3 || which == 7) o.dma256_images = 2, o.dma256_edge = 2;
            if (which == 4 || which == 7) o.tail_split = 1, o.halves = 2, o.edge_k = 1;
            if (which == 5) o.forced_split = 4;
            if (which == 6) o.edge_k_bf16 = V_BF16_LW_32x64, o.edge_k8_bf16 = V_BF16_LW_32x64;
            const GemmLaunch lo = plan_gemm_call(d, br, al, o);
            if (l.launcher == GL_BF16_SKINNY ? launch_text(lo) != launch_text(l) : lo.launcher == GL_BF16_SKINNY) flags += " !another switch changes this one";
          }
        }
      }
      if (split[pi] > 1 && (cells[0] != cells[1] || cells[1] != cells[2])) flags += " !a forcing split mode depends on the compute units";
      if (sm == 0 && split[pi] != 0 && (cells[0] != "-" || cells[1] != "-" || cells[2] != "-")) flags += " !the split mode changes a call with the skinny switch off";
      printf("%s %s %s %s", pi ? " /" : "", cells[0].c_str(), cells[1].c_str(), cells[2].c_str());
    }
  }
  printf("%s\n", flags.c_str());
}

} // namespace

int main() {
  static const int64_t ms[] = {1, 16, 17, 31, 32}, ns[] = {16, 200, 1024, 4096}, kbr[][2] = {{32, 1}, {64, 16}, {64, 64}, {1000, 1}};
  const Form *forms[3] = {&V2, &V4, &FLAT};
  for (const Form *f : forms)
    for (int64_t m : ms)
      for (int64_t n : ns)
        for (auto &kb : kbr) call(desc(*f, m, n, kb[0]), kb[1]);
  // never taken: f32, a forced generic kernel, beta 1 (taken)
  call(desc(F32, 8, 1024, 64), 16);
  call(desc(V2, 8, 1024, 64, "bBr", V_GENERIC), 16);
  call(desc(V2, 8, 1024, 64, ""), 16);
  return 0;
}
