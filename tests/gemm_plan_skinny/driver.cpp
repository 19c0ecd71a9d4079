// driver.cpp - TEST INFRASTRUCTURE for tests/test_gemm_plan_skinny.py, never part of the product library.
//
// Steps whole-layer calls through the kernel planner (tpp-mlir_amd/csrc/gemm_plan.h) under the modes of xsmm_hip_set_skinny_bf16 (0, 1, 16,
// 32, 64) at 64, 256 and 304 compute units, strict mode off and on, and prints one line per descriptor
//   <form> <m>x<n>x<k> [ld<lda>,<ldb>,<ldc>] e<epilogue> f<forced> : <variant> <name> [gf] [vf]
// and under it one line per call
//   c br<batch> [a<A,B>/<C>/<D alignment>] : <launch, mode 0> | 1: <cell at 64 CUs> <at 256> <at 304> | 16: <cell> | 32: <cell> | 64: <cell>
// where the mode-0 launch comes from a GemmPlanEnv that never names the new field, and a cell is "-" (the mode-0 launch, field by field)
// or S<MB>x<BN> (launcher skinny, tile = BN, the B image of the descriptor, the text brgemm_bf16_skinny[_flatb|_vnni4]<MBxBN>; anything else
// prints with a "!"). A line carries a "!" too when mode 0 differs from an environment without the field, when strict mode changes any
// cell, when a forcing mode's cell depends on the compute units, or when another switch changes what this one does. ("-" is relative to
// mode 0 at the same compute units and strict mode; the printed mode-0 launch is the one at 256 compute units, strict off.)
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
const Form V2{"v2", DT_BF16, 1, 2, 0}, V4{"v4", DT_BF16, 1, 4, 0}, FLAT{"flat", DT_BF16, 0, 0, 0}, VC{"vc", DT_BF16, 1, 2, 1}, F32{"f32", DT_F32, 0, 0, 0};

GemmDesc desc(const Form &f, int64_t m, int64_t n, int64_t k, const char *ep = "bBr", int forced = -1, int64_t lda = -1, int64_t ldb = -1, int64_t ldc = -1) {
  GemmDesc d;
  memset(&d, 0, sizeof(d));
  d.kind = KIND_GEMM;
  d.has_batch = 1;
  d.dtype = f.dtype;
  d.m = m, d.n = n, d.k = k;
  d.lda = lda >= 0 ? lda : 16 * k; // room for sixteen batch elements side by side in a row of A
  d.ldb = ldb >= 0 ? ldb : n;
  d.ldc = ldc >= 0 ? ldc : n;
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
  printf("%s %ldx%ldx%ld", f.name, (long)m, (long)n, (long)k);
  if (lda >= 0 || ldb >= 0 || ldc >= 0) printf(" ld%ld,%ld,%ld", (long)d.lda, (long)d.ldb, (long)d.ldc);
  printf(" e%s f%d : %s%d %s", *ep ? ep : "-", forced, ok ? "" : "!", d.variant, d.name);
  if (d.generic_forced) printf(" gf");
  if (d.variant_forced) printf(" vf");
  printf("\n");
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

bool taken(const GemmLaunch &l) { return l.launcher == GL_BF16_SKINNY; }

// "-", S<MB>x<BN>, or the launch with a "!"
std::string cell(const GemmDesc &d, const GemmLaunch &l, const std::string &off) {
  if (!taken(l)) return launch_text(l) == off ? "-" : "!" + launch_text(l);
  const int kind = !d.vnni_b ? 2 : d.vnni_factor == 4 ? 4 : 0, mb = d.m <= 16 ? 16 : 32;
  char want[96], out[32];
  snprintf(want, sizeof want, "brgemm_bf16_skinny%s<%dx%d>", kind == 2 ? "_flatb" : kind == 4 ? "_vnni4" : "", mb, l.tile);
  snprintf(out, sizeof out, "S%dx%d", mb, l.tile);
  const bool ok = l.b_kind == kind && l.split == 1 && !l.edge && !l.edge_k && !l.edge_k8 && !l.halves && !l.tail_tiles && l.text && !strcmp(l.text, want);
  return ok ? out : "!" + launch_text(l);
}

// alignments in bytes: A and B, C, D
void call(const GemmDesc &d, int64_t br, int ab = 16, int c = 16, int dd = 16) {
  static const int modes[4] = {1, 16, 32, 64};
  const GemmAlign al{ab >= 16, c >= 16, c >= 8, dd >= 8, dd >= 16};
  printf(" c br%ld", (long)br);
  if (ab != 16 || c != 16 || dd != 16) printf(" a%d/%d/%d", ab, c, dd);
  const std::string off = launch_text(plan_gemm_call(d, br, al, GemmPlanEnv{256, false, -1}));
  printf(" : %s", off.c_str());
  std::string flags, offs[3][2]; // mode 0 per compute-unit count and strict mode: from an environment that never names the field
  for (int strict = 0; strict < 2; ++strict)
    for (int cu = 0; cu < 3; ++cu) {
      GemmPlanEnv e{CUS[cu], strict != 0, -1};
      offs[cu][strict] = launch_text(plan_gemm_call(d, br, al, e));
      e.skinny_bf16 = 0;
      if (launch_text(plan_gemm_call(d, br, al, e)) != offs[cu][strict]) flags += " !mode 0 differs from an environment without the field";
    }
  for (int mi = 0; mi < 4; ++mi) {
    std::string cells[3];
    for (int cu = 0; cu < 3; ++cu) {
      GemmPlanEnv e{CUS[cu], false, -1};
      e.skinny_bf16 = modes[mi];
      const GemmLaunch l = plan_gemm_call(d, br, al, e);
      cells[cu] = cell(d, l, offs[cu][0]);
      GemmPlanEnv s = e;
      s.strict = true;
      if (cell(d, plan_gemm_call(d, br, al, s), offs[cu][1]) != cells[cu]) flags += " !strict mode changes the answer";
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
        if (taken(lo) != taken(l) || (taken(l) && launch_text(lo) != launch_text(l))) flags += " !another switch changes this one";
      }
    }
    if (modes[mi] == 1) printf(" | 1: %s %s %s", cells[0].c_str(), cells[1].c_str(), cells[2].c_str());
    else {
      if (cells[0] != cells[1] || cells[1] != cells[2]) flags += " !a forcing mode depends on the compute units";
      printf(" | %d: %s", modes[mi], cells[1].c_str());
    }
  }
  printf("%s\n", flags.c_str());
}

void calls(const GemmDesc &d) {
  call(d, 1);
  call(d, 16);
}

} // namespace

int main() {
  static const int64_t ms[] = {1, 8, 16, 17, 31, 32, 33}, ns[] = {8, 16, 24, 64, 72, 1000, 1024, 4096}, ks[] = {8, 32, 40, 64, 1000, 1024};
  const Form *forms[3] = {&V2, &V4, &FLAT};
  for (const Form *f : forms)
    for (int64_t m : ms)
      for (int64_t n : ns)
        for (int64_t k : ks) calls(desc(*f, m, n, k));
  // never taken: f32, a VNNI C, forced kernels (the generic one, a variant), an empty batch
  for (int64_t m : {8, 31}) {
    calls(desc(F32, m, 1024, 64));
    calls(desc(VC, m == 31 ? 30 : m, 1024, 64));
    for (const Form *f : forms) {
      calls(desc(*f, m, 1024, 64, "bBr", V_GENERIC));
      calls(desc(*f, m, 1024, 64, "bBr", V_BF16_SMALL32));
      call(desc(*f, m, 1024, 64), 0);
    }
  }
  // the epilogues: beta 1 plain, beta 1 + bias, beta 0 plain
  for (const Form *f : forms) {
    calls(desc(*f, 8, 1024, 64, ""));
    calls(desc(*f, 8, 1024, 64, "B"));
    calls(desc(*f, 8, 1024, 64, "b"));
  }
  // each misalignment, on a call with a bias row: A / B, C (8 and 4 bytes), the bias (4 and 8 bytes)
  for (const Form *f : forms) {
    const GemmDesc d = desc(*f, 8, 1024, 64);
    call(d, 4, 8, 16, 16);
    call(d, 4, 16, 8, 16);
    call(d, 4, 16, 4, 16);
    call(d, 4, 16, 16, 4);
    call(d, 4, 16, 16, 8);
  }
  // leading dimensions wider than the rows (taken); each one off the 16-byte grid; each one too short
  for (const Form *f : forms) {
    calls(desc(*f, 8, 1024, 64, "bBr", -1, 1032, 1032, 1040));
    calls(desc(*f, 8, 1024, 64, "bBr", -1, 1028, 1024, 1024));
    calls(desc(*f, 8, 1024, 64, "bBr", -1, 1024, 1028, 1024));
    calls(desc(*f, 8, 1024, 64, "bBr", -1, 1024, 1024, 1028));
    call(desc(*f, 8, 1024, 64, "bBr", -1, 56, 1024, 1024), 1);
    call(desc(*f, 8, 1024, 64, "bBr", -1, 64, 1016, 1024), 1);
    call(desc(*f, 8, 1024, 64, "bBr", -1, 64, 1024, 1016), 1);
  }
  // n and k off the grid of 8
  calls(desc(V2, 8, 1004, 64));
  calls(desc(V2, 8, 1024, 36));
  calls(desc(FLAT, 8, 1024, 36));
  return 0;
}
