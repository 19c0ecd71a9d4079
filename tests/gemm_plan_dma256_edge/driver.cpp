// driver.cpp - TEST INFRASTRUCTURE for tests/test_gemm_plan_dma256_edge.py, never part of the product library.
//
// Steps whole-layer bf16 calls through the kernel planner (tpp-mlir_amd/csrc/gemm_plan.h) under the modes of xsmm_hip_set_dma256_edge (0, 1, 2)
// and prints, in the notation of tests/gemm_plan/driver.cpp without its descriptor numbers, one line per descriptor
//   <form> <m>x<n>x<k> [ld<lda>,<ldb>,<ldc>] e<epilogue> f<forced> : <variant> <name> [gf] [vf] [bk<B image>]
// and under it one line per call
//   c br<batch> [a<A,B>/<C>/<D alignment>] [strict] : <launch, mode 0> | <mode 1> | <mode 2> | others <same | DIFFER>
// where the mode-0 launch comes from a GemmPlanEnv that never names the new field, and a mode-1 / mode-2 launch that is the mode-0 one field
// by field prints as "-". An edge-tile launch on the 256x256 tile prints as bf16_fast t2 b<image> edge "<text>". others: under each mode,
// with every other switch of the environment turned on (one at a time and all together), this switch takes the call or not as it does
// with them off.
#include "gemm_plan.h"
#include <stdio.h>
#include <string.h>
#include <string>

using namespace tpp;

namespace {

const int CUS = 256;

struct Form {
  const char *name;
  int vnni_b, vf, vnni_c;
};
const Form V2{"v2", 1, 2, 0}, V4{"v4", 1, 4, 0}, FLAT{"flat", 0, 0, 0}, VC{"vc", 1, 2, 1}, VC4{"vc4", 1, 4, 1};

GemmDesc desc(const Form &f, int64_t m, int64_t n, int64_t k, const char *ep = "b", int forced = -1, int64_t lda = -1, int64_t ldb = -1, int64_t ldc = -1) {
  GemmDesc d;
  memset(&d, 0, sizeof(d));
  d.kind = KIND_GEMM;
  d.has_batch = 1;
  d.dtype = DT_BF16;
  d.m = m, d.n = n, d.k = k;
  d.lda = lda >= 0 ? lda : k;
  d.ldb = ldb >= 0 ? ldb : n;
  d.ldc = ldc >= 0 ? ldc : n;
  d.stride_a = m * k;
  d.stride_b = k * n;
  d.beta0 = strchr(ep, 'b') != nullptr;
  d.bias = strchr(ep, 'B') != nullptr;
  d.relu = strchr(ep, 'r') != nullptr;
  d.fused = d.bias || d.relu;
  d.vnni_b = f.vnni_b;
  d.vnni_factor = f.vf;
  d.vnni_c = f.vnni_c;
  const bool ok = plan_gemm(d, forced, GemmPlanEnv{CUS, false, -1});
  printf("%s %ldx%ldx%ld", f.name, (long)m, (long)n, (long)k);
  if (lda >= 0 || ldb >= 0 || ldc >= 0) printf(" ld%ld,%ld,%ld", (long)d.lda, (long)d.ldb, (long)d.ldc);
  printf(" e%s f%d : %s%d %s", *ep ? ep : "-", forced, ok ? "" : "!", d.variant, d.name);
  if (d.generic_forced) printf(" gf");
  if (d.variant_forced) printf(" vf");
  if (bf16_lw_b_kind(d) >= 0) printf(" bk%d", bf16_lw_b_kind(d));
  printf("\n");
  return d;
}

const char *generic_name(GemmGeneric g) {
  switch (g) {
  case GG_BF16_VNNI2: return "<bf16,vnni2>";
  case GG_BF16_VNNI2_VEC: return "<bf16,vnni2,vec>";
  case GG_BF16_VNNI4_VEC: return "<bf16,vnni4,vec>";
  case GG_BF16_FLAT: return "<bf16,flat>";
  default: return "?";
  }
}

bool taken(const GemmLaunch &l) { return l.launcher == GL_BF16_FAST && l.edge; }

std::string launch_text(const GemmLaunch &l) {
  char buf[256];
  switch (l.launcher) {
  case GL_NONE: snprintf(buf, sizeof buf, "none"); break;
  case GL_INVALID: snprintf(buf, sizeof buf, "invalid"); break;
  case GL_BF16_FAST:
    if (l.edge) snprintf(buf, sizeof buf, "bf16_fast t%d b%d edge", l.tile, l.b_kind);
    else if (l.b_kind) snprintf(buf, sizeof buf, "bf16_fast t%d b%d", l.tile, l.b_kind);
    else snprintf(buf, sizeof buf, "bf16_fast t%d", l.tile);
    break;
  case GL_BF16_SMALL32: snprintf(buf, sizeof buf, "bf16_small32 s%d", l.split); break;
  case GL_BF16_LW: snprintf(buf, sizeof buf, "bf16_lw t%d b%d", l.tile, l.b_kind); break;
  case GL_GENERIC: snprintf(buf, sizeof buf, "generic%s", generic_name(l.generic)); break;
  default: snprintf(buf, sizeof buf, "other%d", (int)l.launcher); break;
  }
  std::string s = buf;
  if (l.text && *l.text) s += std::string(" \"") + l.text + "\"";
  if ((l.edge && !taken(l)) || l.edge_k || l.edge_k8 || l.halves || l.tail_tiles || l.split != 1) s += " !flags";
  return s;
}

// alignments in bytes: A and B, C, D
void call(const GemmDesc &d, int64_t br, bool strict = false, int ab = 16, int c = 16, int dd = 16) {
  const GemmAlign al{ab >= 16, c >= 16, c >= 8, dd >= 8, dd >= 16};
  printf(" c br%ld", (long)br);
  if (ab != 16 || c != 16 || dd != 16) printf(" a%d/%d/%d", ab, c, dd);
  if (strict) printf(" strict");
  const std::string off = launch_text(plan_gemm_call(d, br, al, GemmPlanEnv{CUS, strict, -1}));
  printf(" : %s", off.c_str());
  bool others_same = true;
  for (int mode = 0; mode <= 2; ++mode) {
    GemmPlanEnv e{CUS, strict, -1};
    e.dma256_edge = mode;
    const GemmLaunch l = plan_gemm_call(d, br, al, e);
    const std::string on = launch_text(l);
    if (mode == 0) {
      if (on != off) printf(" !mode 0 differs from an environment without the field");
      if (taken(l)) printf(" !taken under mode 0");
    } else {
      printf(" | %s", on == off ? "-" : on.c_str());
    }
    // every other switch, one at a time and all together
    for (int which = 0; which < 8; ++which) {
      GemmPlanEnv o = e;
      if (which == 0 || which == 7) o.edge_tiles = 2;
      if (which == 1) o.edge_tiles = V_BF16_LW_128x128;
      if (which == 2 || which == 7) o.edge_k_bf16 = 1;
      if (which == 3 || which == 7) o.edge_k8_bf16 = 1;
      if (which == 4 || which == 7) o.dma256_images = 2;
      if (which == 5 || which == 7) o.tail_split = 1, o.halves = 2, o.edge_k = 1;
      if (which == 6) o.forced_split = 4;
      if (taken(plan_gemm_call(d, br, al, o)) != taken(l)) others_same = false;
    }
  }
  printf(" | others %s\n", others_same ? "same" : "DIFFER");
}

void calls(const GemmDesc &d) {
  call(d, 1);
  call(d, 1, true);
  call(d, 4);
  call(d, 0);
}

} // namespace

int main() {
  const Form *forms[3] = {&V2, &V4, &FLAT};
  // the measured shapes (profiles/dma256_edge_ab.txt); a divisible one; m, then n, below the tile; n % 8 != 0; k % 32 != 0; k % 64 != 0 (taken);
  // 15 x 16 = 240 tiles (the rule's edge) and 15 x 15 = 225 (below it)
  static const int64_t shapes[][3] = {{4000, 4096, 1024}, {4096, 4000, 1024}, {4100, 4096, 1024}, {5000, 5000, 1024}, {8000, 8000, 1024},
                                      {16000, 1024, 1024}, {256, 256, 1024},  {255, 4096, 1024},  {4096, 248, 1024},  {4096, 4004, 1024},
                                      {4000, 4096, 1000},  {4000, 4096, 96},  {3800, 4096, 1024}, {3800, 3800, 1024}};
  for (const Form *f : forms)
    for (auto &s : shapes) calls(desc(*f, s[0], s[1], s[2]));
  // rows of tests/golden/gemm_plan.txt: divisible, and a ragged n the switch is eligible for
  for (const Form *f : forms) calls(desc(*f, 4096, 4096, 4096));
  calls(desc(V2, 1024, 352, 512, "bBr"));
  calls(desc(V4, 1024, 352, 512, "bBr"));
  // each misalignment, on a call with a bias row: A / B, C, the bias
  for (const Form *f : forms) {
    const GemmDesc d = desc(*f, 4000, 4096, 1024, "bBr");
    calls(d);
    call(d, 1, false, 8, 16, 16);
    call(d, 1, false, 16, 8, 16);
    call(d, 1, false, 16, 16, 4);
    call(d, 1, false, 16, 16, 8);
  }
  // beta 1; leading dimensions wider than the rows; a leading dimension off the 16-byte grid
  for (const Form *f : forms) {
    calls(desc(*f, 4000, 4096, 1024, ""));
    calls(desc(*f, 4000, 4096, 1024, "b", -1, 1032, 4104, 4112));
    calls(desc(*f, 4000, 4096, 1024, "b", -1, 1024, 4096, 4100));
  }
  // forced variants: a loader-wave tile that divides the shape, the generic kernel
  calls(desc(V2, 4000, 4096, 1024, "b", V_BF16_LW_32x64));
  calls(desc(V4, 4000, 4096, 1024, "b", V_BF16_LW4_32x64));
  calls(desc(FLAT, 4000, 4096, 1024, "b", V_BF16_LWF_32x64));
  calls(desc(V2, 4000, 4096, 1024, "b", V_GENERIC));
  calls(desc(FLAT, 4000, 4096, 1024, "b", V_GENERIC));
  calls(desc(V4, 4000, 4096, 1024, "b", V_GENERIC));
  // a VNNI C
  calls(desc(VC, 4000, 4096, 1024));
  calls(desc(VC4, 4000, 4096, 1024));
  return 0;
}
