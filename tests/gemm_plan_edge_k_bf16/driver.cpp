// driver.cpp - TEST INFRASTRUCTURE for tests/test_gemm_plan_edge_k_bf16.py, never part of the product library.
//
// Steps a fixed list of whole-layer calls through the kernel planner (tpp-mlir_amd/csrc/gemm_plan.h) under the modes of the bf16 ragged k
// (xsmm_hip_set_edge_k_bf16: 0, 1, 20 .. 23) crossed with edge-tile modes 0, 2 and 21, and prints one line per call and CU count; the test
// compares the output with tests/golden/gemm_plan_edge_k_bf16.txt and checks the rule on every line. Lines:
//   <m>x<n>x<k> br<batch> <f32|bf16> vf<0 flat|2|4> vc<VNNI C> e<epilogue> lda<lda> ldb<ldb> ldc<ldc> al<ab16><c16><d8> f<forced variant> cus<CUs> :
//       v<variant> vfd<variant forced> <launcher> t<tile> s<split> b<B image> g<generic instance> "<text>" | et<edge-tile mode>:<base> <mode>:<decision> ... | et...
// Left of the first bar: the decision with both switches off. <base>: the decision under the edge-tile mode alone - "-" = the one with
// both off, field by field; "e<variant>" = an edge launch on that tile. <decision> under edge_k_bf16 = 1, 20 .. 23 on top of it: "-" = the
// base decision, field by field, and no ragged-k launch; "k<variant>" = a ragged-k launch on that tile with its B image (20 + t VNNI-2,
// 24 + t flat, 28 + t VNNI-4), launcher bf16_lw, split 1, the tile's "..., ragged k" text; "K<variant>" = the same with the "..., edge
// tiles, ragged k" text; anything else in full behind a "!".
#include "gemm_plan.h"
#include <stdio.h>
#include <string.h>
#include <string>

using namespace tpp;

namespace {

const int CUS[] = {256, 64};
const int ETS[] = {0, 2, 21};
const int EKS[] = {1, 20, 21, 22, 23};
const int BM[4] = {32, 64, 64, 128}, BN[4] = {64, 64, 128, 128};

struct Call {
  int64_t m, n, k, br;
  int vf = 2; // B image: 0 flat, 2 VNNI-2, 4 VNNI-4
  const char *ep = "b";
  int64_t dtype = DT_BF16;
  int64_t lda_extra = 0, ldb_extra = 0, ldc_extra = 0;
  GemmAlign al{true, true, true, true, true};
  int forced = -1;
  int vnni_c = 0;
};

// a whole-layer call: A [m][br * k] row-major read in k-wide batch elements, B [br * k][n] (flat) or its VNNI-2 / VNNI-4 packing
GemmDesc layer(const Call &c) {
  GemmDesc d;
  memset(&d, 0, sizeof(d));
  d.kind = KIND_GEMM;
  d.has_batch = 1;
  d.dtype = c.dtype;
  d.m = c.m, d.n = c.n, d.k = c.k;
  d.lda = c.k * (c.br > 0 ? c.br : 1) + c.lda_extra;
  d.ldb = c.n + c.ldb_extra, d.ldc = c.n + c.ldc_extra;
  d.stride_a = c.k, d.stride_b = c.k * d.ldb;
  d.beta0 = strchr(c.ep, 'b') != nullptr;
  d.bias = strchr(c.ep, 'B') != nullptr;
  d.relu = strchr(c.ep, 'r') != nullptr;
  d.fused = d.bias || d.relu;
  if (c.dtype == DT_BF16) d.vnni_b = c.vf != 0, d.vnni_factor = c.vf, d.vnni_c = c.vnni_c;
  return d;
}

const char *launcher_name(GemmLauncher l) {
  return l == GL_F32_LW ? "f32_lw" : l == GL_F32_LW_GROUPED ? "f32_lw_grouped" : l == GL_BF16_LW ? "bf16_lw" : l == GL_BF16_SMALL32 ? "bf16_small32"
         : l == GL_BF16_FAST ? "bf16_fast" : l == GL_GENERIC ? "generic" : l == GL_NONE ? "none" : "other";
}
std::string tile_text(int variant, const char *suffix) {
  static const char *const tile[4] = {"<32x64,k2>", "<64x64>", "<64x128>", "<128x128>"};
  return std::string(variant < 24 ? "brgemm_bf16_lw" : variant < 28 ? "brgemm_bf16_lw_flatb" : "brgemm_bf16_lw_vnni4") + tile[variant & 3] + suffix;
}
struct Decision {
  GemmDesc d;
  GemmLaunch l;
};
Decision decide(const Call &c, int cus, int et, int ek) {
  GemmPlanEnv env{cus, false, -1};
  env.edge_tiles = et, env.edge_k_bf16 = ek;
  Decision x;
  x.d = layer(c);
  plan_gemm(x.d, c.forced, env);
  x.l = plan_gemm_call(x.d, c.br, c.al, env);
  return x;
}
bool same(const Decision &a, const Decision &b) {
  return a.d.variant == b.d.variant && !strcmp(a.d.name, b.d.name) && a.d.generic_forced == b.d.generic_forced && a.d.variant_forced == b.d.variant_forced &&
         a.l.launcher == b.l.launcher && a.l.tile == b.l.tile && a.l.split == b.l.split && a.l.b_kind == b.l.b_kind && a.l.even == b.l.even &&
         a.l.vec == b.l.vec && a.l.generic == b.l.generic && !strcmp(a.l.text, b.l.text) && a.l.tail_tiles == b.l.tail_tiles &&
         a.l.tail_split == b.l.tail_split && a.l.edge == b.l.edge && a.l.edge_k == b.l.edge_k;
}
int bf16_variant(const GemmLaunch &l) {
  return l.launcher == GL_BF16_LW && l.tile >= 0 && l.tile <= 3 && (l.b_kind == 0 || l.b_kind == 2 || l.b_kind == 4) ? 20 + 2 * l.b_kind + l.tile : -1;
}

void line(const Call &c, int cus) {
  GemmDesc d = layer(c);
  GemmPlanEnv env{cus, false, -1};
  if (!plan_gemm(d, c.forced, env)) {
    printf("%ldx%ldx%ld refused\n", (long)c.m, (long)c.n, (long)c.k);
    return;
  }
  const Decision off = decide(c, cus, 0, 0);
  printf("%ldx%ldx%ld br%ld %s vf%d vc%d e%s lda%ld ldb%ld ldc%ld al%d%d%d f%d cus%d : v%d vfd%d %s t%d s%d b%d g%d \"%s\"", (long)c.m, (long)c.n,
         (long)c.k, (long)c.br, c.dtype == DT_F32 ? "f32" : "bf16", c.dtype == DT_F32 ? 0 : c.vf, c.vnni_c, c.ep, (long)d.lda, (long)d.ldb, (long)d.ldc,
         (int)c.al.ab16, (int)c.al.c16, (int)c.al.d8, c.forced, cus, off.d.variant, off.d.variant_forced, launcher_name(off.l.launcher), off.l.tile,
         off.l.split, off.l.b_kind, (int)off.l.generic, off.l.text);
  for (int et : ETS) {
    const Decision base = decide(c, cus, et, 0);
    const int bv = bf16_variant(base.l);
    if (same(base, off) && !base.l.edge && !base.l.edge_k) printf(" | et%d:-", et);
    else if (base.l.edge && !base.l.edge_k && bv > 0 && base.l.split == 1 && tile_text(bv, ", edge tiles") == base.l.text) printf(" | et%d:e%d", et, bv);
    else if (base.l.edge && base.l.launcher == GL_F32_LW) printf(" | et%d:f%d", et, base.l.tile); // (an f32 control under mode 2: its own edge tiles)
    else printf(" | et%d:!v%d %s t%d \"%s\"", et, base.d.variant, launcher_name(base.l.launcher), base.l.tile, base.l.text);
    for (int ek : EKS) {
      const Decision x = decide(c, cus, et, ek);
      const int v = bf16_variant(x.l);
      const bool desc_same = x.d.variant == off.d.variant && !strcmp(x.d.name, off.d.name) && x.d.generic_forced == off.d.generic_forced &&
                             x.d.variant_forced == off.d.variant_forced;
      if (same(x, base)) printf(" %d:-", ek);
      else if (x.l.edge_k && !x.l.edge && desc_same && v > 0 && x.l.split == 1 && x.l.tail_tiles == 0 && tile_text(v, ", ragged k") == x.l.text) printf(" %d:k%d", ek, v);
      else if (x.l.edge_k && !x.l.edge && desc_same && v > 0 && x.l.split == 1 && x.l.tail_tiles == 0 && tile_text(v, ", edge tiles, ragged k") == x.l.text)
        printf(" %d:K%d", ek, v);
      else printf(" %d:!v%d %s t%d s%d b%d edge%d%d \"%s\"", ek, x.d.variant, launcher_name(x.l.launcher), x.l.tile, x.l.split, x.l.b_kind, (int)x.l.edge, (int)x.l.edge_k, x.l.text);
    }
  }
  printf("\n");
}

void both(const Call &c) {
  for (int cus : CUS) line(c, cus);
}
void images(Call c) {
  for (int vf : {2, 0, 4}) c.vf = vf, both(c);
}

} // namespace

int main() {
  // around every tile's eligibility edge: m = BM - 1, BM, BM + 1 and n = BN - 8, BN, BN + 8, BN + 4, at k = 80 (one batch element) and 784 (three)
  for (int t = 0; t < 4; ++t)
    for (int dm : {-1, 0, 1})
      for (int dn : {-8, 0, 8, 4}) both(Call{BM[t] + dm, BN[t] + dn, 80, 1}), both(Call{BM[t] + dm, BN[t] + dn, 784, 3});
  // the reduction: below a chunk, whole chunks, k % 16 != 0, the lengths taken; no, one and three batch elements
  for (int64_t k : {48, 64, 72, 80, 96, 128, 784})
    for (int64_t br : {0, 1, 3}) both(Call{256, 1024, k, br}), both(Call{200, 1000, k, br});
  both(Call{256, 1024, 1000, 1}), both(Call{256, 1024, 200, 1}); // k % 8 == 0 only: out of scope
  // shapes whose divisible plan is the 32x32 K-split kernel (n a multiple of 32, not of 64)
  both(Call{96, 96, 80, 1}), both(Call{256, 992, 80, 8}), both(Call{96, 96, 784, 2});
  // each leading dimension off its grid (and all of them on it again), per B image
  for (int vf : {2, 0, 4}) {
    Call c{256, 1024, 80, 2};
    c.vf = vf;
    Call x = c;
    x.lda_extra = 4, both(x);
    x = c, x.ldc_extra = 4, both(x);
    x = c, x.ldb_extra = vf == 2 ? 2 : vf == 0 ? 4 : 1, both(x);
    x = c, x.lda_extra = 8, x.ldb_extra = 8, x.ldc_extra = 8, both(x);
  }
  {
    Call c{256, 1024, 80, 2};
    Call x = c;
    x.al.ab16 = false, both(x);
    x = c, x.al.c16 = false, both(x);
    x = c, x.al.c16 = false, x.al.c8 = false, both(x);
    x = c, x.al.d8 = false, x.al.d16 = false, both(x);                  // no bias: D is not read
    x = c, x.ep = "bBr", x.al.d16 = false, both(x);                     // a bias row on 8 bytes
    x = c, x.ep = "bBr", x.al.d8 = false, x.al.d16 = false, both(x);    // ... off them
    x = c, x.ep = "bBr", both(x);
    x = c, x.ep = "Br", both(x);
    x = c, x.ep = "", both(x);
    x = c, x.forced = V_GENERIC, both(x);          // the generic kernel forced
    x = c, x.forced = V_BF16_LW_64x64, both(x);    // a forced tile the k does not allow: as planned
    x = c, x.forced = V_BF16_SMALL32, both(x);     // a forced variant
    x = c, x.vnni_c = 1, both(x);                  // VNNI-2 C: the generic kernel's epilogue only
    x = c, x.dtype = DT_F32, both(x);              // f32 controls: never taken by this switch
    x = Call{1000, 1000, 80, 1}, x.dtype = DT_F32, both(x);
    x = Call{1024, 1024, 784, 1}, x.dtype = DT_F32, both(x);
  }
  // whole layers, all three B images: the rows of the A/B, ragged m / n with and without the edge tiles, a divisible-k control
  struct L { int64_t M, N, K; };
  const L layers[] = {{1024, 1024, 784}, {4096, 1024, 784}, {256, 1024, 400}, {128, 1024, 80}, {1000, 1000, 784}, {2048, 2048, 1200}, {1025, 1096, 80},
                      {72, 72, 112}, {1024, 1024, 832}, {512, 1024, 2000}};
  for (const L &l : layers) images(Call{l.M, l.N, l.K, 1});
  images(Call{1024, 1024, 112, 7});
  return 0;
}
