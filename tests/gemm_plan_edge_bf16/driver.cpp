// driver.cpp - TEST INFRASTRUCTURE for tests/test_gemm_plan_edge_bf16.py, never part of the product library.
//
// Steps a fixed list of whole-layer calls through the kernel planner (tpp-mlir_amd/csrc/gemm_plan.h) under the modes of the edge tiles
// (xsmm_hip_set_edge_tiles) that concern bf16 - and some that must not - and prints one line per call and environment; the test compares
// the output with tests/golden/gemm_plan_edge_bf16.txt and checks the rule's invariants on every line. Lines:
//   <m>x<n>x<k> br<batch> <f32|bf16> vf<0 flat|2|4> vc<VNNI C> e<epilogue> lda<lda> ldb<ldb> ldc<ldc> al<ab16><c16><d8> f<forced variant> cus<CUs> :
//       v<variant> vfd<variant forced> <launcher> t<tile> s<split> b<B image> g<generic instance> "<text>" | <mode>:<decision> ...
// Left of the bar: the decision with the mode off (mode 0). Per mode 0, 1, 2, 6, 20, 21, 22, 23 then "-" = that decision, field by field,
// no edge launch; "e<variant>" = an edge launch on that GemmVariant's tile - bf16: launcher bf16_lw, the tile's index and the B image of
// the variant number (20 + t VNNI-2, 24 + t flat, 28 + t VNNI-4), f32: launcher f32_lw and the tile of variant 6 / 7 / 9 / 10 -, split 1,
// no tail, the tile's "..., edge tiles" text; anything else in full behind a "!".
#include "gemm_plan.h"
#include <stdio.h>
#include <string.h>
#include <string>

using namespace tpp;

namespace {

const int CUS[] = {256, 64};
const int MODES[] = {0, 1, 2, 6, 20, 21, 22, 23};
const int BM[4] = {32, 64, 64, 128}, BN[4] = {64, 64, 128, 128}; // the tiles of modes 20 .. 23

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

// a whole-layer call as the reference's benchmarks issue it: A [m][K] row-major read in k-wide batch elements, B [K][n] (flat) or its
// VNNI-2 / VNNI-4 packing [K / v][n][v]
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
std::string edge_text(int variant) {
  static const char *const tile[4] = {"<32x64,k2>", "<64x64>", "<64x128>", "<128x128>"};
  if (variant >= 20 && variant < 32)
    return std::string(variant < 24 ? "brgemm_bf16_lw" : variant < 28 ? "brgemm_bf16_lw_flatb" : "brgemm_bf16_lw_vnni4") + tile[variant & 3] + ", edge tiles";
  return variant == 6 ? "brgemm_f32_lw<64x64,k2>, edge tiles" : variant == 7 ? "brgemm_f32_lw<64x32,k4>, edge tiles"
         : variant == 9 ? "brgemm_f32_lw<32x32,k4>, edge tiles" : "brgemm_f32_lw<128x64,k1>, edge tiles";
}

void line(const Call &c, int cus) {
  GemmDesc d = layer(c);
  GemmPlanEnv env{cus, false, -1};
  if (!plan_gemm(d, c.forced, env)) {
    printf("%ldx%ldx%ld refused\n", (long)c.m, (long)c.n, (long)c.k);
    return;
  }
  const GemmLaunch off = plan_gemm_call(d, c.br, c.al, env);
  printf("%ldx%ldx%ld br%ld %s vf%d vc%d e%s lda%ld ldb%ld ldc%ld al%d%d%d f%d cus%d : v%d vfd%d %s t%d s%d b%d g%d \"%s\" |", (long)c.m, (long)c.n,
         (long)c.k, (long)c.br, c.dtype == DT_F32 ? "f32" : "bf16", c.dtype == DT_F32 ? 0 : c.vf, c.vnni_c, c.ep, (long)d.lda, (long)d.ldb, (long)d.ldc,
         (int)c.al.ab16, (int)c.al.c16, (int)c.al.d8, c.forced, cus, d.variant, d.variant_forced, launcher_name(off.launcher), off.tile, off.split,
         off.b_kind, (int)off.generic, off.text);
  for (int mode : MODES) {
    env.edge_tiles = mode;
    GemmDesc e = layer(c);
    plan_gemm(e, c.forced, env);
    const GemmLaunch l = plan_gemm_call(e, c.br, c.al, env);
    const bool desc_same = e.variant == d.variant && !strcmp(e.name, d.name) && e.generic_forced == d.generic_forced && e.variant_forced == d.variant_forced;
    const bool same = desc_same && l.launcher == off.launcher && l.tile == off.tile && l.split == off.split && l.b_kind == off.b_kind &&
                      l.even == off.even && l.vec == off.vec && l.generic == off.generic && !strcmp(l.text, off.text) &&
                      l.tail_tiles == off.tail_tiles && l.tail_split == off.tail_split;
    static const int variant_of_tile[5] = {-1, 6, 7, 9, 10};
    int ev = -1;
    if (l.edge && l.launcher == GL_F32_LW && l.tile >= 1 && l.tile <= 4) ev = variant_of_tile[l.tile];
    if (l.edge && l.launcher == GL_BF16_LW && l.tile >= 0 && l.tile <= 3 && (l.b_kind == 0 || l.b_kind == 2 || l.b_kind == 4)) ev = 20 + 2 * l.b_kind + l.tile;
    if (same && !l.edge) printf(" %d:-", mode);
    else if (ev > 0 && desc_same && l.split == 1 && l.tail_tiles == 0 && l.tail_split == 1 && edge_text(ev) == l.text)
      printf(" %d:e%d", mode, ev);
    else
      printf(" %d:!v%d %s t%d s%d b%d edge%d \"%s\"", mode, e.variant, launcher_name(l.launcher), l.tile, l.split, l.b_kind, (int)l.edge, l.text);
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
  // around every tile's eligibility edge: m = BM - 1, BM, BM + 1 and n = BN - 8, BN, BN + 8, BN + 4 (k = 64, one batch element)
  for (int t = 0; t < 4; ++t)
    for (int dm : {-1, 0, 1})
      for (int dn : {-8, 0, 8, 4}) both(Call{BM[t] + dm, BN[t] + dn, 64, 1});
  // the reduction: k = 32, 64, 96 with no, one and two batch elements
  for (int64_t k : {32, 64, 96})
    for (int64_t br : {0, 1, 2}) both(Call{200, 1000, k, br});
  // planned on the 32x32 K-split kernel (m, n multiples of 32, n not of 64), short and long reduction; the same with that variant forced
  both(Call{96, 96, 64, 1}), both(Call{96, 96, 64, 32}), both(Call{256, 992, 64, 16});
  {
    Call x{96, 96, 64, 4};
    x.forced = V_BF16_SMALL32, both(x);
  }
  // each leading dimension off its grid (and all of them on it again), each alignment bit off, a bias with and without its 8 bytes
  for (int vf : {2, 0, 4}) {
    Call c{200, 1000, 64, 4};
    c.vf = vf;
    Call x = c;
    x.lda_extra = 4, both(x);
    x = c, x.ldc_extra = 4, both(x);
    x = c, x.ldb_extra = vf == 2 ? 2 : vf == 0 ? 4 : 1, both(x);
    x = c, x.lda_extra = 8, x.ldb_extra = 8, x.ldc_extra = 8, both(x);
  }
  {
    Call c{200, 1000, 64, 4};
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
    x = c, x.forced = V_BF16_LW_64x64, both(x);    // a forced tile the shape does not divide: as planned
    x = c, x.vnni_c = 1, both(x);                  // VNNI-2 C: the generic kernel's epilogue only
    x = c, x.dtype = DT_F32, both(x);              // the f32 control: mode 2 = mode 1, modes 20 .. 23 = off
    x = Call{1000, 1000, 64, 16}, x.dtype = DT_F32, both(x);
  }
  // whole layers at K = 1024 and at one chunk, all three B images: divisible controls (1024x1024; 96x128, which the 32x64 tile divides),
  // ragged one way and both ways, a tiny one
  struct L { int64_t M, N; };
  const L layers[] = {{1024, 1024}, {96, 128}, {4096, 1024}, {1000, 1000}, {200, 1000}, {4100, 1024}, {1000, 1024}, {2000, 1000}, {72, 72}, {1024, 1000}};
  for (const L &l : layers)
    for (int64_t br : {16, 1}) images(Call{l.M, l.N, 64, br});
  return 0;
}
