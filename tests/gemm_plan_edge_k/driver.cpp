// driver.cpp - TEST INFRASTRUCTURE for tests/test_gemm_plan_edge_k.py, never part of the product library.
//
// Steps a fixed list of whole-layer calls through the kernel planner (tpp-mlir_amd/csrc/gemm_plan.h) under every mode of the ragged-k
// switch (xsmm_hip_set_edge_k) combined with edge-tile modes 0, 1, 2, 6, 10 and 21 (xsmm_hip_set_edge_tiles) and prints one line per call
// and CU count; the test compares the output with tests/golden/gemm_plan_edge_k.txt and checks the rule on every line. Lines:
//   <m>x<n>x<k> br<batch> <f32|bf16> e<epilogue> lda<lda> ldb<ldb> ldc<ldc> al<ab16><c16><d16> f<forced variant> x<a_trans><b_trans><vnni_c> cus<CUs> :
//       v<variant> <launcher> t<tile> s<split> g<generic instance> "<text>" | et<edge-tile mode>:<decision> <edge_k mode>:<decision> ... | et...
// Left of the first bar: the decision with both switches off. Behind "et<mode>:" the decision under that edge-tile mode with edge_k 0,
// against the one with both off: "-" = the same, field by field; "e<variant>" = an edge-tile launch on that GemmVariant's tile. Then per
// edge_k mode 1, 6, 7, 9, 10 the decision against the one of the SAME edge-tile mode with edge_k 0: "-" = the same, field by field, and no
// ragged-k launch; "k<variant>" = a ragged-k launch on that GemmVariant's tile (launcher f32_lw, the tile's index, split 1, no tail, no
// edge flag, the text "<tile>, ragged k"); "K<variant>" = the same with the text "<tile>, edge tiles, ragged k"; anything else in full
// behind a "!".
#include "gemm_plan.h"
#include <initializer_list>
#include <stdio.h>
#include <string.h>
#include <string>

using namespace tpp;

namespace {

const int CUS[] = {256, 64};
const int ETS[] = {0, 1, 2, 6, 10, 21};
const int EKS[] = {1, 6, 7, 9, 10};
const int BM[4] = {64, 64, 32, 128}, BN[4] = {64, 32, 32, 64}; // the tiles of modes 6, 7, 9, 10

struct Call {
  int64_t m, n, k, br;
  const char *ep = "b";
  int64_t dtype = DT_F32;
  int64_t lda_extra = 0, ldb_extra = 0, ldc_extra = 0;
  GemmAlign al{true, true, true, true, true};
  int forced = -1;
  int a_trans = 0, b_trans = 0, vnni_c = 0, f32_prec = 0;
};

// a whole-layer call: A [m][k * br] row-major read in k-wide batch elements, B [k * br][n]
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
  d.vnni_c = c.vnni_c;
  d.f32_prec = c.f32_prec;
  return d;
}

const char *launcher_name(GemmLauncher l) {
  return l == GL_F32_LW ? "f32_lw" : l == GL_F32_LW16 ? "f32_lw16" : l == GL_F32_LW_GROUPED ? "f32_lw_grouped" : l == GL_F32_FAST ? "f32_fast"
         : l == GL_GENERIC ? "generic" : l == GL_NONE ? "none" : l == GL_INVALID ? "invalid" : "other";
}
const char *tile_text(int variant) {
  return variant == 6 ? "brgemm_f32_lw<64x64,k2>" : variant == 7 ? "brgemm_f32_lw<64x32,k4>" : variant == 9 ? "brgemm_f32_lw<32x32,k4>" : "brgemm_f32_lw<128x64,k1>";
}

struct Planned { GemmDesc d; GemmLaunch l; bool ok; };
Planned plan(const Call &c, int cus, int et, int ek) {
  Planned p;
  p.d = layer(c);
  GemmPlanEnv env{cus, false, -1};
  env.edge_tiles = et, env.edge_k = ek;
  p.ok = plan_gemm(p.d, c.forced, env);
  p.d.a_trans = c.a_trans, p.d.b_trans = c.b_trans, p.d.trans_mode = c.a_trans ? 2 : c.b_trans ? 1 : 0; // (siblings are made after dispatch)
  p.l = p.ok ? plan_gemm_call(p.d, c.br, c.al, env) : GemmLaunch{GL_INVALID, 0, 1, 0, false, false, GG_F32, ""};
  return p;
}
bool same(const Planned &a, const Planned &b) {
  return a.d.variant == b.d.variant && !strcmp(a.d.name, b.d.name) && a.l.launcher == b.l.launcher && a.l.tile == b.l.tile && a.l.split == b.l.split &&
         a.l.b_kind == b.l.b_kind && a.l.even == b.l.even && a.l.vec == b.l.vec && a.l.generic == b.l.generic && !strcmp(a.l.text, b.l.text) &&
         a.l.tail_tiles == b.l.tail_tiles && a.l.tail_split == b.l.tail_split && a.l.edge == b.l.edge && a.l.edge_k == b.l.edge_k;
}
void full(const Planned &p) {
  printf("!v%d %s t%d s%d edge%d edgek%d \"%s\"", p.d.variant, launcher_name(p.l.launcher), p.l.tile, p.l.split, (int)p.l.edge, (int)p.l.edge_k, p.l.text);
}

void line(const Call &c, int cus) {
  const Planned off = plan(c, cus, 0, 0);
  if (!off.ok) {
    printf("%ldx%ldx%ld refused\n", (long)c.m, (long)c.n, (long)c.k);
    return;
  }
  printf("%ldx%ldx%ld br%ld %s e%s lda%ld ldb%ld ldc%ld al%d%d%d f%d x%d%d%d cus%d : v%d %s t%d s%d g%d \"%s\"", (long)c.m, (long)c.n, (long)c.k, (long)c.br,
         c.dtype == DT_F32 ? "f32" : "bf16", c.ep, (long)off.d.lda, (long)off.d.ldb, (long)off.d.ldc, (int)c.al.ab16, (int)c.al.c16, (int)c.al.d16, c.forced,
         c.a_trans, c.b_trans, c.vnni_c, cus, off.d.variant, launcher_name(off.l.launcher), off.l.tile, off.l.split, (int)off.l.generic, off.l.text);
  static const int variant_of_tile[5] = {-1, 6, 7, 9, 10};
  for (int et : ETS) {
    const Planned base = plan(c, cus, et, 0);
    printf(" | et%d:", et);
    const int bv = base.l.edge && !base.l.edge_k && base.l.launcher == GL_F32_LW && base.l.tile >= 1 && base.l.tile <= 4 ? variant_of_tile[base.l.tile] : -1;
    if (same(base, off)) printf("-");
    else if (bv > 0 && base.d.variant == off.d.variant && !strcmp(base.l.text, (std::string(tile_text(bv)) + ", edge tiles").c_str())) printf("e%d", bv);
    else full(base);
    for (int ek : EKS) {
      const Planned p = plan(c, cus, et, ek);
      const int kv = p.l.edge_k && p.l.tile >= 1 && p.l.tile <= 4 ? variant_of_tile[p.l.tile] : -1;
      const bool shape = kv > 0 && p.d.variant == base.d.variant && !strcmp(p.d.name, base.d.name) && p.l.launcher == GL_F32_LW && p.l.split == 1 &&
                         p.l.tail_tiles == 0 && p.l.tail_split == 1 && !p.l.edge;
      printf(" %d:", ek);
      if (same(p, base) && !p.l.edge_k) printf("-");
      else if (shape && !strcmp(p.l.text, (std::string(tile_text(kv)) + ", ragged k").c_str())) printf("k%d", kv);
      else if (shape && !strcmp(p.l.text, (std::string(tile_text(kv)) + ", edge tiles, ragged k").c_str())) printf("K%d", kv);
      else full(p);
    }
  }
  printf("\n");
}

void both(const Call &c) {
  for (int cus : CUS) line(c, cus);
}

} // namespace

int main() {
  // around every tile: m = BM - 1, BM, BM + 1, 2 BM and n = BN - 4, BN, BN + 4, BN + 2, 2 BN (k = 72, one batch element)
  for (int t = 0; t < 4; ++t)
    for (int dm : {-1, 0, 1, BM[t]})
      for (int dn : {-4, 0, 4, 2, BN[t]}) both(Call{BM[t] + dm, BN[t] + dn, 72, 1});
  // the reduction, on a divisible and on a ragged output: below 64, multiples of 64, of 8, of 4 only, odd; no batch element, one, three
  for (int64_t k : {32, 56, 64, 72, 80, 96, 100, 104, 127, 128, 200, 784, 1000})
    for (int64_t br : {0, 1, 3}) both(Call{256, 1024, k, br}), both(Call{200, 1000, k, br});
  // leading dimensions off the 4-float grid, each alignment bit off, a bias with and without its 16 bytes, the epilogues, forced kernels,
  // bf16, a transposed operand, a VNNI C, a bf16x6 descriptor (ragged k: planned on the exact generic kernel)
  for (const Call &c : {Call{256, 1024, 200, 1}, Call{200, 1000, 200, 1}}) {
    Call x = c;
    x.ldc_extra = 2, both(x);
    x = c, x.ldc_extra = 4, both(x);
    x = c, x.lda_extra = 2, both(x);
    x = c, x.ldb_extra = 2, both(x);
    x = c, x.lda_extra = 8, x.ldb_extra = 4, x.ldc_extra = 4, both(x);
    x = c, x.al.ab16 = false, both(x);
    x = c, x.al.c16 = false, both(x);
    x = c, x.al.d16 = false, both(x);                  // no bias: D is not read
    x = c, x.ep = "bBr", x.al.d16 = false, both(x);    // a bias row off its 16 bytes
    x = c, x.ep = "bBr", both(x);
    x = c, x.ep = "Br", both(x);
    x = c, x.ep = "", both(x);
    x = c, x.forced = V_GENERIC, both(x);              // the generic kernel forced
    x = c, x.forced = V_F32_LW_64x64K2, both(x);       // a forced tile that does not take the k: as planned
    x = c, x.dtype = DT_BF16, both(x);
    x = c, x.b_trans = 1, both(x);
    x = c, x.a_trans = 1, both(x);
    x = c, x.vnni_c = 1, both(x);
    x = c, x.f32_prec = 6, x.forced = V_F32_X6_64x64, both(x);
  }
  // whole layers with a ragged K as one batch element: divisible outputs, ragged ones, skinny and tiny ones
  struct L { int64_t M, N, K; };
  const L layers[] = {{1024, 1024, 1000}, {512, 1024, 784}, {256, 1024, 200}, {128, 1024, 72},  {1000, 1000, 1000}, {2048, 1024, 1000}, {4096, 4096, 1000},
                      {200, 1000, 784},   {65, 68, 200},    {64, 64, 72},     {32, 32, 72},     {128, 64, 120},     {4000, 520, 1000},  {31, 1000, 200},
                      {1000, 28, 200},    {1024, 1002, 200}};
  for (const L &l : layers) both(Call{l.M, l.N, l.K, 1});
  return 0;
}
