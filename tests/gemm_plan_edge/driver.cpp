// driver.cpp - TEST INFRASTRUCTURE for tests/test_gemm_plan_edge.py, never part of the product library.
//
// Steps a fixed list of whole-layer calls through the kernel planner (tpp-mlir_amd/csrc/gemm_plan.h) under every mode of the edge tiles
// (xsmm_hip_set_edge_tiles) and prints one line per call and environment; the test compares the output with
// tests/golden/gemm_plan_edge.txt and checks the rule's invariants on every line. Lines:
//   <m>x<n>x<k> br<batch> <f32|bf16> e<epilogue> lda<lda> ldb<ldb> ldc<ldc> al<ab16><c16><d16> f<forced variant> cus<CUs> :
//       v<variant> <launcher> t<tile> s<split> g<generic instance> "<text>" | <mode>:<decision> ...
// Left of the bar: the decision with the mode off (mode 0). Per mode 0, 1, 6, 7, 9, 10 then "-" = that decision, field by field, no edge
// launch; "e<variant>" = an edge launch on that GemmVariant's tile (launcher f32_lw, that tile's index, split 1, no tail, the tile's
// "..., edge tiles" text); anything else in full behind a "!".
#include "gemm_plan.h"
#include <stdio.h>
#include <string.h>

using namespace tpp;

namespace {

const int CUS[] = {256, 64};
const int MODES[] = {0, 1, 6, 7, 9, 10};
const int BM[4] = {64, 64, 32, 128}, BN[4] = {64, 32, 32, 64}; // the tiles of modes 6, 7, 9, 10

struct Call {
  int64_t m, n, k, br;
  const char *ep = "b";
  int64_t dtype = DT_F32;
  int64_t lda_extra = 0, ldb_extra = 0, ldc_extra = 0;
  GemmAlign al{true, true, true, true, true};
  int forced = -1;
};

// a whole-layer call as the reference's benchmarks issue it: A [m][K] row-major read in k-wide batch elements, B [K][n]
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
  return d;
}

const char *launcher_name(GemmLauncher l) {
  return l == GL_F32_LW ? "f32_lw" : l == GL_F32_LW16 ? "f32_lw16" : l == GL_F32_LW_GROUPED ? "f32_lw_grouped" : l == GL_F32_FAST ? "f32_fast"
         : l == GL_GENERIC ? "generic" : l == GL_NONE ? "none" : "other";
}
const char *edge_text(int variant) {
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
  printf("%ldx%ldx%ld br%ld %s e%s lda%ld ldb%ld ldc%ld al%d%d%d f%d cus%d : v%d %s t%d s%d g%d \"%s\" |", (long)c.m, (long)c.n, (long)c.k, (long)c.br,
         c.dtype == DT_F32 ? "f32" : "bf16", c.ep, (long)d.lda, (long)d.ldb, (long)d.ldc, (int)c.al.ab16, (int)c.al.c16, (int)c.al.d16, c.forced, cus,
         d.variant, launcher_name(off.launcher), off.tile, off.split, (int)off.generic, off.text);
  for (int mode : MODES) {
    env.edge_tiles = mode;
    GemmDesc e = layer(c);
    plan_gemm(e, c.forced, env);
    const GemmLaunch l = plan_gemm_call(e, c.br, c.al, env);
    const bool same = e.variant == d.variant && !strcmp(e.name, d.name) && l.launcher == off.launcher && l.tile == off.tile && l.split == off.split &&
                      l.b_kind == off.b_kind && l.even == off.even && l.vec == off.vec && l.generic == off.generic && !strcmp(l.text, off.text) &&
                      l.tail_tiles == off.tail_tiles && l.tail_split == off.tail_split;
    static const int variant_of_tile[5] = {-1, 6, 7, 9, 10};
    const int ev = l.edge && l.tile >= 1 && l.tile <= 4 ? variant_of_tile[l.tile] : -1;
    if (same && !l.edge) printf(" %d:-", mode);
    else if (ev > 0 && e.variant == d.variant && !strcmp(e.name, d.name) && l.launcher == GL_F32_LW && l.split == 1 && l.tail_tiles == 0 &&
             l.tail_split == 1 && !strcmp(l.text, edge_text(ev)))
      printf(" %d:e%d", mode, ev);
    else
      printf(" %d:!v%d %s t%d s%d edge%d \"%s\"", mode, e.variant, launcher_name(l.launcher), l.tile, l.split, (int)l.edge, l.text);
  }
  printf("\n");
}

void both(const Call &c) {
  for (int cus : CUS) line(c, cus);
}

} // namespace

int main() {
  // around every tile's eligibility edge: m = BM - 1, BM, BM + 1 and n = BN - 4, BN, BN + 4, BN + 2 (k = 64, one batch element)
  for (int t = 0; t < 4; ++t)
    for (int dm : {-1, 0, 1})
      for (int dn : {-4, 0, 4, 2}) both(Call{BM[t] + dm, BN[t] + dn, 64, 1});
  // the reduction: k = 32 (one and two batch elements), 64, 96; no batch element
  for (int64_t k : {32, 64, 96})
    for (int64_t br : {0, 1, 2}) both(Call{200, 1000, k, br});
  both(Call{192, 1000, 32, 2}), both(Call{192, 1000, 64, 2}); // (m a multiple of 32: the 32-k pairs and the ragged-n 32x32 tile of mode 0)
  // leading dimensions off the 4-float grid, each alignment bit off, a bias with and without its 16-byte alignment, the epilogues
  {
    Call c{200, 1000, 64, 4};
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
    x = c, x.ep = "bBr", x.al.d8 = false, x.al.d16 = false, both(x);
    x = c, x.ep = "bBr", both(x);
    x = c, x.ep = "Br", both(x);
    x = c, x.ep = "", both(x);
    x = c, x.forced = V_GENERIC, both(x);              // the generic kernel forced
    x = c, x.forced = V_F32_LW_64x64K2, both(x);       // a forced tile the shape does not divide: as planned
    x = c, x.dtype = DT_BF16, both(x);
  }
  // whole layers, K = 1024 and 512: ragged both ways, one way, a divisible control, skinny and tiny ones
  struct L { int64_t M, N, K; };
  const L layers[] = {{1000, 1000, 1024}, {1000, 1024, 1024}, {1024, 1000, 1024}, {4000, 4000, 1024}, {2000, 1000, 512}, {200, 1000, 1024},
                      {65, 68, 1024},     {1408, 1024, 1024}, {4000, 520, 1024},  {4000, 2000, 1024}, {1000, 1000, 64},  {200, 1000, 64},
                      {4000, 520, 64},    {520, 4000, 64},    {128, 68, 64},      {4096, 48, 64},     {129, 8200, 64},   {33, 36, 64},
                      {40, 16420, 64},    {1000, 1002, 64},   {31, 1000, 64},     {1000, 28, 64}};
  for (const L &l : layers) both(Call{l.M, l.N, 64, l.K / 64});
  return 0;
}
