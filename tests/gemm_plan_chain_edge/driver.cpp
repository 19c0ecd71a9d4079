// driver.cpp - TEST INFRASTRUCTURE for tests/test_gemm_plan_chain_edge.py, never part of the product library.
//
// Steps a fixed list of bf16 / f32 layer chains through the planner's two ragged-chain functions (tpp-mlir_amd/csrc/gemm_plan.h
// chain_edge_b_kind, plan_chain_edge; xsmm_hip_set_chain_edge) and prints one line per chain and CU count; the test compares the output
// with tests/golden/gemm_plan_chain_edge.txt and checks the rule on every line. Lines:
//   <m>x<n> k<k of layer 0>,<k of layer 1>,.. br<batch of layer 0>,.. <f32|bf16> vf<0 flat|2|4> f<forced variant> sw<switch> et<forced tile, -1 none> st<strict> cus<CUs> :
//       v<variant the descriptor of layer 0 was planned on> gf<generic forced> kind<B image, -1 none> "<why not>" | tile<tile, -1 none> "<why not>"
// Left of the bar: what plan_gemm and chain_edge_b_kind say of the calls (every call of a chain, the first differing answer); right of
// it: plan_chain_edge's answer for the shape, whatever the left side says.
#include "gemm_plan.h"
#include <initializer_list>
#include <stdio.h>
#include <string.h>
#include <vector>

using namespace tpp;

namespace {

const int BM[4] = {32, 64, 64, 128}, BN[4] = {64, 64, 128, 128};

struct Chain {
  int64_t m, n;
  std::vector<int64_t> k, br;
  int et = -1;       // the tile xsmm_hip_set_edge_tiles(20 + et) names
  int vf = 2;        // B image: 0 flat, 2 VNNI-2, 4 VNNI-4
  int64_t dtype = DT_BF16;
  int forced = -1;   // xsmm_hip_force_variant at dispatch
  int sw = 1;        // xsmm_hip_set_chain_edge
  bool strict = false;
};

// layer l of the chain as the MLP dispatches it: A [m][br * k] row-major in k-wide batch elements, B [br * k][n] in its image, beta 0 + bias + relu
GemmDesc layer(const Chain &c, size_t l) {
  GemmDesc d;
  memset(&d, 0, sizeof(d));
  d.kind = KIND_GEMM;
  d.has_batch = 1;
  d.fused = 1;
  d.dtype = c.dtype;
  d.m = c.m, d.n = c.n, d.k = c.k[l];
  d.lda = c.k[l] * c.br[l], d.ldb = c.n, d.ldc = c.n;
  d.stride_a = c.k[l], d.stride_b = c.k[l] * c.n;
  d.beta0 = 1, d.bias = 1, d.relu = 1;
  if (c.dtype == DT_BF16) d.vnni_b = c.vf != 0, d.vnni_factor = c.vf;
  return d;
}

void line(const Chain &c, int cus) {
  GemmPlanEnv env{cus, c.strict, -1};
  int kind = -2, v0 = -1, gf0 = 0;
  const char *why = "";
  for (size_t l = 0; l < c.k.size(); ++l) {
    GemmDesc d = layer(c, l);
    if (!plan_gemm(d, c.forced, env)) {
      printf("%ldx%ld refused\n", (long)c.m, (long)c.n);
      return;
    }
    if (l == 0) v0 = d.variant, gf0 = d.generic_forced;
    const char *w = nullptr;
    const int kd = chain_edge_b_kind(d, c.sw, &w);
    if (kind == -2) kind = kd, why = w ? w : "";
    else if (kd != kind && kind >= 0) kind = -1, why = w ? w : "the calls' B operands differ in kind";
  }
  const ChainEdgePlan p = plan_chain_edge(c.m, c.n, (int)c.k.size(), c.k.data(), c.br.data(), cus, c.et, c.strict);
  printf("%ldx%ld k", (long)c.m, (long)c.n);
  for (size_t l = 0; l < c.k.size(); ++l) printf("%s%ld", l ? "," : "", (long)c.k[l]);
  printf(" br");
  for (size_t l = 0; l < c.br.size(); ++l) printf("%s%ld", l ? "," : "", (long)c.br[l]);
  printf(" %s vf%d f%d sw%d et%d st%d cus%d : v%d gf%d kind%d \"%s\" | tile%d \"%s\"\n", c.dtype == DT_F32 ? "f32" : "bf16", c.dtype == DT_F32 ? 0 : c.vf, c.forced,
         c.sw, c.et, (int)c.strict, cus, v0, gf0, kind, why, p.tile, p.why);
}
void both(const Chain &c) {
  for (int cus : {256, 64}) line(c, cus);
}
Chain mlp(int64_t m, int64_t n, int64_t k0 = 0, int64_t br0 = 1, int et = -1) {
  Chain c{m, n, {k0 ? k0 : n, n, n}, {br0, 1, 1}};
  c.et = et;
  return c;
}

} // namespace

int main() {
  // the GPU test's shapes: tile t forced, m = BM + 8 (two row blocks) and 3 BM - 3 (three), n = BN and 2 BN, layer 0 of 192 k; the three B images;
  // one chain per tile with two batch elements in every layer; the divisible neighbour m = 2 BM
  for (int t = 0; t < 4; ++t) {
    for (int64_t m : {BM[t] + 8, 3 * BM[t] - 3, 3 * BM[t] - 8})
      for (int64_t n : {BN[t], 2 * BN[t]})
        for (int vf : {2, 0, 4}) {
          Chain c = mlp(m, n, 192, 1, t);
          c.vf = vf;
          both(c);
        }
    Chain b{3 * BM[t] - 3, 2 * BN[t], {128, BN[t], BN[t]}, {2, 2, 2}};
    b.et = t;
    both(b);
    both(mlp(2 * BM[t], 2 * BN[t], 192, 1, t));
  }
  // the rows of the A/B and a rank's share of 4096 rows over 3 ranks: no tile forced, then each tile forced
  for (int64_t m : {1000, 4100, 1366, 2000, 1024, 4096})
    for (int et : {-1, 0, 1, 2, 3}) both(mlp(m, 1024, 0, 1, et));
  both(mlp(683, 1024)), both(mlp(4032, 1024));
  // refusals, one each (everything else as 1000 x 1024 x 3 layers)
  both(mlp(8200, 1024));                                   // too many tiles: 65 x 8 of the largest tile
  { Chain c = mlp(1000, 1024); c.strict = true; both(c); } // strict mode
  { Chain c = mlp(1000, 1024); c.sw = 0; both(c); }        // the switch off
  { Chain c = mlp(1000, 1024); c.forced = V_GENERIC; both(c); } // the generic kernel forced
  { Chain c = mlp(1024, 1024); c.forced = V_BF16_LW_64x64; both(c); c.m = 1000; both(c); } // a forced tile: honoured at 1024 rows (a forced kernel), not at 1000
  both(Chain{1000, 1000, {1024, 960, 960}, {1, 1, 1}}), both(Chain{1000, 1032, {1024, 1024, 1024}, {1, 1, 1}}); // ragged n (every k in whole chunks)
  both(mlp(1000, 1000));                                   // ... and the MLP of that width: its later layers' k is ragged as well
  both(mlp(24, 1024)), both(mlp(31, 64));                  // m below every tile's rows
  { Chain c = mlp(40, 1024, 0, 1, 1); both(c); }           // m below the forced tile's rows: the smallest tile that fits
  { Chain c = mlp(1000, 1024); c.dtype = DT_F32; both(c); } // f32
  { Chain c = mlp(1000, 1024, 1000); both(c); }             // a ragged k in layer 0
  { Chain c = mlp(1000, 1024, 1024, 0); both(c); }          // an empty batch
  { Chain c{1000, 1024, {1024}, {1}}; both(c); }            // one call
  { Chain c{1000, 1024, std::vector<int64_t>(9, 1024), std::vector<int64_t>(9, 1)}; both(c); } // nine calls
  { Chain c{1000, 1024, std::vector<int64_t>(8, 1024), std::vector<int64_t>(8, 1)}; both(c); } // eight
  return 0;
}
