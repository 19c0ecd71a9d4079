// driver.cpp - TEST INFRASTRUCTURE for tests/test_gemm_plan_chain_rounds.py, never part of the product library.
//
// Steps a fixed list of bf16 / f32 layer chains through the planner's multi-round rule (tpp-mlir_amd/csrc/gemm_plan.h
// chain_rounds_planned_tile, plan_chain_rounds; xsmm_hip_set_chain_rounds) and prints one line per chain and CU count; the test compares the
// output with tests/golden/gemm_plan_chain_rounds.txt and checks the rule on every line. Lines:
//   <m>x<n> k<k of layer 0>,.. br<batch of layer 0>,.. <f32|bf16> vf<0 flat|2|4> f<forced variant of layer 0>,<.. of the others> sw<switch> st<strict> cus<CUs> :
//       v<variant of layer 0>,<.. of layer 1> pt<tile all calls were planned on, -1 none, -2 not bf16> | tile<tile, -1 none> G<groups> R<rounds> g<gated> "<why not>"
// (a gated line names the tile, groups and rounds the rule gives and the gate that keeps the chain call by call)
#include "gemm_plan.h"
#include <initializer_list>
#include <stdio.h>
#include <string.h>
#include <vector>

using namespace tpp;

namespace {

const int BM[4] = {32, 64, 64, 128}, BN[4] = {64, 64, 128, 128}, NSLOT[4] = {8, 8, 6, 4};
const int BASE[5] = {V_BF16_LWF_32x64, 0, V_BF16_LW_32x64, 0, V_BF16_LW4_32x64}; // B image -> variant of its 32x64 + K2 tile

struct Chain {
  int64_t m, n;
  std::vector<int64_t> k, br;
  int sw = 1;        // xsmm_hip_set_chain_rounds
  int vf = 2;        // B image: 0 flat, 2 VNNI-2, 4 VNNI-4
  int64_t dtype = DT_BF16;
  int forced0 = -1, forced = -1; // xsmm_hip_force_variant at the dispatch of layer 0 / of the later layers
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
  std::vector<GemmDesc> ds;
  for (size_t l = 0; l < c.k.size(); ++l) {
    GemmDesc d = layer(c, l);
    if (!plan_gemm(d, l == 0 ? c.forced0 : c.forced, env)) {
      printf("%ldx%ld refused\n", (long)c.m, (long)c.n);
      return;
    }
    ds.push_back(d);
  }
  std::vector<const GemmDesc *> dp;
  for (const GemmDesc &d : ds) dp.push_back(&d);
  const int pt = chain_rounds_planned_tile((int)dp.size(), dp.data());
  const ChainRoundsPlan p = plan_chain_rounds(c.m, c.n, (int)c.k.size(), c.k.data(), c.br.data(), cus, pt, c.sw, c.strict);
  int rounds = 0;
  if (p.tile >= 0) rounds = (int)((c.m / BM[p.tile] + p.groups - 1) / p.groups);
  printf("%ldx%ld k", (long)c.m, (long)c.n);
  for (size_t l = 0; l < c.k.size(); ++l) printf("%s%ld", l ? "," : "", (long)c.k[l]);
  printf(" br");
  for (size_t l = 0; l < c.br.size(); ++l) printf("%s%ld", l ? "," : "", (long)c.br[l]);
  printf(" %s vf%d f%d,%d sw%d st%d cus%d : v%d,%d pt%d | tile%d G%d R%d g%d \"%s\"\n", c.dtype == DT_F32 ? "f32" : "bf16", c.dtype == DT_F32 ? 0 : c.vf, c.forced0, c.forced,
         c.sw, (int)c.strict, cus, ds[0].variant, ds.size() > 1 ? ds[1].variant : -1, pt, p.tile, p.groups, rounds, (int)p.gated, p.why);
}
void both(const Chain &c) {
  for (int cus : {256, 64}) line(c, cus);
}
Chain mlp(int64_t m, int64_t n = 1024, int sw = 1) {
  Chain c{m, n, {n, n, n}, {1, 1, 1}};
  c.sw = sw;
  return c;
}
Chain forced(Chain c, int t, int vf = 2) {
  c.vf = vf;
  c.forced0 = c.forced = BASE[vf] + t;
  return c;
}

} // namespace

int main() {
  // the GPU test's shapes: tile t forced at dispatch, mode 1000 + G; the three B images
  for (int t = 0; t < 4; ++t)
    for (int vf : {2, 0, 4}) {
      const int64_t bm = BM[t], bn = BN[t], ns = 64 * NSLOT[t];
      both(forced(Chain{5 * bm, 2 * bn, {192, 2 * bn, 2 * bn}, {1, 1, 1}, 1002}, t, vf)); // uneven: groups own 3 and 2 blocks
      both(forced(Chain{4 * bm, bn, {192, bn, bn}, {1, 1, 1}, 1002}, t, vf));             // even
      both(forced(Chain{3 * bm, 2 * bn, {192, 2 * bn, 2 * bn}, {1, 1, 1}, 1001}, t, vf)); // one group walks every block
      both(forced(Chain{3 * bm, ns, {ns, ns, ns}, {1, 1, 1}, 1002}, t, vf));              // NSLOT chunks per layer: the B loaders run ahead across steps
      both(forced(Chain{5 * bm, 2 * bn, {128, bn, bn}, {2, 2, 2}, 1002}, t, vf));         // two batch elements per layer
      both(forced(Chain{3 * bm, 2 * bn, {192, 2 * bn, 2 * bn}, {1, 1, 1}, 1003}, t, vf)); // a forced G >= tiles_m
      both(forced(Chain{3 * bm, 2 * bn, {192, 2 * bn, 2 * bn}, {1, 1, 1}, 1}, t, vf));    // a chain that fits, under mode 1
    }
  // mode 1 on a real overflow: tile 0 forced, n = 64, m = 32 x (CUs + 8), k = 64 (the GPU test reads the CU count from the device)
  for (int cus : {256, 64, 304}) line(forced(Chain{32 * (cus + 8), 64, {64, 64, 64}, {1, 1, 1}, 1}, 0), cus);
  { Chain c = forced(Chain{32 * (256 + 8), 64, {64, 64, 64}, {1, 1, 1}, 1}, 0); c.strict = true; both(c); } // .. and in strict mode: the planned tile
  // three 1024-wide layers (the rows of the A/B, the divisible 1024 and 4096, one more row of tiles than the CUs hold), as planned
  for (int64_t m : {4224, 8192, 16384, 32768, 4096, 1024, 4352, 12288})
    for (int sw : {1, 0}) both(mlp(m, 1024, sw));
  both(mlp(8192, 1024, 1016)), both(mlp(8192, 1024, 1032)), both(mlp(8192, 1024, 1033)), both(mlp(8192, 1024, 1063)), both(mlp(8192, 1024, 1064)); // forced G: 16, 32, 33 (too many), tiles_m - 1, tiles_m
  both(mlp(4096, 1024, 1016)); // a forced G on a chain that fits in one round
  { Chain c = mlp(8192); c.vf = 0; both(c); c.vf = 4; both(c); } // the other B images
  // refusals, one each (everything else as 8192 x 1024 x 3 layers; the switch off is above)
  { Chain c = mlp(8192); c.strict = true; both(c); }                                  // strict mode, one shared tile: taken
  { Chain c = mlp(8192); c.forced0 = V_BF16_LW_64x64; both(c); c.strict = true; both(c); } // mixed tiles: the largest dividing tile; refused in strict mode
  both(mlp(8200)), both(mlp(4100));                                                   // a ragged m
  both(Chain{8192, 1032, {1024, 1024, 1024}, {1, 1, 1}}), both(Chain{8192, 1000, {1024, 960, 960}, {1, 1, 1}}); // a ragged n (every k in whole chunks)
  { Chain c = mlp(8192); c.k[0] = 1000; both(c); c.k[0] = 1056; both(c); }            // a k % 64 in layer 0
  { Chain c = mlp(8192); c.dtype = DT_F32; both(c); }                                 // f32
  { Chain c = mlp(8192); c.br[0] = 0; both(c); }                                      // an empty batch
  { Chain c{8192, 1024, {1024}, {1}}; both(c); }                                      // one call
  { Chain c{8192, 1024, std::vector<int64_t>(9, 1024), std::vector<int64_t>(9, 1)}; both(c); } // nine calls
  { Chain c{8192, 1024, std::vector<int64_t>(8, 1024), std::vector<int64_t>(8, 1)}; both(c); } // eight
  both(mlp(8192, 65536 / 2)), both(mlp(256, 16384 + 8192));                           // a row of tiles wider than the compute units (at 64)
  return 0;
}
