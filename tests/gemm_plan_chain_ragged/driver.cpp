// driver.cpp - TEST INFRASTRUCTURE for tests/test_gemm_plan_chain_ragged.py, never part of the product library.
//
// Steps a fixed list of bf16 / f32 layer chains through the planner's ragged-width functions (tpp-mlir_amd/csrc/gemm_plan.h chain_ragged_b_kind,
// plan_chain_ragged; xsmm_hip_set_chain_ragged) and, on the same chains, through plan_chain_edge and plan_chain_rounds, and prints one line
// per chain and CU count; the test compares the output with tests/golden/gemm_plan_chain_ragged.txt and checks the rule on every line. Lines:
//   <m>x<n> k<k of layer 0>,.. br<batch of layer 0>,.. <f32|bf16> vf<0 flat|2|4> f<forced variant> sw<switch> ce<chain-edge switch> cr<chain-rounds switch>
//       et<forced tile, -1 none> st<strict> x<1 beta 1 | 2 a VNNI C | 4 ldb off the grid | 8 layer 1 has another B image> cus<CUs> : v<variant of layer 0>,<of layer 1> gf<generic forced> kind<B image, -1 none> "<why not>" | tile<tile, -1 none> "<why not>"
//       and, on the chains of the comparison group only: | edge kind<..> "<why not>" tile<..> "<why not>" | rounds pt<planned tile> tile<..> G<groups> R<rounds> g<gated> "<why not>"
// Left of the first bar: what plan_gemm and chain_ragged_b_kind say of the calls (the first differing answer); then plan_chain_ragged's answer
// for the shape with the calls' B image (that of layer 0 where they have none); then chain_edge_b_kind / plan_chain_edge and
// chain_rounds_planned_tile / plan_chain_rounds on the same chain, as tests/gemm_plan_chain_edge and tests/gemm_plan_chain_rounds print them.
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
  int sw = 1;        // xsmm_hip_set_chain_ragged
  int ce = 1, cr = 1; // xsmm_hip_set_chain_edge, xsmm_hip_set_chain_rounds
  bool strict = false;
  bool beta1 = false, vnni_c = false;
  int64_t ldb_off = 0; // added to ldb: an operand off the grid
  int vf1 = -1;        // B image of layer 1, -1 = as layer 0
  bool others = false; // print plan_chain_edge's and plan_chain_rounds' answers as well
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
  d.lda = c.k[l] * c.br[l], d.ldb = c.n + c.ldb_off, d.ldc = c.n;
  d.stride_a = c.k[l], d.stride_b = c.k[l] * c.n;
  d.beta0 = !c.beta1, d.bias = 1, d.relu = 1;
  d.vnni_c = c.vnni_c;
  const int vf = l == 1 && c.vf1 >= 0 ? c.vf1 : c.vf;
  if (c.dtype == DT_BF16) d.vnni_b = vf != 0, d.vnni_factor = vf;
  return d;
}

void line(const Chain &c, int cus) {
  GemmPlanEnv env{cus, c.strict, -1};
  int kind = -2, ekind = -2, kind0 = -1;
  const char *why = "", *ewhy = "";
  std::vector<GemmDesc> ds;
  for (size_t l = 0; l < c.k.size(); ++l) {
    GemmDesc d = layer(c, l);
    if (!plan_gemm(d, c.forced, env)) {
      printf("%ldx%ld refused\n", (long)c.m, (long)c.n);
      return;
    }
    ds.push_back(d);
    const char *w = nullptr;
    const int kd = chain_ragged_b_kind(d, c.sw, &w);
    if (l == 0) kind0 = kd;
    if (kind == -2) kind = kd, why = w ? w : "";
    else if (kd != kind && kind >= 0) kind = -1, why = w ? w : "the calls' B operands differ in kind";
    const int ek = chain_edge_b_kind(d, c.ce, &w);
    if (ekind == -2) ekind = ek, ewhy = w ? w : "";
    else if (ek != ekind && ekind >= 0) ekind = -1, ewhy = w ? w : "the calls' B operands differ in kind";
  }
  std::vector<const GemmDesc *> dp;
  for (const GemmDesc &d : ds) dp.push_back(&d);
  const int image = kind >= 0 ? kind : kind0 >= 0 ? kind0 : c.vf == 2 ? 0 : c.vf == 0 ? 2 : 4;
  const ChainRaggedPlan p = plan_chain_ragged(c.m, c.n, (int)c.k.size(), c.k.data(), c.br.data(), cus, c.et, kind < 0 && kind0 >= 0 && c.vf1 >= 0 ? -1 : image, c.sw, c.strict);
  const ChainEdgePlan e = plan_chain_edge(c.m, c.n, (int)c.k.size(), c.k.data(), c.br.data(), cus, c.et, c.strict);
  const int pt = chain_rounds_planned_tile((int)dp.size(), dp.data());
  const ChainRoundsPlan r = plan_chain_rounds(c.m, c.n, (int)c.k.size(), c.k.data(), c.br.data(), cus, pt, c.cr, c.strict);
  const int rounds = r.tile >= 0 ? (int)((c.m / BM[r.tile] + r.groups - 1) / r.groups) : 0;
  printf("%ldx%ld k", (long)c.m, (long)c.n);
  for (size_t l = 0; l < c.k.size(); ++l) printf("%s%ld", l ? "," : "", (long)c.k[l]);
  printf(" br");
  for (size_t l = 0; l < c.br.size(); ++l) printf("%s%ld", l ? "," : "", (long)c.br[l]);
  printf(" %s vf%d f%d sw%d ce%d cr%d et%d st%d x%d cus%d : v%d,%d gf%d kind%d \"%s\" | tile%d \"%s\"",
         c.dtype == DT_F32 ? "f32" : "bf16", c.dtype == DT_F32 ? 0 : c.vf, c.forced, c.sw, c.ce, c.cr, c.et, (int)c.strict, (c.beta1 ? 1 : 0) | (c.vnni_c ? 2 : 0) | (c.ldb_off ? 4 : 0) | (c.vf1 >= 0 ? 8 : 0), cus, ds[0].variant,
         ds.size() > 1 ? ds[1].variant : -1, (int)ds[0].generic_forced, kind, why, p.tile, p.why);
  if (c.others) printf(" | edge kind%d \"%s\" tile%d \"%s\" | rounds pt%d tile%d G%d R%d g%d \"%s\"", ekind, ewhy, e.tile, e.why, pt, r.tile, r.groups, rounds, (int)r.gated, r.why);
  printf("\n");
}
void at(const Chain &c, std::initializer_list<int> cus) {
  for (int n : cus) line(c, n);
}
void one(const Chain &c) { line(c, 256); }
Chain mlp(int64_t m, int64_t n, int64_t k0 = 0, int64_t br0 = 1, int et = -1) {
  Chain c{m, n, {k0 ? k0 : n, n, n}, {br0, 1, 1}};
  c.et = et;
  return c;
}

} // namespace

int main() {
  // per tile t, forced: m around BM (n = BN + 8, layer 0 of 72), n in {BN, BN + 4, 2 BN + 24, 1000} (m = BM + 8, layer 0 of 80), and a whole-k layer 0
  // (128) with the ragged n = BN + 8 and with n = BN (nothing ragged in width); the later layers have k = n
  for (int t = 0; t < 4; ++t) {
    for (int64_t m : {BM[t] - 8, BM[t], BM[t] + 8, 3 * BM[t] - 3}) one(mlp(m, BN[t] + 8, 72, 1, t));
    for (int64_t n : {(int64_t)BN[t], (int64_t)BN[t] + 4, 2 * (int64_t)BN[t] + 24, (int64_t)1000}) one(mlp(BM[t] + 8, n, 80, 1, t));
    one(mlp(BM[t] + 8, BN[t] + 8, 128, 1, t)), one(mlp(BM[t] + 8, BN[t], 128, 1, t));
  }
  // the GPU test's other chains on the 64x64 tile, the three B images: n = BN + 16, three batch elements of 200, two batch elements per layer, four
  // layers; 64x128 forced for a VNNI-2 chain (no such instance: the smallest tile that fits); 192 columns on the 128x128 tile
  for (int vf : {2, 0, 4}) {
    Chain a = mlp(72, 80, 104, 1, 1), b = mlp(189, 72, 200, 3, 1), c{189, 144, {112, 72, 72}, {2, 2, 2}}, d{72, 72, {128, 72, 72, 72}, {1, 1, 1, 1}};
    c.et = d.et = 1;
    for (Chain *x : {&a, &b, &c, &d}) x->vf = vf, one(*x);
  }
  one(mlp(189, 136, 200, 1, 2)), one(mlp(136, 192, 120, 1, 3));
  // the rows of the A/B at 256, 64 and 304 compute units; forced tiles; the other B images at 2000 rows (64x128 exists for them)
  for (int64_t m : {1000, 1024, 2000, 4096}) at(mlp(m, 1000), {256, 64, 304});
  for (int et : {0, 3}) one(mlp(1000, 1000, 0, 1, et)), one(mlp(2000, 1000, 0, 1, et));
  one(mlp(1024, 1000, 784)), one(mlp(1024, 1000, 64, 16)), one(mlp(200, 200)), one(mlp(200, 200, 784));
  { Chain c = mlp(2000, 1000); c.vf = 0; one(c); c.vf = 4; one(c); }
  // lines of tests/golden/gemm_plan_chain_edge.txt and _rounds.txt with this switch off and on: their answers are the parent's. A divisible
  // chain, chains ragged in m alone, in n, in k; more tiles than compute units; the other two switches off as well
  for (int sw : {0, 1}) {
    for (Chain c : {mlp(1024, 1024), mlp(1000, 1024), mlp(1000, 1000), Chain{1000, 1032, {1024, 1024, 1024}, {1, 1, 1}}, mlp(4224, 1024), mlp(8192, 1024)}) {
      c.sw = sw, c.others = true;
      at(c, {256, 64});
    }
    { Chain c = mlp(1000, 1024); c.sw = sw, c.ce = c.cr = 0, c.others = true; one(c); }
  }
  // refusals, one each (everything else as 1000 x 1000 x 3 layers)
  { Chain c = mlp(1000, 1000); c.strict = true; one(c); }           // strict mode
  { Chain c = mlp(1000, 1000); c.dtype = DT_F32; one(c); }          // f32
  { Chain c = mlp(1000, 1000); c.beta1 = true; one(c); }            // beta 1
  { Chain c = mlp(1000, 1000); c.vnni_c = true; one(c); }           // a VNNI C
  { Chain c = mlp(1000, 1000); c.forced = V_GENERIC; one(c); }      // the generic kernel forced
  { Chain c = mlp(1000, 1000, 76); one(c); c.k[0] = 56; one(c); }   // k % 8 == 4, k < 64
  { Chain c = mlp(1000, 1000); c.ldb_off = 2; one(c); }             // an operand off the grid
  { Chain c = mlp(1000, 1000); c.vf1 = 4; one(c); }                 // the calls' B images differ
  { Chain c = mlp(1000, 1000, 1000, 0); one(c); }                   // an empty batch
  { Chain c = mlp(1000, 1004, 1000); c.k[1] = c.k[2] = 1000; one(c); } // n % 8 != 0
  one(mlp(24, 1000)), one(mlp(1000, 56, 1000)), one(mlp(40, 1000, 0, 1, 1)); // m / n below every tile; m below the forced tile: the smallest that fits
  one(mlp(8200, 1000)), one(mlp(4100, 1000));                       // more tiles than compute units (never several rounds)
  { Chain c{1000, 1000, {1000}, {1}}; one(c); }                     // one call
  { Chain c{1000, 1000, std::vector<int64_t>(9, 1000), std::vector<int64_t>(9, 1)}; one(c); } // nine calls
  { Chain c{1000, 1000, std::vector<int64_t>(8, 1000), std::vector<int64_t>(8, 1)}; one(c); } // eight
  return 0;
}
