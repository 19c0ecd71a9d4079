// driver.cpp - TEST INFRASTRUCTURE for tests/test_gemm_plan_chain_widths.py, never part of the product library.
//
// Steps a fixed list of bf16 / f32 layer chains through the planner's mixed-width rule (tpp-mlir_amd/csrc/gemm_plan.h plan_chain_widths;
// xsmm_hip_set_chain_widths) the way rt_chain.h try_chain_launch asks it, and prints one line per chain and CU count; the test compares the
// output with tests/golden/gemm_plan_chain_widths.txt and checks the rule on every line. Lines:
//   <m> n<n of layer 0>,.. k<k of layer 0>,.. br<batch of layer 0>,.. <f32|bf16> vf<0 flat|2|4> f<forced variant, -1 none> sw<switch> st<strict>
//       x<1 beta 1 | 2 a VNNI C | 8 layer 1 has another B image> cus<CUs> : v<variant of layer 0>,<of layer 1> pt<planned tile> kind<B image, -1 none> | tile<tile, -1 none> "<why not>"
//       and, on the equal-width chains of the comparison group: | edge tile<..> "<why not>" | rounds tile<..> G<groups> g<gated> "<why not>" | ragged tile<..> "<why not>"
// kind: what try_chain_launch hands the rule - the B image every call has by bf16_lw_b_kind, -1 when a call has none, is not bf16 / beta 0,
// stores a VNNI C, went to the generic kernel, or the images differ.
#include "gemm_plan.h"
#include <initializer_list>
#include <stdio.h>
#include <string.h>
#include <vector>

using namespace tpp;

namespace {

struct Chain {
  int64_t m;
  std::vector<int64_t> n, k, br;
  int vf = 2;        // B image: 0 flat, 2 VNNI-2, 4 VNNI-4
  int64_t dtype = DT_BF16;
  int forced = -1;   // xsmm_hip_force_variant at dispatch
  int sw = 1;        // xsmm_hip_set_chain_widths
  bool strict = false;
  bool beta1 = false, vnni_c = false;
  int vf1 = -1;        // B image of layer 1, -1 = as layer 0
  int kind_given = -2; // >= 0: hand the rule this B image whatever the calls say (the rule's own m and n terms: no call with such a shape has one)
  bool others = false; // print plan_chain_edge's, plan_chain_rounds' and plan_chain_ragged's answers as well (equal-width chains)
};

// layer l of the chain as the MLP dispatches it: A [m][br * k] row-major in k-wide batch elements, B [br * k][n] in its image, beta 0 + bias + relu
GemmDesc layer(const Chain &c, size_t l) {
  GemmDesc d;
  memset(&d, 0, sizeof(d));
  d.kind = KIND_GEMM;
  d.has_batch = 1;
  d.fused = 1;
  d.dtype = c.dtype;
  d.m = c.m, d.n = c.n[l], d.k = c.k[l];
  d.lda = c.k[l] * c.br[l], d.ldb = c.n[l], d.ldc = c.n[l];
  d.stride_a = c.k[l], d.stride_b = c.k[l] * c.n[l];
  d.beta0 = !c.beta1, d.bias = 1, d.relu = 1;
  d.vnni_c = c.vnni_c;
  const int vf = l == 1 && c.vf1 >= 0 ? c.vf1 : c.vf;
  if (c.dtype == DT_BF16) d.vnni_b = vf != 0, d.vnni_factor = vf;
  return d;
}

void list(const char *tag, const std::vector<int64_t> &v) {
  printf(" %s", tag);
  for (size_t l = 0; l < v.size(); ++l) printf("%s%ld", l ? "," : "", (long)v[l]);
}

void line(const Chain &c, int cus) {
  GemmPlanEnv env{cus, c.strict, -1};
  std::vector<GemmDesc> ds;
  for (size_t l = 0; l < c.k.size(); ++l) {
    GemmDesc d = layer(c, l);
    if (!plan_gemm(d, c.forced, env)) {
      printf("%ld refused\n", (long)c.m);
      return;
    }
    ds.push_back(d);
  }
  std::vector<const GemmDesc *> dp;
  for (const GemmDesc &d : ds) dp.push_back(&d);
  int kind = c.dtype == DT_BF16 ? bf16_lw_b_kind(ds[0]) : -1;
  for (const GemmDesc &d : ds)
    if (d.dtype != DT_BF16 || d.vnni_c || !d.beta0 || d.variant == V_GENERIC || bf16_lw_b_kind(d) != kind) kind = -1;
  if (c.kind_given >= 0) kind = c.kind_given;
  const int pt = chain_rounds_planned_tile((int)dp.size(), dp.data());
  const int L = (int)c.k.size();
  const ChainWidthsPlan p = plan_chain_widths(c.m, L, c.n.data(), c.k.data(), c.br.data(), cus, pt, kind, c.sw, c.strict);
  printf("%ld", (long)c.m);
  list("n", c.n), list("k", c.k), list("br", c.br);
  printf(" %s vf%d f%d sw%d st%d x%d cus%d : v%d,%d pt%d kind%d | tile%d \"%s\"", c.dtype == DT_F32 ? "f32" : "bf16", c.dtype == DT_F32 ? 0 : c.vf, c.forced, c.sw, (int)c.strict,
         (c.beta1 ? 1 : 0) | (c.vnni_c ? 2 : 0) | (c.vf1 >= 0 ? 8 : 0), cus, ds[0].variant, ds.size() > 1 ? ds[1].variant : -1, pt, kind, p.tile, p.why);
  if (c.others) {
    const ChainEdgePlan e = plan_chain_edge(c.m, c.n[0], L, c.k.data(), c.br.data(), cus, -1, c.strict);
    const ChainRoundsPlan r = plan_chain_rounds(c.m, c.n[0], L, c.k.data(), c.br.data(), cus, pt, 1, c.strict);
    const ChainRaggedPlan g = plan_chain_ragged(c.m, c.n[0], L, c.k.data(), c.br.data(), cus, -1, kind >= 0 ? kind : 0, 1, c.strict);
    printf(" | edge tile%d \"%s\" | rounds tile%d G%d g%d \"%s\" | ragged tile%d \"%s\"", e.tile, e.why, r.tile, r.groups, (int)r.gated, r.why, g.tile, g.why);
  }
  printf("\n");
}
void at(const Chain &c, std::initializer_list<int> cus) {
  for (int n : cus) line(c, n);
}
void one(const Chain &c) { line(c, 256); }
// an MLP of these layer widths on m rows: layers[0] is the input's width; every layer one batch element of its predecessor's width
Chain mlp(int64_t m, std::vector<int64_t> layers) {
  Chain c{m, {}, {}, {}};
  for (size_t l = 1; l < layers.size(); ++l) c.n.push_back(layers[l]), c.k.push_back(layers[l - 1]), c.br.push_back(1);
  return c;
}
// the GPU test's chains: layer 0 of k0, the later ones read their predecessor in br batch elements
Chain gpu(int64_t m, std::vector<int64_t> ns, int64_t k0, int64_t br, int forced, int vf) {
  Chain c{m, ns, {}, {}};
  for (size_t l = 0; l < ns.size(); ++l) c.k.push_back(l ? ns[l - 1] / br : k0), c.br.push_back(br);
  c.forced = forced, c.vf = vf;
  return c;
}

} // namespace

int main() {
  const int BM[4] = {32, 64, 64, 128}, BN[4] = {64, 64, 128, 128}, BASE[5] = {24, 0, 20, 0, 28}; // (BASE[vf]: the variant of the image's 32x64 tile)
  // the rows of the A/B (as ShardedMlp dispatches them: layers[0] is the input's width) at 256, 64 and 304 compute units, two of them with the other B images
  at(mlp(1024, {1024, 4096, 1024}), {256, 64, 304}), at(mlp(256, {1024, 4096, 1024}), {256, 64, 304}), at(mlp(2048, {1024, 2048, 1024}), {256, 64, 304});
  at(mlp(1024, {1024, 512, 256, 128}), {256, 64, 304}), at(mlp(1024, {1024, 2048, 1024, 2048, 1024}), {256, 64, 304});
  for (int vf : {0, 4}) {
    Chain a = mlp(1024, {1024, 4096, 1024}), b = mlp(1024, {1024, 512, 256, 128});
    a.vf = b.vf = vf;
    one(a), one(b);
  }
  // the GPU test's chains: per tile t and image, every call forced to the tile's variant, m = 2 BM
  for (int t = 0; t < 4; ++t)
    for (int vf : {2, 0, 4}) {
      const int64_t bn = BN[t], m = 2 * BM[t];
      const int f = BASE[vf] + t;
      one(gpu(m, {3 * bn, bn, 2 * bn}, 192, 1, f, vf)), one(gpu(m, {bn, 3 * bn, bn}, 192, 1, f, vf)), one(gpu(m, {4 * bn, 2 * bn, bn}, 192, 1, f, vf));
      one(gpu(m, {2 * bn, bn, 2 * bn, bn, 2 * bn, bn, 2 * bn, bn}, 192, 1, f, vf));
      { Chain c = gpu(m, {2 * bn, 2 * bn, bn}, 192, 2, f, vf); c.k[0] = 192; one(c); }
      one(gpu(m, {256, 128, 256}, 128, 1, f, vf));
      { Chain c = gpu(m, {2 * bn, bn}, 256, 1, f, vf); c.br[0] = 3; one(c); }
      one(gpu(m, {3 * bn, bn, 3 * bn}, 192, 1, f, vf)), one(gpu(m, {bn, 3 * bn, 3 * bn}, 192, 1, f, vf));
    }
  // ... its MLP (force_variant(21)) with the switch on and off, and the same without a forced tile (gated: 128-wide layer fits 32x64 alone)
  { Chain c = mlp(256, {256, 512, 128, 256}); c.forced = 21; one(c); c.sw = 0; one(c); c.sw = 1, c.forced = -1; one(c); }
  // strict mode: on the tile all calls were dispatched on; without one, refused
  { Chain c = gpu(128, {192, 64, 128}, 192, 1, 21, 2); c.strict = true; one(c); c.forced = -1; one(c); }
  // equal widths (the plain chain's), with the other chain rules' answers on the same chain: lines of their golden tables
  for (int sw : {0, 1})
    for (Chain c : {mlp(1024, {1024, 1024, 1024, 1024}), mlp(1000, {1024, 1024, 1024, 1024}), mlp(1000, {1000, 1000, 1000, 1000}), mlp(4224, {1024, 1024, 1024, 1024}), mlp(8192, {1024, 1024, 1024, 1024})}) {
      c.sw = sw, c.others = true;
      at(c, {256, 64});
    }
  // refusals, one each (everything else as 1024 rows x [1024, 512, 256, 128])
  const std::vector<int64_t> F = {1024, 512, 256, 128};
  { Chain c = mlp(1024, F); c.sw = 0; one(c); }                       // the switch off
  { Chain c = mlp(1024, F); c.dtype = DT_F32; one(c); }               // f32
  { Chain c = mlp(1024, F); c.beta1 = true; one(c); }                 // beta 1
  { Chain c = mlp(1024, F); c.vnni_c = true; one(c); }                // a VNNI C
  { Chain c = mlp(1024, F); c.forced = V_GENERIC; one(c); }           // the generic kernel
  { Chain c = mlp(1024, F); c.vf1 = 4; one(c); }                      // the calls' B images differ
  { Chain c = mlp(1024, F); c.br[0] = 0; one(c); }                    // an empty batch
  { Chain c = mlp(1024, {200, 512, 256}); one(c); }                   // a k of 200
  { Chain c = mlp(1024, {1024, 512}); one(c); }                       // one call
  { Chain c = mlp(1024, {1024, 512, 256, 512, 256, 512, 256, 512, 256, 512}); one(c); } // nine calls
  { Chain c = mlp(1024, {1024, 512, 256, 512, 256, 512, 256, 512, 256}); one(c); }     // eight
  one(mlp(1000, F)), one(mlp(1024, {1024, 512, 96, 128})), one(mlp(1024, {1024, 1000, 512})); // a ragged m, an n no tile divides, a ragged n
  { Chain c = mlp(1000, F); c.kind_given = 0; one(c); }               // ... handed to the rule with an image all the same: no tile divides m
  { Chain c = mlp(1024, {1024, 512, 96, 128}); c.kind_given = 0; one(c); } // ... or every n
  one(mlp(4096, {1024, 2048, 1024})), one(mlp(8192, F));             // more tiles than compute units (never several rounds)
  return 0;
}
