// driver.cpp - TEST INFRASTRUCTURE for tests/test_gemm_plan_chain_widths_ragged.py, never part of the product library.
//
// Steps a fixed list of bf16 / f32 layer chains through the planner's ragged mixed-width rule (tpp-mlir_amd/csrc/gemm_plan.h
// plan_chain_widths_ragged, chain_widths_ragged_b_kind; xsmm_hip_set_chain_widths_ragged) the way rt_chain.h try_chain_launch asks it, and
// prints one line per chain and CU count; the test compares the output with tests/golden/gemm_plan_chain_widths_ragged.txt and checks the
// rule on every line. Lines:
//   <m> n<n of layer 0>,.. k<k of layer 0>,.. br<batch of layer 0>,.. <f32|bf16> vf<0 flat|2|4> f<forced variant, -1 none> sw<switch> et<forced edge tile, -1 none>
//       st<strict> x<1 beta 1 | 2 a VNNI C | 8 layer 1 has another B image> cus<CUs> : kind<B image, -1 none> "<why no image>" | tile<tile, -1 none> g<gated> "<why not>"
//       | widths tile<..> "<why not>"                       plan_chain_widths' answer on the same chain with its switch on (the partition)
//       and, on the equal-width chains: | edge tile<..> "<..>" | ragged tile<..> "<..>"
// kind: what try_chain_launch hands the rule - the B image every call has by chain_widths_ragged_b_kind, -1 when a call has none or they differ.
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
  int sw = 1;        // xsmm_hip_set_chain_widths_ragged
  int et = -1;       // the tile xsmm_hip_set_edge_tiles(20 + et) names
  bool strict = false;
  bool beta1 = false, vnni_c = false;
  int vf1 = -1;        // B image of layer 1, -1 = as layer 0
  int kind_given = -2; // >= 0: hand the rule this B image whatever the calls say (the rule's own terms)
  bool others = false; // print plan_chain_edge's and plan_chain_ragged's answers as well (equal-width chains)
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
  const char *kw = nullptr;
  int kind = chain_widths_ragged_b_kind(ds[0], c.sw, &kw);
  for (const GemmDesc &d : ds) {
    if (kind < 0) break;
    const char *w = nullptr;
    if (chain_widths_ragged_b_kind(d, c.sw, &w) != kind) kind = -1, kw = w ? w : "the calls' B operands differ in kind";
  }
  if (c.kind_given >= 0) kind = c.kind_given, kw = nullptr;
  const int L = (int)c.k.size();
  const ChainWidthsRaggedPlan p = plan_chain_widths_ragged(c.m, L, c.n.data(), c.k.data(), c.br.data(), cus, c.et, kind, c.sw, c.strict);
  printf("%ld", (long)c.m);
  list("n", c.n), list("k", c.k), list("br", c.br);
  printf(" %s vf%d f%d sw%d et%d st%d x%d cus%d : kind%d \"%s\" | tile%d g%d \"%s\"", c.dtype == DT_F32 ? "f32" : "bf16", c.dtype == DT_F32 ? 0 : c.vf, c.forced, c.sw, c.et, (int)c.strict,
         (c.beta1 ? 1 : 0) | (c.vnni_c ? 2 : 0) | (c.vf1 >= 0 ? 8 : 0), cus, kind, kw ? kw : "", p.tile, (int)p.gated, p.why);
  {
    // the partition: the mixed-width rule on the same chain, its switch on, no tile all calls were dispatched on
    const ChainWidthsPlan w = plan_chain_widths(c.m, L, c.n.data(), c.k.data(), c.br.data(), cus, -1, kind >= 0 ? kind : 0, 1, c.strict);
    printf(" | widths tile%d \"%s\"", w.tile, w.why);
  }
  if (c.others) {
    const ChainEdgePlan e = plan_chain_edge(c.m, c.n[0], L, c.k.data(), c.br.data(), cus, -1, c.strict);
    const ChainRaggedPlan g = plan_chain_ragged(c.m, c.n[0], L, c.k.data(), c.br.data(), cus, -1, kind >= 0 ? kind : 0, 1, c.strict);
    printf(" | edge tile%d \"%s\" | ragged tile%d \"%s\"", e.tile, e.why, g.tile, g.why);
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
// the GPU test's chains: layer 0 of k0, the later ones read their predecessor in br batch elements; the edge tile et forced
Chain gpu(int64_t m, std::vector<int64_t> ns, int64_t k0, int64_t br, int et, int vf) {
  Chain c{m, ns, {}, {}};
  for (size_t l = 0; l < ns.size(); ++l) c.k.push_back(l ? ns[l - 1] / br : k0), c.br.push_back(br);
  c.et = et, c.vf = vf;
  return c;
}

} // namespace

int main() {
  const int BM[4] = {32, 64, 64, 128}, BN[4] = {64, 64, 128, 128};
  // the rows of the A/B (as ShardedMlp dispatches them: layers[0] is the input's width) at 256, 64 and 304 compute units
  for (Chain c : {mlp(1024, {784, 512, 256, 128}), mlp(1000, {784, 512, 256, 128}), mlp(1000, {1024, 512, 256, 128}), mlp(512, {784, 256, 64, 256, 784}), mlp(1000, {1000, 500, 250}),
                  mlp(1000, {1000, 504, 248}), mlp(200, {200, 136, 72, 200}), mlp(1000, {1000, 2000, 1000})})
    at(c, {256, 64, 304});
  // ... two of them with the other B images, and the gated one with every tile forced
  for (int vf : {0, 4}) {
    Chain a = mlp(1000, {784, 512, 256, 128}), b = mlp(1000, {1000, 2000, 1000});
    a.vf = b.vf = vf;
    one(a), one(b);
  }
  for (int et = 0; et < 4; ++et) {
    Chain c = mlp(1000, {1000, 2000, 1000});
    c.et = et;
    one(c);
  }
  // the GPU test's chains: per tile t and image, the edge tile forced, m = BM + 8 and 3 BM - 3 (64x128 with VNNI-2 has no instance: passed over)
  for (int t = 0; t < 4; ++t)
    for (int vf : {2, 0, 4})
      for (int64_t m : {(int64_t)BM[t] + 8, (int64_t)3 * BM[t] - 3}) {
        const int64_t bn = BN[t];
        one(gpu(m, {3 * bn + 8, bn + 8, 2 * bn + 24}, 192, 1, t, vf)), one(gpu(m, {bn + 8, 3 * bn, bn + 16}, 128, 1, t, vf));
        one(gpu(m, {4 * bn, 2 * bn, bn}, 72, 1, t, vf)), one(gpu(m, {4 * bn, 2 * bn, bn}, 200, 1, t, vf));
        { Chain c = gpu(m, {2 * bn, bn}, 200, 1, t, vf); c.br[0] = 3; one(c); }
        one(gpu(m, {2 * bn + 8, bn + 8, 2 * bn + 8, bn + 8, 2 * bn + 8, bn + 8, 2 * bn + 8, bn + 8}, 136, 1, t, vf));
        { Chain c = gpu(m, {2 * bn + 16, 2 * bn + 16, bn + 8}, 144, 2, t, vf); one(c); }
        if (m == 3 * BM[t] - 3) one(gpu(m, {3 * bn, bn, 2 * bn}, 192, 1, t, vf));
      }
  // ... its MLPs under set_edge_tiles(21), with the switch on and off
  for (Chain c : {mlp(200, {200, 136, 72, 200}), mlp(96, {784, 256, 128, 64})}) {
    c.et = 1;
    one(c);
    c.sw = 0;
    one(c);
  }
  // strict mode: never
  { Chain c = mlp(1000, {784, 512, 256, 128}); c.strict = true; one(c); c.et = 0; one(c); }
  // THE PARTITION. A chain some tile divides entirely is the mixed-width rule's whatever its switch says, also with more tiles than compute units ..
  one(mlp(1024, {1024, 512, 256, 128})), one(mlp(1024, {1024, 4096, 1024})), one(mlp(16384, {1024, 512, 256, 128}));
  { Chain c = mlp(1024, {1024, 512, 256, 128}); c.et = 1; one(c); }
  // .. one that only a larger tile would leave ragged is divided by a smaller one: still the mixed-width rule's
  one(mlp(96, {128, 192, 64}));
  // .. and equal widths are the other three chain switches', with their rules' answers on the same chain
  for (Chain c : {mlp(1024, {1024, 1024, 1024, 1024}), mlp(1000, {1024, 1024, 1024, 1024}), mlp(1000, {1000, 1000, 1000, 1000}), mlp(200, {200, 200, 200, 200})}) {
    c.others = true;
    at(c, {256, 64});
  }
  // refusals, one each (everything else as 1000 rows x [784, 512, 256, 128])
  const std::vector<int64_t> F = {784, 512, 256, 128};
  { Chain c = mlp(1000, F); c.sw = 0; one(c); }                       // the switch off
  { Chain c = mlp(1000, F); c.dtype = DT_F32; one(c); }               // f32
  { Chain c = mlp(1000, F); c.beta1 = true; one(c); }                 // beta 1
  { Chain c = mlp(1000, F); c.vnni_c = true; one(c); }                // a VNNI C
  { Chain c = mlp(1000, F); c.forced = V_GENERIC; one(c); }           // the generic kernel, forced
  { Chain c = mlp(1024, F); c.forced = 21; one(c); }                  // another forced kernel
  { Chain c = mlp(1000, F); c.vf1 = 4; one(c); }                      // the calls' B images differ
  { Chain c = mlp(1000, F); c.br[0] = 0; c.kind_given = 0; one(c); }  // an empty batch
  { Chain c = mlp(1000, {780, 512, 256}); one(c); }                   // k % 8 == 4
  { Chain c = mlp(1000, {56, 512, 256}); one(c); }                    // k < 64
  { Chain c = mlp(1000, {780, 512, 256}); c.kind_given = 0; one(c); } // ... handed to the rule with an image all the same
  { Chain c = mlp(1000, {784, 512}); one(c); }                        // one call
  { Chain c = mlp(1000, {784, 512, 256, 512, 256, 512, 256, 512, 256, 512}); one(c); } // nine calls
  { Chain c = mlp(1000, {784, 512, 256, 512, 256, 512, 256, 512, 256}); one(c); }      // eight
  one(mlp(1000, {1000, 500, 250}));                                   // n % 8 != 0 (the calls have no image: their leading dimensions)
  { Chain c = mlp(1000, {1000, 500, 250}); c.kind_given = 0; one(c); } // ... handed to the rule all the same
  { Chain c = mlp(24, F); c.kind_given = 0; one(c); }                  // m below every tile
  { Chain c = mlp(1000, {784, 512, 256, 56}); c.kind_given = 0; one(c); } // an n below every tile
  one(mlp(4000, {784, 2048, 1024})), one(mlp(16000, F));               // more tiles than compute units (never several rounds)
  // a forced tile without an instance (64x128, VNNI-2): passed over for the smallest tile that fits; with the flat image it is taken
  { Chain c = mlp(200, {200, 264, 136}); c.et = 2; one(c); c.vf = 0; one(c); }
  // ... and where only 64x128 fits by the grid, VNNI-2 lands on 128x128 (gated without a forced tile: a layer fits 64x64 alone)
  { Chain c = mlp(1000, {1000, 2000, 1000}); c.vf = 0; c.et = 2; one(c); }
  return 0;
}
