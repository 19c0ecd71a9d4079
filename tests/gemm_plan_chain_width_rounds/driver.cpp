// driver.cpp - TEST INFRASTRUCTURE for tests/test_gemm_plan_chain_width_rounds.py, never part of the product library.
//
// Steps a fixed list of bf16 / f32 layer chains through the planner's column-round rule (tpp-mlir_amd/csrc/gemm_plan.h plan_chain_width_rounds;
// xsmm_hip_set_chain_width_rounds) the way rt_chain.h try_chain_launch asks it, and prints one line per chain and CU count; the test compares
// the output with tests/golden/gemm_plan_chain_width_rounds.txt and checks the rule on every line. Lines:
//   <m> n<n of layer 0>,.. k<k of layer 0>,.. br<batch of layer 0>,.. <f32|bf16> vf<0 flat|2|4> f<forced variant, -1 none> sw<switch> cw<xsmm_hip_set_chain_widths> st<strict>
//       x<1 beta 1 | 2 a VNNI C | 8 layer 1 has another B image> cus<CUs> : pt<planned tile> kind<B image, -1 none> | tile<tile, -1 none> W<groups> g<gated> "<why not>"
//       | widths tile<plan_chain_widths' tile> | <launch: rounds, widths or none>
// kind: what try_chain_launch hands the rule - the B image every call has by bf16_lw_b_kind, -1 when a call has none, is not bf16 / beta 0,
// stores a VNNI C, went to the generic kernel, or the images differ. launch: which of the two rules try_chain_launch's order of asking ends
// in - a forced W in front of plan_chain_widths, the rule behind it.
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
  int sw = 1;        // xsmm_hip_set_chain_width_rounds
  int cw = 0;        // xsmm_hip_set_chain_widths
  bool strict = false;
  bool beta1 = false, vnni_c = false;
  int vf1 = -1;        // B image of layer 1, -1 = as layer 0
  int kind_given = -2; // >= 0: hand the rule this B image whatever the calls say (the rule's own m and n terms: no call with such a shape has one)
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
  const ChainWidthRoundsPlan p = plan_chain_width_rounds(c.m, L, c.n.data(), c.k.data(), c.br.data(), cus, pt, kind, c.sw, c.strict);
  const ChainWidthsPlan w = plan_chain_widths(c.m, L, c.n.data(), c.k.data(), c.br.data(), cus, pt, kind, c.cw, c.strict);
  // try_chain_launch's order: a forced W, then the one-round rule, then this rule (never on a gated answer)
  const bool mine = p.tile >= 0 && !p.gated;
  const char *launch = chain_width_rounds_mode_forced(c.sw) && mine ? "rounds" : w.tile >= 0 ? "widths" : mine ? "rounds" : "none";
  printf("%ld", (long)c.m);
  list("n", c.n), list("k", c.k), list("br", c.br);
  printf(" %s vf%d f%d sw%d cw%d st%d x%d cus%d : pt%d kind%d | tile%d W%d g%d \"%s\" | widths tile%d | %s\n", c.dtype == DT_F32 ? "f32" : "bf16", c.dtype == DT_F32 ? 0 : c.vf, c.forced, c.sw, c.cw,
         (int)c.strict, (c.beta1 ? 1 : 0) | (c.vnni_c ? 2 : 0) | (c.vf1 >= 0 ? 8 : 0), cus, pt, kind, p.tile, p.groups, (int)p.gated, p.why, w.tile, launch);
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
Chain gpu(int64_t m, std::vector<int64_t> ns, int64_t k0, int64_t br, int forced, int vf, int w) {
  Chain c{m, ns, {}, {}};
  for (size_t l = 0; l < ns.size(); ++l) c.k.push_back(l ? ns[l - 1] / br : k0), c.br.push_back(br);
  c.forced = forced, c.vf = vf, c.sw = 1000 + w;
  return c;
}

} // namespace

int main() {
  const int BM[4] = {32, 64, 64, 128}, BN[4] = {64, 64, 128, 128}, BASE[5] = {24, 0, 20, 0, 28}; // (BASE[vf]: the variant of the image's 32x64 tile)
  // the rows of the A/B (as ShardedMlp dispatches them: layers[0] is the input's width) at 256, 64 and 304 compute units, with the one-round switch off and on
  for (int cw : {0, 1})
    for (int64_t m : {256, 1024, 2048, 4096}) {
      Chain c = mlp(m, {1024, 4096, 1024});
      c.cw = cw;
      at(c, {256, 64, 304});
    }
  for (int cw : {0, 1}) {
    Chain a = mlp(2048, {1024, 2048, 1024}), b = mlp(1024, {1024, 2048, 1024, 2048, 1024}), f = mlp(1024, {1024, 512, 256, 128});
    a.cw = b.cw = f.cw = cw;
    at(a, {256, 64, 304}), at(b, {256, 64, 304}), at(f, {256, 64, 304});
  }
  for (int vf : {0, 4})
    for (int64_t m : {1024, 4096}) {
      Chain a = mlp(m, {1024, 4096, 1024});
      a.vf = vf;
      one(a);
    }
  // ... two of them with a forced W: fitting (on the smallest tile that fits with it), not fitting (W >= max T on every tile; m / BM * W above the compute units)
  for (int w : {4, 8, 16, 32, 64, 300}) {
    Chain c = mlp(1024, {1024, 4096, 1024});
    c.sw = 1000 + w;
    one(c);
    c.cw = 1;
    one(c);
  }
  // ... and with every call on the 64x64 tile (the A/B's forced-W rows)
  for (int w : {8, 16}) {
    Chain c = mlp(1024, {1024, 4096, 1024});
    c.forced = 21, c.sw = 1000 + w;
    one(c);
  }
  // the GPU test's chains: per tile t and image, every call forced to the tile's variant, m = 2 BM (one of 3 BM), W forced
  for (int t = 0; t < 4; ++t)
    for (int vf : {2, 0, 4}) {
      const int64_t bn = BN[t], m = 2 * BM[t];
      const int f = BASE[vf] + t;
      one(gpu(m, {4 * bn, bn, 2 * bn}, 192, 1, f, vf, 2)), one(gpu(m, {4 * bn, bn, 2 * bn}, 192, 1, f, vf, 3)), one(gpu(m, {bn, 3 * bn, bn}, 192, 1, f, vf, 1));
      one(gpu(m, {2 * bn, bn, 2 * bn, bn, 2 * bn, bn, 2 * bn, bn}, 192, 1, f, vf, 1));
      { Chain c = gpu(m, {2 * bn, 2 * bn, bn}, 192, 2, f, vf, 1); c.k[0] = 192; one(c); }
      { Chain c = gpu(m, {3 * bn, bn}, 256, 1, f, vf, 2); c.br[0] = 3; one(c); }
      one(gpu(3 * BM[t], {4 * bn, 2 * bn}, 192, 1, f, vf, 2));
      one(gpu(m, {1024, 512, 1024}, 512, 1, f, vf, 3));
      one(gpu(m, {4 * bn, bn, 4 * bn}, 192, 1, f, vf, 2)), one(gpu(m, {bn, 4 * bn, 4 * bn}, 192, 1, f, vf, 2));
    }
  // ... its chain that exceeds the chip, by the rule on the 32x64 tile, at three CU counts; with a forced W above the compute units; under the one-round switch alone
  { Chain c = gpu(1024, {640, 64, 640}, 64, 1, 20, 2, 1); c.sw = 1; at(c, {256, 64, 304}); c.sw = 1009; one(c); c.sw = 0, c.cw = 1; one(c); }
  // ... its small chain by the rule (max T fits in one round: two balanced rounds), and forced W >= max T
  { Chain c = gpu(128, {256, 64, 128}, 192, 1, 21, 2, 1); c.sw = 1; one(c); for (int w : {4, 5, 64}) { c.sw = 1000 + w; one(c); } }
  // ... its funnel under both switches (the one-round rule takes it), and its MLP (force_variant(21), mode 1002 and off)
  for (int t = 0; t < 4; ++t) { Chain c = gpu(2 * BM[t], {4 * BN[t], 2 * BN[t], BN[t]}, 192, 1, 20 + t, 2, 1); c.sw = 1, c.cw = 1; one(c); c.cw = 0; one(c); }
  { Chain c = mlp(256, {256, 512, 128, 256}); c.forced = 21, c.sw = 1002; one(c); c.sw = 0; one(c); c.sw = 1, c.forced = -1; one(c); }
  // strict mode: on the tile all calls were dispatched on; without one, refused (rule and forced W)
  { Chain c = gpu(128, {256, 64, 128}, 192, 1, 21, 2, 2); c.strict = true; one(c); c.sw = 1; one(c); c.forced = -1; one(c); c.sw = 1002; one(c); }
  // a planned tile that does not fit with its balanced W: strict refuses, otherwise another tile
  { Chain c = mlp(16384, {1024, 4096, 1024}); c.forced = 20; one(c); c.strict = true; one(c); }
  // refusals, one each (everything else as 1024 rows x [1024, 4096, 1024])
  const std::vector<int64_t> F = {1024, 4096, 1024};
  { Chain c = mlp(1024, F); c.sw = 0; one(c); }                       // the switch off
  { Chain c = mlp(1024, F); c.dtype = DT_F32; one(c); }               // f32
  { Chain c = mlp(1024, F); c.beta1 = true; one(c); }                 // beta 1
  { Chain c = mlp(1024, F); c.vnni_c = true; one(c); }                // a VNNI C
  { Chain c = mlp(1024, F); c.forced = V_GENERIC; one(c); }           // the generic kernel
  { Chain c = mlp(1024, F); c.vf1 = 4; one(c); }                      // the calls' B images differ
  { Chain c = mlp(1024, F); c.br[0] = 0; one(c); }                    // an empty batch
  { Chain c = mlp(1024, {200, 4096, 1024}); c.kind_given = 0; one(c); } // a k of 200
  { Chain c = mlp(1024, {1024, 4096}); one(c); }                      // one call
  { Chain c = mlp(1024, {1024, 512, 256, 512, 256, 512, 256, 512, 256, 512}); one(c); } // nine calls
  { Chain c = mlp(1024, {1024, 512, 256, 512, 256, 512, 256, 512, 256}); one(c); }     // eight
  one(mlp(1024, {1024, 1024, 1024}));                                 // every n equal
  one(mlp(1000, F)), one(mlp(1024, {1024, 4096, 96, 128})), one(mlp(1024, {1024, 1000, 512})); // a ragged m, an n no tile divides, a ragged n
  { Chain c = mlp(1000, F); c.kind_given = 0; one(c); }               // ... handed to the rule with an image all the same: no tile divides m
  { Chain c = mlp(1024, {1024, 4096, 96, 128}); c.kind_given = 0; one(c); } // ... or every n
  { Chain c = mlp(65536, F); c.kind_given = 0; one(c); at(c, {64}); } // more row blocks than compute units on every tile
  one(mlp(8192, F)), one(mlp(16384, F));                              // many rounds
  return 0;
}
