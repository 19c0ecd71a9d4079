// driver.cpp - TEST INFRASTRUCTURE for tests/test_gemm_plan_chain_skinny.py, never part of the product library.
//
// Steps a fixed list of layer chains through the planner's rule for skinny-batch chains (tpp-mlir_amd/csrc/gemm_plan.h chain_skinny_b_kind,
// plan_chain_skinny; xsmm_hip_set_chain_skinny) and through plan_chain with the new switch beside the seven others; the test compares the
// output with tests/golden/gemm_plan_chain_skinny.txt and checks the rule on every line. Lines:
//   rule m<m> n<n of layer 0>,.. k<k of layer 0>,.. br<batch of layer 0>,.. img<B image: 0 VNNI-2, 2 flat, 4 VNNI-4> md<mode> cus<CUs> st<strict> | kind<image by
//        chain_skinny_b_kind, -1 none> bn<BN> G<groups> g<gated> "<why not>"
//   chain m<m> n<..> img<..> sw<the other switches on: a name, none or all> sk<mode> cus<CUs> | <form>:<tile>:<groups>:<tiles_m>x<tiles_n> "<why>" [= off | DIFFERS from <the
//        answer with the new switch 0>]
#include "gemm_plan.h"
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

using namespace tpp;

namespace {

struct Chain {
  int64_t m;
  std::vector<int64_t> n, k, br;
  int img = 0;
};

// layer l as the MLP dispatches it: A [m][br * k] row-major in k-wide batch elements (layer 0) / the predecessor's output, B [br * k][n] in
// its image, beta 0 + bias + relu
GemmDesc layer(const Chain &c, size_t l) {
  GemmDesc d;
  memset(&d, 0, sizeof(d));
  d.kind = KIND_GEMM;
  d.has_batch = 1;
  d.fused = 1;
  d.dtype = DT_BF16;
  d.m = c.m, d.n = c.n[l], d.k = c.k[l];
  d.lda = l == 0 ? c.k[0] * (c.br[0] > 0 ? c.br[0] : 1) : c.n[l - 1];
  d.ldb = d.n, d.ldc = d.n;
  d.stride_a = c.k[l], d.stride_b = c.k[l] * d.n;
  d.beta0 = 1, d.bias = 1, d.relu = 1;
  d.vnni_b = c.img != 2, d.vnni_factor = c.img == 4 ? 4 : 2;
  return d;
}
bool plan_all(const Chain &c, int cus, bool strict, std::vector<GemmDesc> &ds) {
  GemmPlanEnv env{cus, strict, -1};
  for (size_t l = 0; l < c.k.size(); ++l) {
    GemmDesc d = layer(c, l);
    if (!plan_gemm(d, -1, env)) return false;
    ds.push_back(d);
  }
  return true;
}
void list(const char *name, const std::vector<int64_t> &v) {
  printf(" %s", name);
  for (size_t i = 0; i < v.size(); ++i) printf("%s%ld", i ? "," : "", (long)v[i]);
}

void rule(const Chain &c, int mode, int cus, bool strict) {
  std::vector<GemmDesc> ds;
  printf("rule m%ld", (long)c.m);
  list("n", c.n), list("k", c.k), list("br", c.br);
  printf(" img%d md%d cus%d st%d |", c.img, mode, cus, (int)strict);
  if (!plan_all(c, cus, strict, ds)) {
    printf(" refused at dispatch\n");
    return;
  }
  const char *why = nullptr;
  int kind = chain_skinny_b_kind(ds[0], &why);
  for (size_t l = 1; l < ds.size() && kind >= 0; ++l)
    if (chain_skinny_b_kind(ds[l], &why) != kind) kind = -1;
  ChainSkinnyPlan p{0, 0, why ? why : "", false};
  if (kind >= 0) p = plan_chain_skinny(c.m, (int)c.k.size(), c.n.data(), c.k.data(), c.br.data(), cus, kind, mode, strict);
  printf(" kind%d bn%d G%d g%d \"%s\"\n", kind, p.bn, p.groups, (int)p.gated, p.why);
}

const char *form_name(int f) {
  static const char *const names[CF_FORMS] = {"calls", "f32", "plain", "edge", "rounds", "ragged", "widths", "wrounds", "wragged", "dma256", "skinny"};
  return f >= 0 && f < CF_FORMS ? names[f] : "?";
}
std::string answer(const ChainLaunchPlan &p) {
  char buf[400];
  if (p.form == CF_CALLS) {
    int at = snprintf(buf, sizeof(buf), "calls \"%s\"", p.why);
    for (int i = 0; i < p.n_notes && at < (int)sizeof(buf); ++i) at += snprintf(buf + at, sizeof(buf) - at, " [no %s: %.60s]", p.notes[i].rule, p.notes[i].why);
  }
  else snprintf(buf, sizeof(buf), "%s:%d:b%d:%d:%dx%d", form_name(p.form), p.tile, p.b_kind, p.groups, p.tiles_m, p.tiles_n);
  return buf;
}
const char *const SW[9] = {"none", "edge", "rounds", "ragged", "widths", "wrounds", "wragged", "dma256", "all"};
ChainPlanEnv env_of(int sw, int skinny) {
  auto on = [&](int i) { return sw == i || sw == 8 ? 1 : 0; };
  return ChainPlanEnv{false, on(1), on(2), on(3), on(4), on(5), on(6), on(7), 0, 0, skinny};
}
void chain(const Chain &c, int skinny, int cus) {
  std::vector<GemmDesc> ds;
  if (!plan_all(c, cus, false, ds)) return;
  std::vector<const GemmDesc *> dp;
  for (const GemmDesc &d : ds) dp.push_back(&d);
  for (int sw = 0; sw < 9; ++sw) {
    ChainCus cu{[](void *a) { return (int64_t)(intptr_t)a; }, (void *)(intptr_t)cus}, cu0 = cu;
    const std::string on = answer(plan_chain((int)dp.size(), dp.data(), c.br.data(), env_of(sw, skinny), cu));
    const std::string off = answer(plan_chain((int)dp.size(), dp.data(), c.br.data(), env_of(sw, 0), cu0));
    printf("chain m%ld", (long)c.m);
    list("n", c.n);
    printf(" img%d sw-%s sk%d cus%d | %s %s%s\n", c.img, SW[sw], skinny, cus, on.c_str(), on == off ? "= off" : "DIFFERS from ", on == off ? "" : off.c_str());
  }
}

Chain mk(int64_t m, std::vector<int64_t> n, int64_t k0, int img = 0) {
  Chain c{m, n, {k0}, std::vector<int64_t>(n.size(), 1), img};
  for (size_t l = 1; l < n.size(); ++l) c.k.push_back(n[l - 1]);
  return c;
}

} // namespace

int main() {
  // every m x every kind of chain x the three images, by rule and under a forced BN
  for (int64_t m : {1, 16, 17, 31, 32})
    for (int img : {0, 2, 4})
      for (int mode : {1, 32}) {
        rule(mk(m, {256, 256, 256}, 256, img), mode, 256, false);       // equal widths
        rule(mk(m, {512, 256, 128}, 784, img), mode, 256, false);       // the funnel
        rule(mk(m, {256, 24, 256}, 256, img), mode, 256, false);        // an n below BN
        rule(mk(m, {100, 64}, 256, img), mode, 256, false);             // n % 8 != 0
        for (int64_t k0 : {8, 72, 1000, 4}) rule(mk(m, {256, 256}, k0, img), mode, 256, false);
        Chain e = mk(m, {256, 256, 256}, 256, img);                     // an empty batch
        e.br[1] = 0;
        rule(e, mode, 256, false);
      }
  // every mode; three CU counts; strict
  for (int64_t m : {16, 17})
    for (int img : {0, 2, 4})
      for (int mode : {0, 1, 16, 32, 64, 2016, 1000 * 600 + 16, 3032, 2, 1000 * 2 + 48}) {
        rule(mk(m, {256, 256, 256}, 256, img), mode, 256, false);
        rule(mk(m, {512, 256, 128}, 784, img), mode, 256, false);
      }
  for (int cus : {64, 256, 304})
    for (int mode : {1, 16, 64, 2016, 1000 * 300 + 16, 1000 * 64 + 32, 1000 * 65 + 32})
      for (int img : {0, 2}) {
        rule(mk(8, {4096, 11008, 4096}, 4096, img), mode, cus, false);
        rule(mk(8, {1000, 1000, 1000}, 1000, img), mode, cus, false);
      }
  for (int mode : {1, 32, 2016}) rule(mk(8, {256, 256, 256}, 256), mode, 256, true);
  rule(Chain{8, {256}, {256}, {1}}, 32, 256, false);                                                               // one call
  rule(mk(8, std::vector<int64_t>(8, 64), 64), 32, 256, false), rule(mk(8, std::vector<int64_t>(9, 64), 64), 32, 256, false); // eight, nine
  { Chain c = mk(8, {144, 96, 64}, 40); c.br = {2, 2, 3}; c.k = {40, 72, 32}; rule(c, 1, 256, false); rule(c, 64, 256, false); } // batches along k
  // through plan_chain, beside each of the seven other switches and all of them: an m < 32 chain is the new form's, every m >= 32 chain
  // answers as with the new switch 0
  for (int skinny : {1, 16, 2032}) {
    chain(mk(8, {256, 200, 256, 64}, 256), skinny, 256);
    chain(mk(31, {512, 256, 128}, 784, 4), skinny, 256);
  }
  for (int skinny : {1, 2016})
    for (int cus : {256, 64}) {
      chain(mk(64, {64, 64, 64}, 64), skinny, cus);
      chain(mk(100, {128, 128, 128}, 128), skinny, cus);
      chain(mk(200, {200, 200, 200, 200}, 200), skinny, cus);
      chain(mk(256, {512, 128, 256}, 256), skinny, cus);
      chain(mk(200, {136, 72, 200}, 200), skinny, cus);
      chain(mk(1024, {1024, 1024, 1024}, 1024), skinny, cus);
      chain(mk(16384, {1024, 1024, 1024}, 1024), skinny, cus);
      chain(mk(32, {128, 128}, 64, 2), skinny, cus);
      chain(mk(32, {72, 64}, 64), skinny, cus);
    }
  return 0;
}
