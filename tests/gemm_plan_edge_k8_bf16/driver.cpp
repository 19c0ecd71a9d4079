// driver.cpp - TEST INFRASTRUCTURE for tests/test_gemm_plan_edge_k8_bf16.py, never part of the product library.
//
// Steps whole-layer bf16 calls through the kernel planner (tpp-mlir_amd/csrc/gemm_plan.h) under the modes of the half-step ragged k
// (xsmm_hip_set_edge_k8_bf16: 0, 1, 21) crossed with edge-tile modes 0, 2 and 22 and the older ragged-k switch (xsmm_hip_set_edge_k_bf16) 0 and
// 1, and prints one line per call and CU count; the test compares the output with tests/golden/gemm_plan_edge_k8_bf16.txt and checks
// the rule on every line. One line per m, n, k and B image; the (batch count, CU count) pairs that get the same answers share a part,
// and inside a part the (edge-tile mode, old switch) pairs that get the same answers share a group:
//   <m>x<n>x<k> vf<0 flat|2|4> | br<batch>c<CUs>,... : v<variant> <launcher> t<tile> s<split> b<B image> "<text>" ; <et>/<old>,...=<base> <d> <d> <d> ; ... | ...
// Behind the colon: the decision with every switch off, from a GemmPlanEnv that never names the new field. <base>: the decision under
// the edge-tile mode and the old switch, again without naming the new field - "-" = the one with all off, field by field;
// "e<variant>" = an edge launch on that tile; "k<variant>" / "K<variant>" = the old switch's ragged-k launch (", ragged k" / ", edge
// tiles, ragged k"). The three <d>: edge_k8_bf16 = 0, 1, 21 on top of it - "-" = the base decision, field by field, and no half-step
// launch; "h<variant>" = a half-step launch on that tile with its B image (20 + t VNNI-2, 24 + t flat, 28 + t VNNI-4), launcher bf16_lw,
// split 1, the tile's "..., ragged k, half step" text; "H<variant>" = the same with the "..., edge tiles, ragged k, half step" text;
// anything else in full behind a "!".
#include "gemm_plan.h"
#include <stdio.h>
#include <string.h>
#include <string>
#include <utility>
#include <vector>

using namespace tpp;

namespace {

const int CUS[] = {256, 304};
const int ETS[] = {0, 2, 22};
const int OLD[] = {0, 1};
const int NEW[] = {0, 1, 21};

struct Call {
  int64_t m, n, k, br;
  int vf; // B image: 0 flat, 2 VNNI-2, 4 VNNI-4
};

// a whole-layer call, beta 0: A [m][br * k] row-major read in k-wide batch elements, B [br * k][n] (flat) or its VNNI-2 / VNNI-4 packing
GemmDesc layer(const Call &c) {
  GemmDesc d;
  memset(&d, 0, sizeof(d));
  d.kind = KIND_GEMM;
  d.has_batch = 1;
  d.dtype = DT_BF16;
  d.m = c.m, d.n = c.n, d.k = c.k;
  d.lda = c.k * c.br;
  d.ldb = c.n, d.ldc = c.n;
  d.stride_a = c.k, d.stride_b = c.k * d.ldb;
  d.beta0 = 1;
  d.vnni_b = c.vf != 0, d.vnni_factor = c.vf;
  return d;
}

const char *launcher_name(GemmLauncher l) {
  return l == GL_BF16_LW ? "bf16_lw" : l == GL_BF16_SMALL32 ? "bf16_small32" : l == GL_BF16_FAST ? "bf16_fast" : l == GL_GENERIC ? "generic" : l == GL_NONE ? "none" : "other";
}
std::string tile_text(int variant, const char *suffix) {
  static const char *const tile[4] = {"<32x64,k2>", "<64x64>", "<64x128>", "<128x128>"};
  return std::string(variant < 24 ? "brgemm_bf16_lw" : variant < 28 ? "brgemm_bf16_lw_flatb" : "brgemm_bf16_lw_vnni4") + tile[variant & 3] + suffix;
}
struct Decision {
  GemmDesc d;
  GemmLaunch l;
};
const GemmAlign ALIGNED{true, true, true, true, true};
// nw < 0: the environment never names the new field
Decision decide(const Call &c, int cus, int et, int old, int nw) {
  GemmPlanEnv env{cus, false, -1};
  env.edge_tiles = et, env.edge_k_bf16 = old;
  if (nw >= 0) env.edge_k8_bf16 = nw;
  Decision x;
  x.d = layer(c);
  plan_gemm(x.d, -1, env);
  x.l = plan_gemm_call(x.d, c.br, ALIGNED, env);
  return x;
}
bool same(const Decision &a, const Decision &b) {
  return a.d.variant == b.d.variant && !strcmp(a.d.name, b.d.name) && a.d.generic_forced == b.d.generic_forced && a.d.variant_forced == b.d.variant_forced &&
         a.l.launcher == b.l.launcher && a.l.tile == b.l.tile && a.l.split == b.l.split && a.l.b_kind == b.l.b_kind && a.l.even == b.l.even &&
         a.l.vec == b.l.vec && a.l.generic == b.l.generic && !strcmp(a.l.text, b.l.text) && a.l.tail_tiles == b.l.tail_tiles &&
         a.l.tail_split == b.l.tail_split && a.l.edge == b.l.edge && a.l.edge_k == b.l.edge_k && a.l.edge_k8 == b.l.edge_k8;
}
int bf16_variant(const GemmLaunch &l) {
  return l.launcher == GL_BF16_LW && l.tile >= 0 && l.tile <= 3 && (l.b_kind == 0 || l.b_kind == 2 || l.b_kind == 4) ? 20 + 2 * l.b_kind + l.tile : -1;
}

// the decisions of one call at one CU count: "<off decision> ; <et>/<old>,...=<base> <d0> <d1> <d21> ; ..." - the (edge-tile mode, old
// switch) pairs with the same four answers share a group
std::string decisions(const Call &c, int cus) {
  char buf[512];
  const Decision off = decide(c, cus, 0, 0, -1);
  snprintf(buf, sizeof buf, "v%d %s t%d s%d b%d \"%s\"", off.d.variant, launcher_name(off.l.launcher), off.l.tile, off.l.split, off.l.b_kind, off.l.text);
  std::string out = buf;
  std::vector<std::pair<std::string, std::string>> groups; // answers -> keys
  for (int et : ETS)
    for (int old : OLD) {
      const Decision base = decide(c, cus, et, old, -1);
      const int bv = bf16_variant(base.l);
      const bool plain = bv > 0 && base.l.split == 1 && !base.l.edge_k8;
      if (same(base, off) && !base.l.edge && !base.l.edge_k && !base.l.edge_k8) snprintf(buf, sizeof buf, "-");
      else if (plain && base.l.edge && !base.l.edge_k && tile_text(bv, ", edge tiles") == base.l.text) snprintf(buf, sizeof buf, "e%d", bv);
      else if (plain && !base.l.edge && base.l.edge_k && tile_text(bv, ", ragged k") == base.l.text) snprintf(buf, sizeof buf, "k%d", bv);
      else if (plain && !base.l.edge && base.l.edge_k && tile_text(bv, ", edge tiles, ragged k") == base.l.text) snprintf(buf, sizeof buf, "K%d", bv);
      else snprintf(buf, sizeof buf, "!v%d %s t%d \"%s\"", base.d.variant, launcher_name(base.l.launcher), base.l.tile, base.l.text);
      std::string ans = buf;
      for (int nw : NEW) {
        const Decision x = decide(c, cus, et, old, nw);
        const int v = bf16_variant(x.l);
        const bool desc_same = x.d.variant == off.d.variant && !strcmp(x.d.name, off.d.name) && x.d.generic_forced == off.d.generic_forced &&
                               x.d.variant_forced == off.d.variant_forced;
        const bool half = x.l.edge_k8 && !x.l.edge_k && !x.l.edge && desc_same && v > 0 && x.l.split == 1 && x.l.tail_tiles == 0;
        if (same(x, base)) snprintf(buf, sizeof buf, " -");
        else if (half && tile_text(v, ", ragged k, half step") == x.l.text) snprintf(buf, sizeof buf, " h%d", v);
        else if (half && tile_text(v, ", edge tiles, ragged k, half step") == x.l.text) snprintf(buf, sizeof buf, " H%d", v);
        else snprintf(buf, sizeof buf, " !v%d %s t%d s%d b%d edge%d%d%d \"%s\"", x.d.variant, launcher_name(x.l.launcher), x.l.tile, x.l.split, x.l.b_kind,
                      (int)x.l.edge, (int)x.l.edge_k, (int)x.l.edge_k8, x.l.text);
        ans += buf;
      }
      snprintf(buf, sizeof buf, "%d/%d", et, old);
      bool found = false;
      for (auto &g : groups)
        if (g.first == ans) g.second += std::string(",") + buf, found = true;
      if (!found) groups.push_back({ans, buf});
    }
  for (auto &g : groups) out += " ; " + g.second + "=" + g.first;
  return out;
}

// one line per m, n, k and image: the (batch count, CU count) pairs with the same decisions share a part
void line(int64_t m, int64_t n, int64_t k, int vf) {
  std::vector<std::pair<std::string, std::string>> parts; // decisions -> keys
  for (int64_t br : {1, 3})
    for (int cus : CUS) {
      const std::string d = decisions(Call{m, n, k, br, vf}, cus);
      char key[32];
      snprintf(key, sizeof key, "br%ldc%d", (long)br, cus);
      bool found = false;
      for (auto &p : parts)
        if (p.first == d) p.second += std::string(",") + key, found = true;
      if (!found) parts.push_back({d, key});
    }
  printf("%ldx%ldx%ld vf%d", (long)m, (long)n, (long)k, vf);
  for (auto &p : parts) printf(" | %s : %s", p.second.c_str(), p.first.c_str());
  printf("\n");
}

} // namespace

int main() {
  for (int64_t m : {128, 256, 1000, 1024, 4096})
    for (int64_t n : {128, 256, 1000, 1024, 4096})
      for (int64_t k : {72, 200, 1000, 784, 1024})
        for (int vf : {2, 0, 4}) line(m, n, k, vf);
  return 0;
}
