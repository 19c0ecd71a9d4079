// driver.cpp - TEST INFRASTRUCTURE for tests/test_gemm_plan_chain_dma256.py, never part of the product library.
//
// Steps a fixed list of bf16 / f32 layer chains through the planner's rule for chains on the 256x256 tile (tpp-mlir_amd/csrc/gemm_plan.h
// chain_dma256_b_kind, chain_dma256_on_tile, plan_chain_dma256; xsmm_hip_set_chain_dma256) and prints one line per chain and CU count; the
// test compares the output with tests/golden/gemm_plan_chain_dma256.txt and checks the rule on every line. Lines:
//   <m>x<n> k<k of layer 0>,.. br<batch of layer 0>,.. <f32|bf16> vf<0 flat|2|4> f<forced variant of layer 0>,<.. of the others> img<xsmm_hip_set_dma256_images> sw<switch> st<strict> cus<CUs> :
//       v<variant of layer 0>,<.. of layer 1> kind<shared B image, -1 none, -2 f32> on<every call on the tile> | take<0|1> G<groups> R<rounds> g<gated> "<why not>"
// (a gated line names the groups and rounds the rule gives and the gate that keeps the chain call by call)
#include "gemm_plan.h"
#include <initializer_list>
#include <stdio.h>
#include <string.h>
#include <vector>

using namespace tpp;

namespace {

struct Chain {
  int64_t m, n;
  std::vector<int64_t> k, br;
  int sw = 1;        // xsmm_hip_set_chain_dma256
  int vf = 2;        // B image: 0 flat, 2 VNNI-2, 4 VNNI-4
  int64_t dtype = DT_BF16;
  int forced0 = -1, forced = -1; // xsmm_hip_force_variant at the dispatch of layer 0 / of the later layers
  int images = 0;    // xsmm_hip_set_dma256_images
  bool strict = false;
  int64_t n1 = 0;    // > 0: the later layers' n (a chain of different widths)
};

// layer l of the chain as the MLP dispatches it: A [m][br * k] row-major in k-wide batch elements, B [br * k][n] in its image, beta 0 + bias + relu
GemmDesc layer(const Chain &c, size_t l) {
  GemmDesc d;
  memset(&d, 0, sizeof(d));
  d.kind = KIND_GEMM;
  d.has_batch = 1;
  d.fused = 1;
  d.dtype = c.dtype;
  d.m = c.m, d.n = l > 0 && c.n1 ? c.n1 : c.n, d.k = c.k[l];
  d.lda = c.k[l] * c.br[l], d.ldb = d.n, d.ldc = d.n;
  d.stride_a = c.k[l], d.stride_b = c.k[l] * d.n;
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
  // what rt_chain.h try_chain_launch hands the rule: the shared image, every call on the tile (mode 1 alone reads the images mode), same m and n
  int kind = chain_dma256_b_kind(ds[0]);
  bool on = true, same = true;
  for (const GemmDesc &d : ds) {
    const int kd = chain_dma256_b_kind(d);
    if (kind != -2 && kd != kind) kind = kd == -2 ? -2 : -1;
    on = on && chain_dma256_on_tile(d, c.sw == 1 ? c.images : 0);
    if (d.m != ds[0].m || d.n != ds[0].n) same = false;
  }
  ChainDma256Plan p{false, 0, "the calls differ in m or n, or a batch is empty", false};
  if (same) p = plan_chain_dma256(c.m, c.n, (int)c.k.size(), c.k.data(), c.br.data(), cus, on, kind, c.sw, c.strict);
  const int rounds = p.take ? (int)((c.m / 256 + p.groups - 1) / p.groups) : 0;
  printf("%ldx%ld k", (long)c.m, (long)c.n);
  for (size_t l = 0; l < c.k.size(); ++l) printf("%s%ld", l ? "," : "", (long)c.k[l]);
  printf(" br");
  for (size_t l = 0; l < c.br.size(); ++l) printf("%s%ld", l ? "," : "", (long)c.br[l]);
  printf(" %s vf%d f%d,%d img%d sw%d st%d cus%d : v%d,%d kind%d on%d | take%d G%d R%d g%d \"%s\"\n", c.dtype == DT_F32 ? "f32" : "bf16", c.dtype == DT_F32 ? 0 : c.vf, c.forced0,
         c.forced, c.images, c.sw, (int)c.strict, cus, ds[0].variant, ds.size() > 1 ? ds[1].variant : -1, kind, (int)on, (int)p.take, p.groups, rounds, (int)p.gated, p.why);
}
void both(const Chain &c) {
  for (int cus : {256, 64}) line(c, cus);
}
Chain mlp(int64_t m, int64_t n = 1024, int sw = 1) {
  Chain c{m, n, {n, n, n}, {1, 1, 1}};
  c.sw = sw;
  return c;
}
Chain with(Chain c, int vf, int images = 0, int forced = -1, bool strict = false) {
  c.vf = vf, c.images = images, c.forced0 = c.forced = forced, c.strict = strict;
  return c;
}

} // namespace

int main() {
  // the GPU test's shapes: three layers with k0 = 32, 96, 160 (two batch elements), 224 and k = n behind them, the three B images, mode 2 and forced G
  for (int vf : {2, 0, 4}) {
    both(with(Chain{256, 256, {32, 256, 256}, {1, 1, 1}, 2}, vf));
    both(with(Chain{512, 512, {96, 512, 512}, {1, 1, 1}, 2}, vf));
    both(with(Chain{768, 512, {160, 512, 512}, {2, 1, 1}, 2}, vf));
    both(with(Chain{1024, 512, {224, 512, 512}, {1, 1, 1}, 2}, vf));
    both(with(Chain{1280, 256, {32, 256, 256}, {1, 1, 1}, 1002}, vf));
    both(with(Chain{1024, 512, {96, 512, 512}, {1, 1, 1}, 1002}, vf));
    both(with(Chain{768, 256, {160, 256, 256}, {1, 1, 1}, 1001}, vf));
    both(with(Chain{768, 256, {160, 256, 256}, {1, 1, 1}, 1004}, vf)); // a forced G > tiles_m
    // mode 1: forced onto the tile at dispatch (VNNI-2) / taken by xsmm_hip_set_dma256_images(2) (flat, VNNI-4); planned by rule: elsewhere
    both(with(Chain{1024, 512, {512, 512, 512}, {1, 1, 1}, 1}, vf, vf == 2 ? 0 : 2, vf == 2 ? V_BF16_DMA256 : -1));
    both(with(Chain{1024, 512, {512, 512, 512}, {1, 1, 1}, 1}, vf));
    both(with(Chain{1024, 512, {512, 512, 512}, {1, 1, 1}, 1}, vf, 1)); // the images rule: 8 tiles are not this tile's
  }
  // mode 1 on a real overflow: VNNI-2 forced onto the tile, two layers, n = 256, m = 256 x (CUs + 8) (the GPU test reads the CU count from the device)
  for (int cus : {256, 64, 304}) line(with(Chain{256 * (cus + 8), 256, {64, 256}, {1, 1}, 1}, 2, 0, V_BF16_DMA256), cus);
  // three 1024-wide layers and 4096 rows x three 4096-wide layers (the rows of the A/B), as planned: every mode, the three images
  for (int64_t m : {8192, 16384, 32768, 4096, 1024})
    for (int sw : {1, 2, 0}) both(mlp(m, 1024, sw));
  for (int sw : {1, 2}) both(mlp(4096, 4096, sw));
  for (int vf : {0, 4})
    for (int images : {0, 1, 2})
      for (int64_t m : {16384, 4096}) both(with(mlp(m), vf, images));
  both(mlp(16384, 1024, 1032)), both(mlp(16384, 1024, 1064)), both(mlp(16384, 1024, 1065)), both(mlp(16384, 1024, 1001)); // forced G: 32, tiles_m, too many, 1
  // strict mode: only where every call was dispatched on the tile
  both(with(mlp(16384), 2, 0, -1, true)), both(with(mlp(16384, 1024, 2), 2, 0, -1, true)), both(with(mlp(4096, 1024, 2), 2, 0, -1, true));
  both(with(mlp(4096, 1024, 2), 2, 0, V_BF16_DMA256, true)), both(with(mlp(4096, 1024, 1000 + 16), 2, 0, -1, true));
  // refusals, one each (everything else as 16384 x 1024 x 3 layers under mode 2; the switch off is above)
  both(mlp(16400, 1024, 2)), both(mlp(384, 256, 2)), both(Chain{512, 384, {384, 384, 384}, {1, 1, 1}, 2});  // 256 not dividing m / n
  { Chain c = mlp(16384, 1024, 2); c.k[0] = 40; both(c); c.k[0] = 1000; both(c); c.k[0] = 48; both(c); } // a k % 32
  { Chain c = mlp(16384, 1024, 2); c.dtype = DT_F32; both(c); }                                          // f32
  { Chain c = mlp(16384, 1024, 2); c.br[0] = 0; both(c); }                                               // an empty batch
  { Chain c{16384, 1024, {1024}, {1}, 2}; both(c); }                                                     // one call
  { Chain c{16384, 1024, std::vector<int64_t>(9, 1024), std::vector<int64_t>(9, 1), 2}; both(c); }       // nine calls
  { Chain c{16384, 1024, std::vector<int64_t>(8, 1024), std::vector<int64_t>(8, 1), 2}; both(c); }       // eight
  { Chain c = mlp(1024, 1024, 2); c.n1 = 512; c.k = {1024, 1024, 512}; both(c); }                         // layers of different n
  { Chain c = mlp(16384, 1024, 2); c.forced = V_GENERIC; both(c); }                                      // the generic kernel forced
  both(mlp(256, 65536 / 2, 2));                                                                          // a row of tiles wider than the compute units (at 64)
  both(mlp(16384, 1024, 3)), both(mlp(16384, 1024, 1000));                                               // values the setter refuses: off
  return 0;
}
