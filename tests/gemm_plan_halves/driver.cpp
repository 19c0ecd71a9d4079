// driver.cpp - TEST INFRASTRUCTURE for tests/test_gemm_plan_halves.py, never part of the product library.
//
// Steps a fixed list of f32 calls through the kernel planner (tpp-mlir_amd/csrc/gemm_plan.h) under every setting of the halves switch
// (xsmm_hip_set_f32_halves: GemmPlanEnv::halves 0, 1, 2) and prints one line per call and environment; the test compares the output
// with tests/golden/gemm_plan_halves.txt and checks the rule's invariants on every line. Lines:
//   <call|group> <m>x<n>x<k> br<batch> f<forced variant> cus<CUs> S<forced split> T<tail split> E<edge tiles> K<edge k> strict<0|1> al<0|1> :
//       v<variant> <launcher> t<tile> s<split> tail<tail tiles> e<edge> k<edge k> "<name>" "<text>" | h<halves under mode 0><mode 1><mode 2>
// Left of the bar: the decision under mode 0. A mode whose decision differs from it in anything but GemmLaunch::halves, or whose
// descriptor differs in variant or name, prints "!" and the decision in full instead of its digit.
#include "gemm_plan.h"
#include <stdio.h>
#include <string.h>

using namespace tpp;

namespace {

// a whole-layer call as the reference's benchmarks issue it: A [m][k br] row-major read in k-wide batch elements, B [k br][n]
GemmDesc layer(int64_t m, int64_t n, int64_t k, int64_t br) {
  GemmDesc d;
  memset(&d, 0, sizeof(d));
  d.kind = KIND_GEMM;
  d.has_batch = 1;
  d.dtype = DT_F32;
  d.m = m, d.n = n, d.k = k;
  d.lda = k * br, d.ldb = n, d.ldc = n;
  d.stride_a = k, d.stride_b = k * n;
  d.beta0 = true;
  return d;
}

const char *launcher_name(GemmLauncher l) {
  return l == GL_F32_LW ? "f32_lw" : l == GL_F32_LW16 ? "f32_lw16" : l == GL_F32_LW_GROUPED ? "f32_lw_grouped" : l == GL_F32_FAST ? "f32_fast"
         : l == GL_GENERIC ? "generic" : "other";
}

struct Env { int cus = 256, fsplit = -1, tail = 0, edge = 0, edge_k = 0; bool strict = false, aligned = true; };

bool same_but_halves(const GemmLaunch &a, const GemmLaunch &b) {
  return a.launcher == b.launcher && a.tile == b.tile && a.split == b.split && a.b_kind == b.b_kind && a.even == b.even && a.vec == b.vec &&
         a.generic == b.generic && !strcmp(a.text, b.text) && a.tail_tiles == b.tail_tiles && a.tail_split == b.tail_split && a.edge == b.edge &&
         a.edge_k == b.edge_k;
}

// group: the call's descriptor as n_items items of one tile-queue group (plan_gemm_group) instead of one invoke
void line(int64_t m, int64_t n, int64_t k, int64_t br, int forced, const Env &e, int group = 0) {
  GemmLaunch got[3];
  GemmDesc desc[3];
  for (int mode = 0; mode < 3; ++mode) {
    GemmPlanEnv env{e.cus, e.strict, e.fsplit, e.tail, e.edge, e.edge_k};
    env.halves = mode;
    desc[mode] = layer(m, n, k, br);
    if (!plan_gemm(desc[mode], forced, env)) {
      printf("%ldx%ldx%ld refused\n", (long)m, (long)n, (long)k);
      return;
    }
    const GemmAlign al{e.aligned, e.aligned, true, true, e.aligned};
    got[mode] = group ? plan_gemm_group(desc[mode], group, e.aligned, e.aligned, true, br, env) : plan_gemm_call(desc[mode], br, al, env);
  }
  const GemmLaunch &o = got[0];
  printf("%s %ldx%ldx%ld br%ld f%d cus%d S%d T%d E%d K%d strict%d al%d : v%d %s t%d s%d tail%d e%d k%d \"%s\" \"%s\" | h", group ? "group" : "call", (long)m,
         (long)n, (long)k, (long)br, forced, e.cus, e.fsplit, e.tail, e.edge, e.edge_k, (int)e.strict, (int)e.aligned, desc[0].variant,
         launcher_name(o.launcher), o.tile, o.split, o.tail_tiles, (int)o.edge, (int)o.edge_k, desc[0].name, o.text);
  for (int mode = 0; mode < 3; ++mode) {
    const GemmLaunch &l = got[mode];
    if (same_but_halves(l, o) && desc[mode].variant == desc[0].variant && !strcmp(desc[mode].name, desc[0].name)) printf("%d", (int)l.halves);
    else printf("!(v%d %s t%d s%d tail%d e%d k%d \"%s\" h%d)", desc[mode].variant, launcher_name(l.launcher), l.tile, l.split, l.tail_tiles, (int)l.edge,
                (int)l.edge_k, l.text, (int)l.halves);
  }
  printf("\n");
}

} // namespace

int main() {
  for (int cus : {256, 64}) {
    Env e;
    e.cus = cus;
    // eligible: the 64x64 + K2 tile as planned - one tile per CU (C2), 2.5 rounds, two rounds - and forced on the shapes of the GPU test
    line(1024, 1024, 64, 16, -1, e);
    line(1024, 2560, 64, 16, -1, e);
    line(2048, 1024, 64, 16, 6, e);
    line(1024, 1536, 64, 16, 6, e);
    line(1024, 1024, 64, 8, -1, e);
    for (int64_t br : {1, 2}) line(64, 64, 64, br, 6, e);
    for (int64_t br : {3, 4, 5, 7}) line(128, 192, 64, br, 6, e);
    line(128, 128, 128, 3, 6, e);
    line(64, 128, 64, 4, 6, e);
    line(192, 64, 64, 2, 6, e);
    line(1088, 1024, 64, 2, 6, e);
    line(1024, 1024, 64, 0, -1, e); // an empty batch
    // fewer tiles than CUs with a long batch: the split model takes the call
    line(64, 128, 64, 8, 6, e);
    line(256, 256, 64, 64, 6, e);
    // ineligible shapes: n or m not in whole 64x64 tiles (the forced tile is not honoured), other tiles as planned or forced
    line(64, 96, 64, 4, 6, e);
    line(96, 64, 64, 4, 6, e);
    line(64, 96, 64, 4, -1, e);
    line(512, 1024, 64, 16, -1, e);  // 64x32 + K4 (C3)
    line(256, 1024, 64, 16, -1, e);  // 32x32 + K4
    line(128, 1024, 64, 16, -1, e);  // 32x16 half-width tiles
    line(1024, 1024, 64, 16, 5, e);  // 64x64, one K group
    line(1024, 1024, 64, 16, 7, e);  // 64x32 + K4 forced
    line(4096, 4096, 64, 16, -1, e); // 128x64
    line(1024, 1024, 64, 16, 8, e);  // the generic kernel forced
    line(1024, 1024, 32, 16, -1, e); // 32-k tiles: pair mode on the grouped kernel
    // a forced split count, the tail split, strict mode, unaligned operands
    Env s = e;
    s.fsplit = 2;
    line(64, 128, 64, 4, 6, s), line(1024, 1024, 64, 16, -1, s);
    s.fsplit = 0;
    line(64, 128, 64, 8, 6, s), line(1024, 1024, 64, 16, -1, s);
    Env t = e;
    t.tail = 1;
    line(1024, 2560, 64, 16, 6, t), line(1024, 1088, 64, 16, 6, t), line(1024, 1024, 64, 16, 6, t);
    t.tail = 4;
    line(1024, 1088, 64, 2, 6, t), line(1024, 1088, 64, 16, 6, t);
    Env st = e;
    st.strict = true;
    line(1024, 1024, 64, 16, -1, st), line(128, 192, 64, 4, 6, st);
    Env u = e;
    u.aligned = false;
    line(1024, 1024, 64, 16, -1, u);
    // edge tiles and ragged k: planned on the generic kernel, taken by their own switches, never as halves; a divisible call under them
    Env g = e;
    g.edge = 6;
    line(1000, 1000, 64, 16, -1, g), line(1024, 1024, 64, 16, -1, g);
    g.edge = 1;
    line(1056, 1000, 64, 16, -1, g);
    Env r = e;
    r.edge_k = 6;
    line(1024, 1024, 72, 14, -1, r), line(1024, 1024, 64, 16, -1, r);
    r.edge = 6;
    line(1000, 1024, 72, 14, -1, r);
    // a tile-queue group of 64x64x64 items, a group of whole layers
    line(64, 64, 64, 2, -1, e, 24), line(64, 64, 64, 2, -1, e, 1024), line(1024, 1024, 64, 16, -1, e, 2);
  }
  return 0;
}
