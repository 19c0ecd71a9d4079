// driver.cpp - TEST INFRASTRUCTURE for tests/test_gemm_plan.py, never part of the product library.
//
// Steps a fixed list of GEMM calls through the kernel planner (tpp-mlir_amd/csrc/gemm_plan.h) and prints one canonical line per
// decision; the test compares the output with tests/golden/gemm_plan.txt. Lines:
//   D<i> <form> <m>x<n>x<k> [ld<lda>,<ldb>,<ldc>] [s<stride_a>,<stride_b>] e<epilogue> f<forced> : <variant> <name> [gf] [vf] [ct] [bk]
//        a descriptor planned by plan_gemm with that forced variant (-1 = none; "!" = refused): variant, kernel name, and where
//        they apply generic_forced, variant_forced, f32_chain_tile, bf16_lw_b_kind. Leading dimensions default to k, n, n and
//        strides to m k, k n (packed blocks); they are printed when given.
//   D<i> c br<br> [a<A|B>/<C>/<D>] [S<split>] [strict] : <launch>   one invoke (plan_gemm_call); alignments in bytes, when not 16
//   D<i> g n<items> [v<vec_ok><out_ok><pair_ok>] h<br_hint> [...] : <launch>   a tile-queue group (plan_gemm_group)
//   D<i> qp n<items> br<br> [...] : <0|1>  /  D<i> q n<quads> br<br> : <launch>   quads (gemm_quads_pay, plan_gemm_quads)
// Forms: f32, x6 (f32 under bf16x6), bt (f32, B read transposed), v2 / v4 (bf16, VNNI-2 / VNNI-4 B), flat (bf16, flat B),
// vc (bf16 VNNI-2 with a VNNI-2 C). Epilogue: b = beta 0, B = bias, r = relu.
#include "gemm_plan.h"
#include <stdio.h>
#include <string.h>
#include <vector>

using namespace tpp;

namespace {

const int CUS = 256; // MI355X, and what a host without a device plans for
int g_next = 0;

struct Form {
  const char *name;
  int64_t dtype;
  int vnni_b, vf, vnni_c, b_trans, prec;
};
const Form F32{"f32", DT_F32, 0, 0, 0, 0, 0}, X6{"x6", DT_F32, 0, 0, 0, 0, 6}, BT{"bt", DT_F32, 0, 0, 0, 1, 0},
    V2{"v2", DT_BF16, 1, 2, 0, 0, 0}, V4{"v4", DT_BF16, 1, 4, 0, 0, 0}, FLAT{"flat", DT_BF16, 0, 0, 0, 0, 0},
    VC{"vc", DT_BF16, 1, 2, 1, 0, 0};

struct D {
  int id;
  GemmDesc d;
};

GemmPlanEnv env(int split = -1, bool strict = false) { return GemmPlanEnv{CUS, strict, split}; }

// ep: "b" beta 0, "B" bias, "r" relu (any combination, "" = none)
D desc(const Form &f, int64_t m, int64_t n, int64_t k, const char *ep = "b", int forced = -1, int64_t lda = -1, int64_t ldb = -1,
       int64_t ldc = -1, int64_t sa = -1, int64_t sb = -1) {
  GemmDesc d;
  memset(&d, 0, sizeof(d));
  d.kind = KIND_GEMM;
  d.has_batch = 1;
  d.dtype = f.dtype;
  d.m = m, d.n = n, d.k = k;
  d.lda = lda >= 0 ? lda : k;
  d.ldb = ldb >= 0 ? ldb : n;
  d.ldc = ldc >= 0 ? ldc : n;
  d.stride_a = sa >= 0 ? sa : m * k;
  d.stride_b = sb >= 0 ? sb : k * n;
  d.beta0 = strchr(ep, 'b') != nullptr;
  d.bias = strchr(ep, 'B') != nullptr;
  d.relu = strchr(ep, 'r') != nullptr;
  d.fused = d.bias || d.relu;
  d.vnni_b = f.vnni_b;
  d.vnni_factor = f.vf;
  d.vnni_c = f.vnni_c;
  d.f32_prec = f.prec;
  const bool ok = plan_gemm(d, forced, env());
  if (f.b_trans) { // what the tile queue makes of a folded transpose (rt_rewrites.h dt_sibling)
    d.b_trans = 1;
    d.variant = V_GENERIC;
    d.generic_forced = 1;
    snprintf(d.name, sizeof(d.name), "brgemm_grouped(generic), B read transposed");
  }
  D r{g_next++, d};
  printf("D%d %s %ldx%ldx%ld", r.id, f.name, (long)m, (long)n, (long)k);
  if (lda >= 0 || ldb >= 0 || ldc >= 0) printf(" ld%ld,%ld,%ld", (long)d.lda, (long)d.ldb, (long)d.ldc);
  if (sa >= 0 || sb >= 0) printf(" s%ld,%ld", (long)d.stride_a, (long)d.stride_b);
  printf(" e%s f%d : %s%d %s", *ep ? ep : "-", forced, ok ? "" : "!", d.variant, d.name);
  if (d.generic_forced) printf(" gf");
  if (d.variant_forced) printf(" vf");
  if (f32_chain_tile(d) >= 0) printf(" ct%d", f32_chain_tile(d));
  if (bf16_lw_b_kind(d) >= 0) printf(" bk%d", bf16_lw_b_kind(d));
  printf("\n");
  return r;
}

const char *generic_name(GemmGeneric g) {
  switch (g) {
  case GG_F32: return "<f32>";
  case GG_F32_VEC: return "<f32,vec>";
  case GG_BF16_VNNI2: return "<bf16,vnni2>";
  case GG_BF16_VNNI2_VEC: return "<bf16,vnni2,vec>";
  case GG_BF16_VNNI4_VEC: return "<bf16,vnni4,vec>";
  case GG_BF16_FLAT: return "<bf16,flat>";
  }
  return "?";
}

void print_launch(const GemmLaunch &l) {
  switch (l.launcher) {
  case GL_NONE: printf("none"); break;
  case GL_INVALID: printf("invalid"); break;
  case GL_F32_FAST: printf("f32_fast t%d", l.tile); break;
  case GL_F32_LW: printf("f32_lw t%d s%d", l.tile, l.split); break;
  case GL_F32_LW16: printf("f32_lw16 t%d s%d", l.tile, l.split); break;
  case GL_F32_LW_GROUPED: printf("f32_lw_grouped t%d s%d", l.tile, l.split); break;
  case GL_F32_X6: printf("f32_x6 t%d v%d", l.tile, (int)l.vec); break;
  case GL_BF16_FAST: printf("bf16_fast t%d", l.tile); break;
  case GL_BF16_SMALL32: printf("bf16_small32 s%d", l.split); break;
  case GL_BF16_GROUPED64: printf("bf16_grouped64"); break;
  case GL_BF16_LW: printf("bf16_lw t%d b%d", l.tile, l.b_kind); break;
  case GL_BF16_LW_GROUPED: printf("bf16_lw_grouped t%d b%d e%d", l.tile, l.b_kind, (int)l.even); break;
  case GL_BF16_LW_QUADS: printf("bf16_lw_quads b%d", l.b_kind); break;
  case GL_GENERIC: printf("generic%s", generic_name(l.generic)); break;
  }
  if (l.text && *l.text) printf(" \"%s\"", l.text);
  printf("\n");
}

void env_suffix(const GemmPlanEnv &e) {
  if (e.forced_split != -1) printf(" S%d", e.forced_split);
  if (e.strict) printf(" strict");
}

// alignments in bytes: A and B, C, D
void call(const D &x, int64_t br, int ab = 16, int c = 16, int dd = 16, GemmPlanEnv e = env()) {
  const GemmAlign al{ab >= 16, c >= 16, c >= 8, dd >= 8, dd >= 16};
  printf("D%d c br%ld", x.id, (long)br);
  if (ab != 16 || c != 16 || dd != 16) printf(" a%d/%d/%d", ab, c, dd);
  env_suffix(e);
  printf(" : ");
  print_launch(plan_gemm_call(x.d, br, al, e));
}

void group(const D &x, int n, int64_t hint, bool vec = true, bool out = true, bool pair = true, GemmPlanEnv e = env()) {
  printf("D%d g n%d", x.id, n);
  if (!vec || !out || !pair) printf(" v%d%d%d", (int)vec, (int)out, (int)pair);
  printf(" h%ld", (long)hint);
  env_suffix(e);
  printf(" : ");
  print_launch(plan_gemm_group(x.d, n, vec, out, pair, hint, e));
}

void quads(const D &x, int n, int64_t br, GemmPlanEnv e = env()) {
  printf("D%d qp n%d br%ld", x.id, n, (long)br);
  env_suffix(e);
  printf(" : %d\n", (int)gemm_quads_pay(x.d, n, br, e));
  if (n % 4 == 0 && e.forced_split == -1 && !e.strict) {
    printf("D%d q n%d br%ld : ", x.id, n / 4, (long)br);
    print_launch(plan_gemm_quads(x.d, n / 4, br));
  }
}

// a call at every batch count of interest: empty, one, odd, even, and a long reduction (>= 48 64-k chunks)
void calls(const D &x, int64_t br_long) {
  for (int64_t br : {(int64_t)0, (int64_t)1, (int64_t)3, (int64_t)2, br_long}) call(x, br);
}

const int GROUP_NS[] = {1, 4, 64, 256, 640, 768, 65535, 65536, 131070, 131071};

} // namespace

int main() {
  // ---- named shapes: C2 (1024^3, br 16), C3 (512 x 1024 x 1024, bias + relu), the C4 layer, C5, 4096^3 ------------------------
  {
    D c2 = desc(F32, 1024, 1024, 64, "b", -1, 64, 1024, 1024, 64, 64 * 1024);
    calls(c2, 16), call(c2, 64), call(c2, 16, 4), call(c2, 16, 16, 8);
    D c2w = desc(F32, 1024, 1024, 1024);
    calls(c2w, 64);
    D c3 = desc(F32, 512, 1024, 1024, "bBr");
    calls(c3, 48), call(c3, 1, 16, 16, 8), call(c3, 1, 16, 16, 4);
    D c4 = desc(V2, 4096, 1024, 1024, "bBr");
    calls(c4, 48), call(c4, 1, 16, 8, 8), call(c4, 1, 16, 16, 4), call(c4, 1, 4);
    D c4v4 = desc(V4, 4096, 1024, 1024, "bBr");
    calls(c4v4, 48);
    D c5 = desc(V2, 2048, 2048, 2048);
    calls(c5, 48);
    D c5f = desc(FLAT, 2048, 2048, 2048);
    calls(c5f, 48), call(c5f, 1, 4), call(c5f, 1, 16, 8);
    for (const Form *f : {&F32, &V2, &V4, &FLAT, &X6}) {
      D big = desc(*f, 4096, 4096, 4096);
      call(big, 1), call(big, 0);
    }
  }
  // ---- the reference's benchmark layers (tests/golden/benchmark_configs.json): whole-layer calls and their tile invokes -------
  {
    struct L { int64_t M, N, K, tm, tn, tk; };
    const L layers[] = {{1024, 2560, 1024, 64, 64, 64}, {1024, 512, 256, 64, 64, 64},   {1024, 1024, 512, 64, 64, 64},
                        {1024, 352, 512, 32, 32, 32},   {128, 1024, 1024, 64, 64, 64},  {128, 4096, 1024, 64, 64, 64},
                        {128, 768, 2304, 64, 48, 64},   {128, 768, 3072, 32, 48, 32},   {128, 1024, 4096, 64, 64, 64},
                        {128, 3072, 768, 64, 64, 64},   {128, 768, 768, 32, 64, 64},    {256, 1024, 1024, 64, 64, 64},
                        {256, 1024, 1024, 32, 32, 32},  {256, 4096, 1024, 64, 64, 64},  {256, 768, 3072, 64, 64, 64},
                        {256, 1024, 4096, 64, 64, 64},  {256, 3072, 768, 64, 64, 64},   {256, 768, 768, 64, 64, 64}};
    for (const L &l : layers)
      for (const Form *f : {&F32, &V2, &V4}) {
        D w = desc(*f, l.M, l.N, l.K, "bBr");
        call(w, 1);
        D t = desc(*f, l.tm, l.tn, l.tk, "bBr");
        const int64_t br = l.K / l.tk;
        const int n = (int)((l.M / l.tm) * (l.N / l.tn));
        call(t, br), group(t, n, br);
        if (l.tk == 32) group(t, n, br, true, true, false);
      }
    // some as 64-k brgemm calls over a row-major layer (A: lda = K, stride 64; B: stride 64 rows)
    for (int i : {0, 4, 6, 8, 11, 15}) {
      const L &l = layers[i];
      for (const Form *f : {&F32, &V2}) {
        D b = desc(*f, l.M, l.N, 64, "b", -1, l.K, l.N, l.N, 64, 64 * l.N);
        call(b, l.K / 64);
      }
    }
  }
  // ---- small and ragged tiles: 32x32x32, n = 48, k not a multiple of 64, ragged m / n ------------------------------------------
  {
    struct S { int64_t m, n, k; };
    const S shapes[] = {{32, 32, 32}, {64, 48, 64}, {32, 48, 32}, {64, 48, 32}, {64, 64, 48}, {96, 96, 64}, {40, 64, 64}, {33, 35, 17}};
    for (const S &s : shapes)
      for (const Form *f : {&F32, &V2, &V4}) {
        D t = desc(*f, s.m, s.n, s.k);
        call(t, 2), call(t, 3), call(t, 96);
        group(t, 64, 16), group(t, 768, 2);
      }
    // every work-list length of interest, on the tiles that reach the grouped kernels' size rules
    for (const Form *f : {&F32, &V2, &V4})
      for (const S &s : {S{64, 64, 64}, S{32, 32, 32}, S{64, 48, 64}}) {
        D t = desc(*f, s.m, s.n, s.k, "bBr");
        for (int n : GROUP_NS) group(t, n, 16);
      }
  }
  // ---- operand forms and epilogues: vnni_c, b_trans, bf16x6, beta0 / bias / relu --------------------------------------------
  {
    for (const char *ep : {"", "B", "r", "Br"}) {
      D f = desc(F32, 128, 1024, 1024, ep);
      call(f, 1, 16, 16, 8), group(f, 1, 1, true, false, true);
      D v = desc(V2, 256, 1024, 1024, ep);
      call(v, 1, 16, 16, 4), call(v, 1, 16, 8, 8);
    }
    for (const Form *f : {&VC, &BT, &X6})
      for (int64_t m : {(int64_t)64, (int64_t)1024})
        for (int64_t n : {(int64_t)64, (int64_t)48}) {
          D t = desc(*f, m, n, 64, "bBr");
          call(t, 16), call(t, 1, 4), group(t, 64, 16);
        }
    D vc4 = desc(Form{"vc4", DT_BF16, 1, 4, 1, 0, 0}, 128, 128, 64);
    call(vc4, 2), group(vc4, 64, 2);
    D btv = desc(Form{"btv", DT_BF16, 1, 2, 0, 1, 0}, 64, 64, 64);
    call(btv, 2), group(btv, 64, 2);
    for (int fx = 12; fx <= 15; ++fx)
      for (const Form *f : {&X6, &F32}) {
        D t = desc(*f, 1024, 1024, 1024, "bBr", fx);
        call(t, 1), call(t, 1, 4);
        D r = desc(*f, 96, 96, 64, "b", fx);
        call(r, 1);
      }
    D x6r = desc(X6, 512, 1024, 1024, "b", -1, 1024, 1024, 1026);
    call(x6r, 1);
  }
  // ---- alignment: leading dimensions / strides at 16 / 8 / 4 bytes, lane-offset limits below and at 1 << 20 / 21 / 22 ---------
  {
    for (const Form *f : {&F32, &V2, &V4, &FLAT}) {
      for (int64_t pad : {(int64_t)2, (int64_t)4}) {
        D a = desc(*f, 256, 1024, 1024, "b", -1, 1024 + pad, 1024, 1024);
        call(a, 1), group(a, 16, 2);
        D b = desc(*f, 256, 1024, 1024, "b", -1, 1024, 1024 + pad, 1024);
        call(b, 1), group(b, 16, 2);
        D c = desc(*f, 256, 1024, 1024, "b", -1, 1024, 1024, 1024 + pad);
        call(c, 1), group(c, 16, 2);
        D s = desc(*f, 64, 64, 64, "b", -1, -1, -1, -1, 64 * 64 + pad, 64 * 64 + pad);
        call(s, 2), group(s, 1024, 16);
      }
      for (int lim : {20, 21, 22, 24}) {
        if (lim == 24 && f != &F32) continue;
        // all three just below the bound, then each at it
        const int64_t ld = (int64_t)1 << lim;
        D below = desc(*f, 64, 64, 64, "b", -1, ld - 8, ld - 8, ld - 8);
        call(below, 2), group(below, 1024, 16);
        for (int which = 0; which < 3; ++which) {
          D t = desc(*f, 64, 64, 64, "b", -1, which == 0 ? ld : ld - 8, which == 1 ? ld : ld - 8, which == 2 ? ld : ld - 8);
          call(t, 2), group(t, 1024, 16);
        }
      }
    }
    // the 32-k pair limits of the f32 loader-wave kernels (stride < 1 << 26), negative strides
    for (int64_t st : {((int64_t)1 << 26) - 8, (int64_t)1 << 26, (int64_t)-1024}) {
      D t = desc(F32, 64, 64, 32, "b", -1, -1, -1, -1, st, st);
      call(t, 2), group(t, 64, 2), group(t, 1024, 2);
      D u = desc(V2, 64, 64, 64, "b", -1, -1, -1, -1, st, st);
      group(u, 64, 16), group(u, 1024, 16);
    }
  }
  // ---- forced variants 0 .. 31 (and the generic kernel) on a shape that fits and one that does not -----------------------------
  {
    for (int v = 0; v < 32; ++v)
      for (const Form *f : {&F32, &V2, &V4, &FLAT}) {
        if (f == &FLAT && v < V_BF16_FAST) continue;
        desc(*f, 256, 256, 256, "b", v);
        if (v == V_GENERIC || v == V_BF16_SMALL32 || v == V_F32_LW16_32x16 || v == V_BF16_LW_32x64) {
          D odd = desc(*f, 96, 96, 64, "b", v);
          call(odd, 2), group(odd, 64, 2);
        }
      }
    for (int v : {V_GENERIC, V_BF16_SMALL32, V_BF16_LW_32x64, V_BF16_LW4_32x64, V_F32_LW16_32x16}) {
      for (const Form *f : {&F32, &V2, &V4}) {
        D skinny = desc(*f, 128, 1024, 1024, "b", v);
        call(skinny, 1), call(skinny, 4);
        D tile = desc(*f, 64, 64, 64, "b", v);
        call(tile, 64), group(tile, 64, 64);
        D t32 = desc(*f, 32, 32, 32, "b", v);
        call(t32, 32), group(t32, 256, 32);
      }
    }
  }
  // ---- forced split counts and strict mode --------------------------------------------------------------------------------------
  {
    std::vector<D> ds;
    for (const Form *f : {&F32, &V2, &V4}) {
      ds.push_back(desc(*f, 128, 1024, 4096));
      ds.push_back(desc(*f, 128, 768, 64));
      ds.push_back(desc(*f, 64, 64, 64));
      ds.push_back(desc(*f, 64, 48, 64));
      ds.push_back(desc(*f, 32, 32, 32));
    }
    for (const GemmPlanEnv &e : {env(-1, false), env(0, false), env(2, false), env(5, false), env(-1, true), env(2, true)}) {
        for (size_t i = 0; i < ds.size(); i += 5) {
          call(ds[i], 1, 16, 16, 16, e);
          call(ds[i + 1], 48, 16, 16, 16, e);
          group(ds[i + 2], 64, 64, true, true, true, e), group(ds[i + 2], 1024, 16, true, true, true, e);
          group(ds[i + 3], 32, 36, true, true, true, e);
          call(ds[i + 4], 32, 16, 16, 16, e), group(ds[i + 4], 4096, 32, true, true, true, e);
        }
      }
  }
  // ---- quads ------------------------------------------------------------------------------------------------------------------
  {
    for (const Form *f : {&V2, &V4}) {
      D t = desc(*f, 64, 64, 64, "bBr");
      for (int n : {4, 6, 64, 256, 640, 642, 1024})
        for (int64_t br : {(int64_t)1, (int64_t)16}) quads(t, n, br);
      quads(t, 640, 0), quads(t, 640, 16, env(2)), quads(t, 640, 16, env(-1, true));
    }
    for (const Form *f : {&F32, &FLAT}) {
      D t = desc(*f, 64, 64, 64, "bBr");
      quads(t, 640, 16);
    }
    D big = desc(V2, 128, 64, 64);
    quads(big, 640, 16);
    D odd = desc(V2, 64, 64, 64, "b", -1, 68, 64, 64);
    quads(odd, 640, 16);
    D forced = desc(V2, 64, 64, 64, "b", V_BF16_LW_64x64);
    quads(forced, 640, 16);
    D fg = desc(V2, 64, 64, 64, "b", V_GENERIC);
    quads(fg, 640, 16);
  }
  return 0;
}
