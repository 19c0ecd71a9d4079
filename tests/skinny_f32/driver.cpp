// driver.cpp - TEST INFRASTRUCTURE for tests/test_skinny_f32_cpu.py, never part of the product library. Linked with the real gemm_plan.cpp.
//   driver maps            walks the maps of tpp-mlir_amd/csrc/brgemm_f32_skinny.h by brute force and prints counts
//   driver plan            a written list of calls through plan_gemm_call under xsmm_hip_set_skinny_f32 modes 0, 1, 16, 32, 64
//   driver golden < specs  descriptors "form m n k lda ldb ldc sa sb ep forced" (-1: the default; ep "-": none): does mode 64 change a plan?
#include "brgemm_f32_skinny.h"
#include "gemm_plan.h"
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

using namespace tpp;

static int maps() {
  for (int bn = 16; bn <= 64; bn *= 2) {
    const int C = skf_cols(bn);
    // every (k, column) of a step's 16 x BN slab is loaded by exactly one lane, at its address in the flat B; MFMA (r, j) pairs the same
    // real k on both sides, B's column is the lane's output column j, and over r and the four k-slots every k of the step comes once
    std::vector<int> seen(16 * bn, 0), kseen(16 * bn, 0);
    long once = 0, bad = 0;
    for (int l = 0; l < 64; ++l)
      for (int r = 0; r < 4; ++r)
        for (int e = 0; e < C; ++e) {
          ++seen[skf_load_k(l, r) * bn + skf_load_col(bn, l, e)];
          bad += skf_load_byte(bn, l, r, 1000) + 4 * e != 4 * (skf_load_k(l, r) * 1000 + skf_load_col(bn, l, e));
          const int kb = skf_load_k(l, skf_mfma_b_row(r, e)), ka = skf_a_k(l, skf_mfma_a_elem(r, e)); // MFMA (r, j = e)
          bad += ka != kb || skf_load_col(bn, l, skf_mfma_b_elem(r, e)) != skf_out_col(bn, l, e) || skf_a_row(0, l) != (l & 15);
          ++kseen[kb * bn + skf_out_col(bn, l, e)];
        }
    for (int i = 0; i < 16 * bn; ++i) once += seen[i] == 1 && kseen[i] == 1;
    printf("slab bn %d once %ld bad %ld\n", bn, once, bad);
    // every output element owned by exactly one (block, lane, register); a lane's C columns all stored or all skipped; blocks inside n
    for (int m : {1, 7, 16, 17, 31})
      for (int n : {bn, bn + 4, bn + 12, 200}) {
        std::vector<int> stored((size_t)m * n, 0);
        long sbad = 0, sonce = 0;
        for (int b = 0; b < skf_blocks(n, bn); ++b) {
          const int n0 = skf_origin(b, n, bn);
          sbad += n0 < 0 || n0 + bn > n || n0 % 4 != 0;
          for (int l = 0; l < 64; ++l)
            for (int j = 0; j < C; ++j) {
              const bool stores = skf_out_col(bn, l, 0) >= skf_skip(b, n, bn);
              sbad += stores != skf_owns(b, n, bn, n0 + skf_out_col(bn, l, j));
              for (int s = 0; s < skf_mb(m) / 16; ++s)
                for (int i = 0; i < 4; ++i)
                  if (stores && skf_out_row(s, l, i) < m) ++stored[(size_t)skf_out_row(s, l, i) * n + n0 + skf_out_col(bn, l, j)];
            }
        }
        for (int v : stored) sonce += v == 1;
        printf("store bn %d m %d n %d once %ld bad %ld\n", bn, m, n, sonce, sbad);
      }
  }
  // ragged k: the lane groups kept in the last step hold exactly the k below the limit, no full step is masked
  for (int kmod = 0; kmod < 16; kmod += 4) {
    const int k = 32 + kmod;
    long kept_below = 0, bad = 0;
    for (int ks = 0; ks < skf_steps(k); ++ks)
      for (int l = 0; l < 64; ++l)
        for (int e = 0; e < 4; ++e) {
          const bool kept = skf_group_kept(l, skf_step_klim(k, ks)), below = ks * SKF_KSTEP + skf_a_k(l, e) < k;
          kept_below += kept && below, bad += kept != below;
        }
    printf("mask kmod %d steps %d kept_below %ld bad %ld\n", kmod, skf_steps(k), kept_below, bad);
  }
  // the deal: contiguous ascending runs that cover every step once
  for (int S : {1, 3, SKF_WMAX - 1, SKF_WMAX, SKF_WMAX + 1, 5 * SKF_WMAX + 3, 63}) {
    const int W = skf_waves(S);
    int next = 0, bad = 0;
    for (int w = 0; w < W; ++w) bad += skf_wave_first(w, W, S) != next || skf_wave_count(w, W, S) < 1, next += skf_wave_count(w, W, S);
    printf("deal steps %d waves %d end %d bad %d\n", S, W, next, bad);
  }
  return 0;
}

static GemmDesc desc(const char *form, int64_t m, int64_t n, int64_t k, int64_t lda, int64_t ldb, int64_t ldc, int64_t sa, int64_t sb, const char *ep, int forced) {
  GemmDesc d;
  memset(&d, 0, sizeof(d));
  d.kind = KIND_GEMM, d.has_batch = 1;
  d.dtype = !strcmp(form, "f32") || !strcmp(form, "x6") || !strcmp(form, "bt") || !strcmp(form, "at") ? DT_F32 : DT_BF16;
  d.m = m, d.n = n, d.k = k;
  d.lda = lda >= 0 ? lda : k, d.ldb = ldb >= 0 ? ldb : n, d.ldc = ldc >= 0 ? ldc : n;
  d.stride_a = sa >= 0 ? sa : m * k, d.stride_b = sb >= 0 ? sb : k * n;
  d.beta0 = strchr(ep, 'b') != nullptr, d.bias = strchr(ep, 'B') != nullptr, d.relu = strchr(ep, 'r') != nullptr;
  d.fused = d.bias || d.relu;
  d.vnni_b = !strcmp(form, "v2") || !strcmp(form, "v4") || !strcmp(form, "vc");
  d.vnni_factor = !strcmp(form, "v4") ? 4 : d.vnni_b ? 2 : 0;
  d.vnni_c = !strcmp(form, "vc");
  d.f32_prec = !strcmp(form, "x6") ? 6 : 0;
  plan_gemm(d, forced, GemmPlanEnv{256, false, -1});
  if (!strcmp(form, "bt") || !strcmp(form, "at")) { // a folded transpose (rt_rewrites.h): the sibling is forced onto the generic kernel
    (form[0] == 'b' ? d.b_trans : d.a_trans) = 1;
    d.variant = V_GENERIC, d.generic_forced = 1;
  }
  return d;
}

// a launch, field by field; strict mode and the switch's mode are arguments
static std::string plan_text(const GemmDesc &d, int64_t br, const GemmAlign &al, bool strict, int mode) {
  GemmPlanEnv e{256, strict, -1};
  e.skinny_f32 = mode;
  const GemmLaunch l = plan_gemm_call(d, br, al, e);
  char buf[200];
  snprintf(buf, sizeof buf, "L%d/t%d/s%d/b%d/g%d/e%d%d%d/h%d/tt%d/%s", (int)l.launcher, l.tile, l.split, l.b_kind, (int)l.generic, l.edge, l.edge_k, l.edge_k8, l.halves,
           l.tail_tiles, l.text ? l.text : "");
  return l.launcher == GL_F32_SKINNY ? std::string(l.text) + "/" + std::to_string(l.tile) : buf;
}

// one row: the cell of each mode - "-" (the mode-0 launch, field by field, strict or not) or the taken kernel's text / BN
static void row(const char *what, const GemmDesc &d, int64_t br = 1, GemmAlign al = GemmAlign{true, true, true, true, true}) {
  printf("plan %s :", what);
  for (int mode : {0, 1, 16, 32, 64}) {
    std::string c[2];
    for (int strict = 0; strict < 2; ++strict) c[strict] = plan_text(d, br, al, strict, mode) == plan_text(d, br, al, strict, 0) ? "-" : plan_text(d, br, al, strict, mode);
    printf(" %s", c[0] == c[1] ? c[0].c_str() : "!strict");
  }
  printf("\n");
}

static int plan() {
  const auto f32 = [](int64_t m, int64_t n, int64_t k, int64_t lda = -1, int64_t ldb = -1, int64_t ldc = -1, const char *ep = "bBr", int forced = -1) {
    return desc("f32", m, n, k, lda, ldb, ldc, k, -1, ep, forced);
  };
  row("m8 n1024 k64 br16", f32(8, 1024, 64, 1024), 16);
  row("m31 n1000 k1000 beta1", f32(31, 1000, 1000, -1, -1, -1, ""));
  row("m17 n4096 k64 br64", f32(17, 4096, 64, 4096), 64);
  row("m16 n4096 k64 br64", f32(16, 4096, 64, 4096), 64);
  row("m31 n4096 k64 br16", f32(31, 4096, 64, 1024), 16);
  row("m1 n48 k4 strided", f32(1, 48, 4, 12, 52, 56));
  row("m16 n16 k16", f32(16, 16, 16));
  row("m32", f32(32, 1024, 64, 1024), 16);
  row("n12", f32(8, 12, 64));
  row("n1022", f32(8, 1022, 64));
  row("k6", f32(8, 1024, 6));
  row("ldb1026", f32(8, 1024, 64, -1, 1026));
  row("unaligned C", f32(8, 1024, 64), 1, GemmAlign{true, false, true, true, true});
  row("unaligned bias", f32(8, 1024, 64), 1, GemmAlign{true, true, true, true, false});
  row("unaligned A", f32(8, 1024, 64), 1, GemmAlign{false, true, true, true, true});
  row("bf16", desc("v2", 8, 1024, 64, -1, -1, -1, -1, -1, "bBr", -1));
  row("forced generic", f32(8, 1024, 64, -1, -1, -1, "bBr", V_GENERIC));
  row("B transposed", desc("bt", 8, 1024, 64, -1, -1, -1, -1, -1, "b", -1));
  row("A transposed", desc("at", 8, 1024, 64, -1, -1, -1, -1, -1, "b", -1));
  row("empty batch", f32(8, 1024, 64), 0);
  return 0;
}

static int golden() {
  char form[8], ep[8];
  long m, n, k, lda, ldb, ldc, sa, sb;
  int forced, descs = 0, differ = 0;
  for (; scanf("%7s %ld %ld %ld %ld %ld %ld %ld %ld %7s %d", form, &m, &n, &k, &lda, &ldb, &ldc, &sa, &sb, ep, &forced) == 11; ++descs) {
    const GemmDesc d = desc(form, m, n, k, lda, ldb, ldc, sa, sb, ep, forced);
    for (int64_t br : {1, 3, 16})
      for (int strict = 0; strict < 2; ++strict)
        differ += plan_text(d, br, GemmAlign{true, true, true, true, true}, strict, 64) != plan_text(d, br, GemmAlign{true, true, true, true, true}, strict, 0);
  }
  printf("golden descs %d differ %d\n", descs, differ);
  return 0;
}

int main(int argc, char **argv) {
  const std::string a = argc == 2 ? argv[1] : "";
  return a == "maps" ? maps() : a == "plan" ? plan() : a == "golden" ? golden() : 2;
}
