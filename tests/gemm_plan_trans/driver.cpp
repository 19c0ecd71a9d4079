// driver.cpp - TEST INFRASTRUCTURE for tests/test_gemm_plan_trans.py, never part of the product library.
//
// Steps the siblings the runtime makes of a gemm behind a folded transpose (tpp-mlir_amd/csrc/rt_rewrites.h dt_sibling: B read
// transposed under modes 1 and 2 of xsmm_hip_set_fold_transpose, A read transposed under mode 2) through the kernel planner
// (tpp-mlir_amd/csrc/gemm_plan.h) and prints one line per sibling and alignment; the test compares the output with
// tests/golden/gemm_plan_trans.txt and checks the rule's invariants on every line. Lines:
//   <A|B|AB> mode<1|2> <m>x<n>x<k> lda<lda> ldb<ldb> sa<stride_a> sb<stride_b> <f32|bf16> vnni<0|1> vec<0|1> : <launcher> <instance> "<text>" | <launcher> <instance> "<text>"
// Left of the bar: a tile-queue group of eight such invokes (plan_gemm_group; vec = every A and B pointer 16-byte aligned); right
// of it: a single invoke (plan_gemm_call).
#include "gemm_plan.h"
#include <stdio.h>
#include <string.h>

using namespace tpp;

namespace {

const char *instance_name(const GemmLaunch &l) {
  static const char *const names[] = {"f32", "f32_vec", "bf16_vnni2", "bf16_vnni2_vec", "bf16_vnni4_vec", "bf16_flat", "f32_bt_vec", "f32_at_vec", "f32_at"};
  return l.launcher == GL_GENERIC ? names[l.generic] : "-";
}
const char *launcher_name(GemmLauncher l) { return l == GL_GENERIC ? "generic" : l == GL_INVALID ? "invalid" : l == GL_NONE ? "none" : "other"; }

struct Sib {
  bool a, b;
  int mode;
  int64_t m, n, k, lda, ldb, sa = 0, sb = 0;
  int64_t dtype = DT_F32;
  int vnni = 0;
};

// what dt_sibling makes: the dispatched gemm (one batch element) planned as usual, then the operand flag, the source's leading
// dimension, the mode, and the generic kernel forced
void line(const Sib &s) {
  GemmDesc d;
  memset(&d, 0, sizeof(d));
  d.kind = KIND_GEMM;
  d.dtype = s.dtype;
  d.m = s.m, d.n = s.n, d.k = s.k;
  d.lda = s.lda, d.ldb = s.ldb, d.ldc = s.n;
  d.stride_a = s.sa, d.stride_b = s.sb;
  d.beta0 = 1;
  d.vnni_b = s.vnni;
  d.vnni_factor = s.vnni ? 2 : 0;
  const GemmPlanEnv env{256, false, -1};
  plan_gemm(d, -1, env);
  d.a_trans = s.a, d.b_trans = s.b, d.trans_mode = s.mode;
  d.variant = V_GENERIC;
  d.generic_forced = 1;
  for (int vec = 1; vec >= 0; --vec) {
    const GemmLaunch g = plan_gemm_group(d, 8, vec != 0, true, false, 1, env);
    const GemmLaunch c = plan_gemm_call(d, 1, GemmAlign{vec != 0, true, true, true, true}, env);
    printf("%s mode%d %ldx%ldx%ld lda%ld ldb%ld sa%ld sb%ld %s vnni%d vec%d : %s %s \"%s\" | %s %s \"%s\"\n", s.a && s.b ? "AB" : s.a ? "A" : "B", s.mode,
           (long)s.m, (long)s.n, (long)s.k, (long)s.lda, (long)s.ldb, (long)s.sa, (long)s.sb, s.dtype == DT_F32 ? "f32" : "bf16", s.vnni, vec,
           launcher_name(g.launcher), instance_name(g), g.text, launcher_name(c.launcher), instance_name(c), c.text);
  }
}

} // namespace

int main() {
  struct Shape { int64_t m, n, k; };
  const Shape shapes[] = {{32, 32, 64}, {64, 48, 64}, {40, 34, 36}, {36, 48, 40}, {64, 64, 4}, {34, 32, 32}, {32, 32, 30}};
  const int64_t src_ld[] = {512, 52, 50};
  for (const Shape &s : shapes)
    for (int64_t ld : src_ld) {
      // B read transposed: the source holds n rows of k; A as dispatched (rows of 512)
      if (ld >= s.k)
        for (int mode : {1, 2}) line(Sib{false, true, mode, s.m, s.n, s.k, 512, ld});
      // A read transposed: the source holds k rows of m; B as dispatched (rows of n). Mode 1 never makes one: planned all the same
      if (ld >= s.m)
        for (int mode : {1, 2}) line(Sib{true, false, mode, s.m, s.n, s.k, ld, s.n});
    }
  // the other operand's leading dimension and the strides off the 4-float grid, leading dimensions at and beyond 2^24
  for (bool a : {false, true}) {
    line(Sib{a, !a, 2, 32, 32, 64, a ? 512 : 66, a ? 34 : 512});
    line(Sib{a, !a, 2, 32, 32, 64, 512, 512, 2, 0});
    line(Sib{a, !a, 2, 32, 32, 64, 512, 512, 0, 6});
    line(Sib{a, !a, 2, 32, 32, 64, 512, 512, 8, 16});
    line(Sib{a, !a, 2, 32, 32, 64, a ? (1 << 24) - 4 : 512, a ? 512 : (1 << 24) - 4});
    line(Sib{a, !a, 2, 32, 32, 64, a ? (1 << 24) : 512, a ? 512 : (1 << 24)});
    line(Sib{a, !a, 2, 32, 32, 64, a ? 512 : (1 << 24), a ? (1 << 24) : 512});
  }
  // no kernel: bf16, a VNNI B operand, both operands transposed
  for (int mode : {1, 2}) {
    for (bool a : {false, true}) {
      line(Sib{a, !a, mode, 32, 32, 64, 512, 512, 0, 0, DT_BF16, 0});
      line(Sib{a, !a, mode, 32, 32, 64, 512, 512, 0, 0, DT_BF16, 1});
      line(Sib{a, !a, mode, 32, 32, 64, 512, 512, 0, 0, DT_F32, 1});
    }
    line(Sib{true, true, mode, 32, 32, 64, 512, 512});
  }
  return 0;
}
