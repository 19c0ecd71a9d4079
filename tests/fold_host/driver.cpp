// driver.cpp - TEST INFRASTRUCTURE (tests/test_fold_epilogue_host.py): the epilogue fold's eligibility rules (rt_tile_queue.h
// try_fold) on the host. runtime.cpp is compiled unchanged against tests/tsan/fake_hip.cpp (the HIP host API and the kernel launchers
// over host memory); this file adds the host stand-in of the epilogue-program launcher (f32), so the queue folds here as it does on
// the GPU. Every case is an invoke sequence run twice on fresh buffers - fold on, fold off - and checked for: the same bytes, and the
// expected folded / declined / ended-group decisions (xsmm_hip_fold_epilogue_stats, xsmm_hip_tile_queue_stats). Prints OK at the end.
#include "../../include/tpp_xsmm_abi.h"
#include "../../tpp-mlir_amd/csrc/xsmm_desc.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>



namespace tpp {
hipError_t launch_postop_grouped(const PostProgram &p, const PostItem *items, int n_items, hipStream_t) {
  if (p.dtype != DT_F32 || p.n < 1 || p.n > 2) return hipErrorInvalidValue;
  for (int it = 0; it < n_items; ++it) {
    const PostItem &e = items[it];
    std::vector<float> x((size_t)p.m * p.cols);
    for (int i = 0; i < p.m; ++i)
      for (int j = 0; j < p.cols; ++j) x[(size_t)i * p.cols + j] = ((const float *)e.C)[i * p.ldc + j];
    for (int s = 0; s < p.n; ++s) {
      const PostOp &o = p.op[s];
      for (int i = 0; i < p.m; ++i)
        for (int j = 0; j < p.cols; ++j) {
          float &v = x[(size_t)i * p.cols + j];
          if (o.op == PO_ZERO) v = 0.0f;
          else if (o.op == PO_RELU) v = v > 0.0f ? v : 0.0f;
          else if (o.op != PO_IDENTITY) {
            const float *q = (const float *)e.other[s];
            const float y = o.bc == 0 ? q[i * o.ld + j] : o.bc == 1 ? q[i * o.ld] : o.bc == 2 ? q[j] : q[0];
            const float a = o.pos == 0 ? v : y, b = o.pos == 0 ? y : v;
            v = o.op == PO_ADD ? a + b : o.op == PO_MUL ? a * b : o.op == PO_SUB ? a - b : a / b;
          }
          if (s == 1 || p.n == 1 || e.out[1] != e.out[0]) ((float *)e.out[s])[i * o.ldo + j] = v;
        }
    }
  }
  return hipSuccess;
}
} // namespace tpp

static const int T = 32, NT = 16, TS = T * T; // 16 tiles of 32 x 32, packed [NT][32][32]
static int failures = 0;
#define CHECK(c, ...)                                                                                                               \
  do {                                                                                                                              \
    if (!(c)) {                                                                                                                     \
      ++failures;                                                                                                                   \
      printf("FAIL %s:%d: ", __FILE__, __LINE__);                                                                                   \
      printf(__VA_ARGS__);                                                                                                          \
      printf("\n");                                                                                                                 \
    }                                                                                                                               \
  } while (0)

static float *dev_alloc(size_t n) {
  void *p = nullptr;
  if (hipMalloc(&p, n * sizeof(float)) != 0) abort();
  return (float *)p;
}
struct Bufs { // one allocation per case: O (separate outputs) lies BELOW C in memory
  float *base, *O, *C, *A, *W, *R, *X;
  size_t n;
  explicit Bufs(unsigned seed) {
    n = (size_t)NT * TS * 6 + 64;
    base = dev_alloc(n);
    O = base, C = O + NT * TS, A = C + NT * TS, W = A + NT * TS, R = W + NT * TS, X = R + NT * TS;
    for (size_t i = 0; i < n; ++i) {
      seed = seed * 1664525u + 1013904223u;
      base[i] = (float)((int)((seed >> 16) & 7) - 3);
    }
  }
};
struct Delta {
  int64_t folded, groups, declined, launches;
};
static Delta run_case(bool fold, const std::function<void(Bufs &)> &body, std::vector<float> &out) {
  xsmm_hip_set_fold_epilogue(fold);
  Bufs b(7);
  int64_t f0[3], f1[3], q0[5], q1[5];
  xsmm_hip_flush();
  xsmm_hip_fold_epilogue_stats(f0);
  xsmm_hip_tile_queue_stats(q0);
  body(b);
  xsmm_hip_flush();
  xsmm_hip_synchronize();
  xsmm_hip_fold_epilogue_stats(f1);
  xsmm_hip_tile_queue_stats(q1);
  out.assign(b.base, b.base + b.n);
  return Delta{f1[0] - f0[0], f1[1] - f0[1], f1[2] - f0[2], q1[0] - q0[0]};
}
static Delta both(const char *name, const std::function<void(Bufs &)> &body) {
  std::vector<float> on, off;
  const Delta d = run_case(true, body, on);
  (void)run_case(false, body, off);
  CHECK(memcmp(on.data(), off.data(), on.size() * sizeof(float)) == 0, "%s: fold on and off differ", name);
  printf("%-44s folded %3ld  epilogue launches %2ld  declined %2ld  queue launches %3ld\n", name, (long)d.folded, (long)d.groups,
         (long)d.declined, (long)d.launches);
  return d;
}

int main() {
  xsmm_hip_set_async(1);
  xsmm_hip_set_tile_queue(1);
  const int64_t g = xsmm_gemm_dispatch(1, T, T, T, T, T, T, 4);                              // C = A W (beta 0)
  const int64_t add = xsmm_binary_dispatch(1, 1, T, T, T, T, T, 0);                          // tile + residual
  const int64_t mul = xsmm_binary_dispatch(2, 1, T, T, T, T, T, 0);                         // tile * scale
  // (no broadcast forms here: fake_hip.cpp's element-wise stand-ins ignore broadcast flags; the GPU tests cover them)
  const int64_t half = xsmm_binary_dispatch(1, 1, T / 2, T, T, T, T, 0);                     // half a tile
  const int64_t relu = xsmm_unary_dispatch(5, 1, T, T, T, T, 0), zero = xsmm_unary_dispatch(2, 1, T, T, T, T, 0);
  const int64_t relu_row = xsmm_unary_dispatch(5, 1, T, T, T, T, 2);                         // a broadcast unary: never folded
  auto gemm = [&](Bufs &b, int t) { xsmm_gemm_invoke(1, g, b.A, t * TS, b.W, 0, b.C, t * TS); };
  Delta d;

  for (int iters : {1, 3}) { // the recording pass, then replays of the recorded group
    char nm[64];
    snprintf(nm, sizeof nm, "residual in place, %d iteration(s)", iters);
    d = both(nm, [&](Bufs &b) {
      for (int it = 0; it < iters; ++it)
        for (int t = 0; t < NT; ++t) {
          gemm(b, t);
          xsmm_binary_invoke(1, add, b.R, t * TS, b.C, t * TS, b.C, t * TS); // (the tile in position 1)
        }
    });
    CHECK(d.folded == NT * iters && d.declined == 0 && d.launches == iters && d.groups == iters, "%s", nm);
  }
  d = both("bias + relu, separate outputs below C, x3", [&](Bufs &b) {
    for (int it = 0; it < 3; ++it)
      for (int t = 0; t < NT; ++t) {
        gemm(b, t);
        xsmm_binary_invoke(1, add, b.C, t * TS, b.R, t * TS, b.O, t * TS);
        xsmm_unary_invoke(1, relu, b.O, t * TS, b.O, t * TS);
      }
  });
  CHECK(d.folded == 2 * NT * 3 && d.declined == 0 && d.launches == 3, "bias + relu separate");
  d = both("zero whose input pointer is another buffer, x3", [&](Bufs &b) {
    for (int it = 0; it < 3; ++it)
      for (int t = 0; t < NT; ++t) {
        gemm(b, t);
        xsmm_unary_invoke(1, zero, b.X, t * TS, b.C, t * TS); // (a zero reads nothing: it continues the tile it overwrites)
      }
  });
  CHECK(d.folded == NT * 3 && d.declined == 0 && d.launches == 3, "zero, other input");
  d = both("zero whose input pointer is another item's C, x3", [&](Bufs &b) {
    for (int it = 0; it < 3; ++it)
      for (int t = 0; t < NT; ++t) {
        gemm(b, t);
        xsmm_unary_invoke(1, zero, b.C, ((t + 1) % NT) * TS, b.C, t * TS);
      }
  });
  CHECK(d.folded == NT * 3 && d.launches == 3, "zero, neighbour's input");
  d = both("scale then residual, tile in both positions", [&](Bufs &b) {
    for (int t = 0; t < NT; ++t) {
      gemm(b, t);
      xsmm_binary_invoke(1, mul, b.C, t * TS, b.X, t * TS, b.C, t * TS);
      xsmm_binary_invoke(1, add, b.R, t * TS, b.C, t * TS, b.C, t * TS);
    }
  });
  CHECK(d.folded == 2 * NT && d.declined == 0 && d.launches == 1, "two stages");

  // declines: each flushes the group (as without the fold) and counts
  d = both("partial tile", [&](Bufs &b) {
    for (int t = 0; t < NT; ++t) gemm(b, t);
    xsmm_binary_invoke(1, half, b.C, 0, b.R, 0, b.C, 0);
  });
  CHECK(d.folded == 0 && d.declined == 1, "partial tile");
  d = both("other operand written by a queued item", [&](Bufs &b) {
    for (int t = 0; t < NT; ++t) gemm(b, t);
    xsmm_binary_invoke(1, add, b.C, 0, b.C, TS, b.C, 0);
  });
  CHECK(d.folded == 0 && d.declined == 1, "other operand queued");
  d = both("output over another item's operand", [&](Bufs &b) {
    for (int t = 0; t < NT; ++t) gemm(b, t);
    xsmm_binary_invoke(1, add, b.C, 0, b.R, 0, b.A, TS);
  });
  CHECK(d.folded == 0 && d.declined == 1, "output over A");
  d = both("output overlapping its own other operand", [&](Bufs &b) {
    for (int t = 0; t < NT; ++t) gemm(b, t);
    xsmm_binary_invoke(1, add, b.C, 0, b.R, 0, b.R, 8);
  });
  CHECK(d.folded == 0 && d.declined == 1, "output over other");
  d = both("broadcast unary", [&](Bufs &b) {
    for (int t = 0; t < NT; ++t) gemm(b, t);
    xsmm_unary_invoke(1, relu_row, b.C, 0, b.C, 0);
  });
  CHECK(d.folded == 0 && d.declined == 1, "broadcast unary");
  d = both("third post-op", [&](Bufs &b) {
    for (int t = 0; t < NT; ++t) gemm(b, t);
    for (int k = 0; k < 3; ++k) xsmm_unary_invoke(1, relu, b.C, 0, b.C, 0);
  });
  CHECK(d.folded == 2 && d.declined == 1, "third post-op");
  d = both("another stream", [&](Bufs &b) {
    for (int t = 0; t < NT; ++t) gemm(b, t);
    xsmm_hip_set_stream((void *)0x1000);
    xsmm_unary_invoke(1, relu, b.C, 0, b.C, 0);
    xsmm_hip_set_stream(nullptr);
  });
  CHECK(d.folded == 0, "another stream"); // (changing the stream is a synchronisation point: the group is launched before the relu)
  d = both("another program ends the group", [&](Bufs &b) {
    for (int t = 0; t < NT; ++t) {
      gemm(b, t);
      xsmm_unary_invoke(1, t < NT / 2 ? relu : zero, b.C, t * TS, b.C, t * TS);
    }
  });
  CHECK(d.folded == NT - 1 && d.declined == 1 && d.launches >= 2, "program change"); // (the first zero ends the relu group; the rest fold into the next)
  xsmm_hip_set_async(0);
  d = both("synchronous mode", [&](Bufs &b) {
    for (int t = 0; t < NT; ++t) {
      gemm(b, t);
      xsmm_unary_invoke(1, relu, b.C, t * TS, b.C, t * TS);
    }
  });
  CHECK(d.folded == 0 && d.declined == 0, "sync mode");
  if (failures) {
    printf("%d FAILURES\n", failures);
    return 1;
  }
  printf("OK\n");
  return 0;
}
