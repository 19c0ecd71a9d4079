// fake_hip.cpp - TEST INFRASTRUCTURE for tests/test_tsan_scheduler.py, never part of the product library.
//
// runtime.cpp (the C-ABI layer: tile queue, multi-producer ring, scheduler thread, host-operand mirroring) is
// compiled unchanged with g++ -fsanitize=thread and linked against THIS file instead of libamdhip64 and the
// gfx950 kernels, so that ThreadSanitizer can watch the host-side concurrency on a machine without a GPU:
//   * the HIP host entry points runtime.cpp uses, over plain host memory: fake_hip_host.h, shared with the host
//     build of the layer-chain launch decision (tests/chain_dispatch/fake_chain.cpp);
//   * the 7 launch / plan functions of xsmm_desc.h as scalar f32 loops executed on the launching thread
//     (so a launch that touches bytes another thread is using IS a data race TSAN reports).
#include "../../tpp-mlir_amd/csrc/xsmm_desc.h"
#include "../../tpp-mlir_amd/csrc/chain_args.h"
#include "../../tpp-mlir_amd/csrc/gemm_plan.h"
#include "fake_hip_host.h"

namespace tpp {

// FAKE_HIP_NO_COMPUTE=1: launches return at once (host-side throughput runs of the enqueue path, e.g. tools/tpp_replay
// built against this file; results are then meaningless)
static const bool g_compute = getenv("FAKE_HIP_NO_COMPUTE") == nullptr;

bool plan_gemm(GemmDesc &d, int) {
  d.variant = 0;
  strcpy(d.name, "fake_host_gemm");
  return d.dtype == DT_F32 && !d.vnni_b && !d.vnni_c;
}

hipError_t launch_gemm(const GemmDesc &d, const void *A_, const void *B_, void *C_, const void *D_, int64_t br, hipStream_t) {
  const float *A = (const float *)A_, *B = (const float *)B_, *D = (const float *)D_;
  float *C = (float *)C_;
  if (!g_compute) return hipSuccess;
  for (int64_t i = 0; i < d.m; ++i)
    for (int64_t j = 0; j < d.n; ++j) {
      float acc = d.beta0 ? 0.0f : C[i * d.ldc + j];
      for (int64_t b = 0; b < br; ++b)
        for (int64_t kk = 0; kk < d.k; ++kk)
          acc += A[b * d.stride_a + i * d.lda + kk] * (d.b_trans ? B[b * d.stride_b + j * d.ldb + kk] : B[b * d.stride_b + kk * d.ldb + j]);
      if (d.bias) acc += D[j];
      if (d.relu && !(acc > 0.0f)) acc = 0.0f;
      C[i * d.ldc + j] = acc;
    }
  return hipSuccess;
}
// THIS build never reaches a chain launch: plan_gemm above refuses bf16 and runtime.cpp's weak stand-in of plan_chain refuses every chain,
// so try_chain_launch ends behind the chain contract. The host build that runs it to the end - the real gemm_plan.cpp, computing and recording
// stand-ins of all nine launch forms - is tests/chain_dispatch/fake_chain.cpp (tests/test_chain_dispatch.py).
hipError_t launch_bf16_chain(int, int, int, const ChainArgs &, hipStream_t) { return hipErrorNotSupported; }
int force_gemm_split(int) { return -1; }
static bool g_fake_strict = false;
int set_strict_kernels(int on) { const int prev = g_fake_strict; g_fake_strict = on != 0; return prev; }
bool strict_kernels() { return g_fake_strict; }
hipError_t launch_f32_chain(int, const ChainArgs &, hipStream_t) { return hipErrorNotSupported; }
const char *last_grouped_kernel() { return "fake_host_gemm"; }
const char *last_refined_kernel() { return ""; }
hipError_t launch_gemm_grouped(const GemmDesc &d, const WorkItem *it, int n, bool, bool, bool, int64_t, hipStream_t s) {
  for (int i = 0; i < n; ++i) (void)launch_gemm(d, it[i].A, it[i].B, it[i].C, it[i].D, it[i].br, s);
  return hipSuccess;
}
bool gemm_quads_pay(const GemmDesc &, int, int64_t) { return false; } // (plan_gemm above refuses bf16: no quads on the host stand-in)
hipError_t launch_gemm_quads(const GemmDesc &, const QuadItem *, int, int64_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_unary(const UnaryDesc &d, const void *in_, float scalar, bool use_scalar, void *out_, hipStream_t) {
  const float *in = (const float *)in_;
  float *out = (float *)out_;
  if (!g_compute) return hipSuccess;
  if (d.op == 29) { // transpose: m x n in, n x m out
    for (int64_t i = 0; i < d.m; ++i)
      for (int64_t j = 0; j < d.n; ++j) out[j * d.ldo + i] = in[i * d.ldi + j];
    return hipSuccess;
  }
  if (d.dtype == DT_BF16) { // identity / zero / relu on raw bf16 words (the host-cache driver's copy-path cases; no arithmetic)
    if (use_scalar || (d.op != 1 && d.op != 2 && d.op != 5)) return hipErrorNotSupported;
    const uint16_t *hi = (const uint16_t *)in_;
    uint16_t *ho = (uint16_t *)out_;
    for (int64_t i = 0; i < d.m; ++i)
      for (int64_t j = 0; j < d.n; ++j) {
        const uint16_t w = d.op == 2 ? 0 : hi[i * d.ldi + j];
        const bool positive = !(w & 0x8000) && (w & 0x7fff) != 0 && !((w & 0x7f80) == 0x7f80 && (w & 0x7f)); // > 0, not NaN
        ho[i * d.ldo + j] = d.op == 5 && !positive ? 0 : w;
      }
    return hipSuccess;
  }
  for (int64_t i = 0; i < d.m; ++i)
    for (int64_t j = 0; j < d.n; ++j) {
      float v = d.op == 2 ? 0.0f : (use_scalar ? scalar : in[i * d.ldi + j]);
      if (d.op == 5 && !(v > 0.0f)) v = 0.0f;
      out[i * d.ldo + j] = v;
    }
  return hipSuccess;
}
hipError_t launch_unary_grouped(const UnaryDesc &d, const WorkItem *it, int n, hipStream_t s) {
  for (int i = 0; i < n; ++i) (void)launch_unary(d, it[i].A, 0.0f, false, it[i].C, s);
  return hipSuccess;
}
hipError_t launch_binary(const BinaryDesc &d, const void *l_, const void *r_, void *out_, hipStream_t) {
  const float *l = (const float *)l_, *r = (const float *)r_;
  float *out = (float *)out_;
  if (!g_compute) return hipSuccess;
  for (int64_t i = 0; i < d.m; ++i)
    for (int64_t j = 0; j < d.n; ++j) {
      // broadcast flags (XsmmEnum.td:58-70): ROW = one value per row, COL = one row of n values, SCALAR = one value
      const float a = d.flags & 16 ? l[0] : d.flags & 4 ? l[j] : d.flags & 1 ? l[i * d.ldi_lhs] : l[i * d.ldi_lhs + j];
      const float b = d.flags & 32 ? r[0] : d.flags & 8 ? r[j] : d.flags & 2 ? r[i * d.ldi_rhs] : r[i * d.ldi_rhs + j];
      out[i * d.ldo + j] = d.op == 1 ? a + b : d.op == 2 ? a * b : d.op == 3 ? a - b : a / b;
    }
  return hipSuccess;
}
hipError_t launch_binary_grouped(const BinaryDesc &d, const WorkItem *it, int n, hipStream_t s) {
  for (int i = 0; i < n; ++i) (void)launch_binary(d, it[i].A, it[i].B, it[i].C, s);
  return hipSuccess;
}

} // namespace tpp
