// fake_skinny_chain.cpp - TEST INFRASTRUCTURE for tests/test_chain_skinny_dispatch.py, never part of the product library.
//
// The stand-in of launch_bf16_skinny_chain (brgemm_bf16_skinny_chain.hip) for the host build of tests/chain_dispatch: it refuses what the real
// launcher refuses, records the argument block, runs THE COUNTER MODEL - every workgroup of the launch walks the schedule header
// (brgemm_bf16_skinny_chain.h) and arrives where the kernel arrives; before the stand-in adds the arrivals every seam counter must hold target -
// arrivals and lie inside the block the argument block points to - and computes layer by layer through oracle/xsmm_oracle.c from the
// ChainArgs ALONE, what the kernel sees. A starved launch writes its error word (host memory here) and stores nothing.
#include "fake_skinny_chain.h"
#include "../../tpp-mlir_amd/csrc/brgemm_bf16_skinny_chain.h"
#include <cstdio>
#include <vector>

extern "C" {
int oracle_set_vnni_factor(int v);
int oracle_fused_brgemm(int64_t dt, int64_t m, int64_t n, int64_t k, int64_t lda, int64_t ldb, int64_t ldc, int64_t stride_a, int64_t stride_b,
                        int64_t gemm_flags, int64_t unary_flags, int64_t unary_kind, int64_t binary_flags, int64_t binary_kind, const void *A,
                        const void *B, void *C, const void *D, int64_t br);
}

namespace {
std::vector<FakeSkinnyLaunch> g_launches;
int g_starve_in = 0, g_starve_layer = 0, g_mismatches = 0;

void counter_model(int bn, const tpp::ChainArgs &a) {
  const int G = a.groups;
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  const bool known = hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)a.cnt) == hipSuccess;
  for (int l = 0; l + 1 < a.nlayers; ++l) {
    unsigned *c = a.cnt + (size_t)l * tpp::CHAIN_CNT_STRIDE;
    if (!known || (uintptr_t)(c + 1) > (uintptr_t)base + size) {
      if (g_mismatches++ < 8) fprintf(stderr, "COUNTER MODEL: skinny launch: counter [%d] lies outside its block\n", l);
      continue;
    }
    // every workgroup walks its blocks of the layer and arrives behind the last one, or at once
    unsigned arrivals = 0;
    const int blocks = tpp::skn_blocks(a.L[l].pad, bn);
    for (int w = 0; w < G; ++w) {
      const int owned = tpp::skc_owned(w, G, blocks);
      for (int i = -1; i < owned; ++i)
        if (tpp::skc_signals(l, a.nlayers) && i == tpp::skc_arrive_after(w, G, blocks)) ++arrivals;
    }
    if (*c + arrivals != a.target || arrivals != tpp::skc_arrivals(G)) {
      if (g_mismatches++ < 8)
        fprintf(stderr, "COUNTER MODEL: skinny launch (m %d layers %d G %d target %u): cnt[%d] = %u, + %u arrivals != %u waited for\n", a.m, a.nlayers, G, a.target, l,
                *c, arrivals, a.target);
    }
    *c += arrivals;
  }
}
} // namespace

extern "C" {
int fake_skinny_launches(void) { return (int)g_launches.size(); }
const FakeSkinnyLaunch *fake_skinny_launch(int i) { return i >= 0 && i < (int)g_launches.size() ? &g_launches[i] : nullptr; }
void fake_skinny_clear(void) { g_launches.clear(); }
void fake_skinny_starve(int nth, int layer) { g_starve_in = nth, g_starve_layer = layer; }
int fake_skinny_counter_mismatches(void) { return g_mismatches; }
}

namespace tpp {

hipError_t launch_bf16_skinny_chain(int b_kind, int bn, const ChainArgs &a, hipStream_t) {
  // (the real launcher's refusals, brgemm_bf16_skinny_chain.hip)
  if (!skn_instance_exists(b_kind, bn) || !skc_launch_shape_ok(a.nlayers, a.groups) || !a.cnt || !a.err || !a.A || ((uintptr_t)a.A & 15)) return hipErrorInvalidValue;
  for (int l = 0; l < a.nlayers; ++l) {
    const ChainLayer &L = a.L[l];
    const int64_t lda = l == 0 ? a.lda : a.L[l - 1].ldc;
    if (!skn_shape_ok(a.m, L.pad, L.k, L.br, bn) || !skc_ld_ok(lda, L.ldb, L.ldc, L.stride_a, L.stride_b, L.pad, L.k)) return hipErrorInvalidValue;
    if (!(L.ep & EP_BETA0) || (L.ep & EP_VNNI_C) || !L.B || !L.C || (((uintptr_t)L.B | (uintptr_t)L.C) & 15)) return hipErrorInvalidValue;
    if ((L.ep & EP_BIAS) && (!L.D || ((uintptr_t)L.D & 7))) return hipErrorInvalidValue;
    if (l > 0 && (int64_t)(L.br - 1) * L.stride_a + L.k > lda) return hipErrorInvalidValue;
  }
  FakeSkinnyLaunch rec{b_kind, bn, a, 0};
  if (g_starve_in > 0 && --g_starve_in == 0) {
    rec.starved = 1;
    g_launches.push_back(rec);
    *a.err = 1u + (unsigned)g_starve_layer;
    return hipSuccess;
  }
  g_launches.push_back(rec);
  counter_model(bn, a);
  for (int l = 0; l < a.nlayers; ++l) {
    const ChainLayer &L = a.L[l];
    if (b_kind != 2) oracle_set_vnni_factor(b_kind == 4 ? 4 : 2);
    const int64_t flags = 4 | (b_kind != 2 ? 2048 : 0);
    const bool bias = (L.ep & EP_BIAS) != 0, relu = (L.ep & EP_RELU) != 0;
    if (oracle_fused_brgemm(DT_BF16, a.m, L.pad, L.k, l == 0 ? a.lda : a.L[l - 1].ldc, L.ldb, L.ldc, L.stride_a, L.stride_b, flags, 0, relu ? 5 : 0, bias ? 4 : 0,
                            bias ? 1 : 0, l == 0 ? a.A : a.L[l - 1].C, L.B, L.C, L.D, L.br))
      return hipErrorInvalidValue;
  }
  return hipSuccess;
}

} // namespace tpp
