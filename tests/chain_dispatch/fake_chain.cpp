// fake_chain.cpp - TEST INFRASTRUCTURE for tests/test_chain_dispatch.py, never part of the product library.
//
// The host build that REACHES the layer-chain launch decision (rt_chain.h try_chain_launch): runtime.cpp, host_cache.cpp and the real
// planner gemm_plan.cpp are compiled unchanged with g++ and linked against this file instead of libamdhip64 and the gfx950 kernels.
// (The other host build, tests/tsan/fake_hip.cpp, plans every bf16 descriptor away and links runtime.cpp's weak refusing stand-ins:
// there a chain never gets past the first rule.)
//   * the HIP host entry points: tests/tsan/fake_hip_host.h, FAKE_HIP_CUS compute units;
//   * plan_gemm / gemm_quads_pay through the real planner, with a GemmPlanEnv filled by the fill brgemm_f32.hip uses (mode_switches.h gemm_plan_env_of);
//   * launch_gemm and the nine chain launchers COMPUTE through oracle/xsmm_oracle.c (oracle_fused_brgemm): a single call from its
//     GemmDesc, a chain layer by layer from the ChainArgs ALONE - what the kernels see. Each launcher first asks the refusal function
//     of its launch mode (brgemm_bf16_lw_launch.h, brgemm_bf16_dma256_chain.h) and answers hipErrorInvalidValue as the real one does;
//   * one record per launch (fake_chain.h), and a COUNTER MODEL: before a chain stand-in returns, every hand-off counter of the launch
//     must hold expected_after - arrivals - both taken from the project's CPU-walkable schedule headers - and lie inside the block
//     the argument block points to; then the stand-in adds the arrivals. A mismatch is what on the device is a launch that times out
//     (too few arrivals expected) or a consumer that does not wait (the counter is already past the target);
//   * fake_chain_starve: a launch that writes its error word and stores nothing (host memory here: nothing is provoked anywhere).
#include "fake_chain.h"
#include "../../tpp-mlir_amd/csrc/gemm_plan.h"
#include "../../tpp-mlir_amd/csrc/mode_switches.h"
#include "../../tpp-mlir_amd/csrc/brgemm_bf16_lw_chain_edge.h"
#include "../../tpp-mlir_amd/csrc/brgemm_bf16_lw_chain_rounds.h"
#include "../../tpp-mlir_amd/csrc/brgemm_bf16_lw_chain_ragged.h"
#include "../../tpp-mlir_amd/csrc/brgemm_bf16_lw_chain_widths.h"
#include "../../tpp-mlir_amd/csrc/brgemm_bf16_lw_chain_wrounds.h"
#include "../../tpp-mlir_amd/csrc/brgemm_bf16_lw_chain_wragged.h"
#include "../../tpp-mlir_amd/csrc/brgemm_bf16_dma256_chain.h"
#include "../tsan/fake_hip_host.h"
#include <atomic>
#include <cstdio>
#include <vector>

extern "C" {
int oracle_set_vnni_factor(int v);
int oracle_fused_brgemm(int64_t dt, int64_t m, int64_t n, int64_t k, int64_t lda, int64_t ldb, int64_t ldc, int64_t stride_a, int64_t stride_b,
                        int64_t gemm_flags, int64_t unary_flags, int64_t unary_kind, int64_t binary_flags, int64_t binary_kind, const void *A,
                        const void *B, void *C, const void *D, int64_t br);
}

namespace {
std::vector<FakeChainLaunch> g_launches;
std::vector<FakeGemmLaunch> g_gemms;
bool g_compute = true;
int g_starve_in = 0, g_starve_layer = 0;
int g_mismatches = 0;
std::atomic<int> g_forced_split{-1};
std::atomic<int> g_strict_kernels{0};

// one layer through the oracle. b_kind: 0 VNNI-2, 2 flat, 4 VNNI-4 (bf16); f32 is flat
int oracle_layer(int64_t dt, int b_kind, int64_t m, int64_t n, int64_t k, int64_t lda, int64_t ldb, int64_t ldc, int64_t sa, int64_t sb, bool beta0, bool bias,
                 bool relu, bool vnni_c, const void *A, const void *B, void *C, const void *D, int64_t br) {
  if (b_kind == 4 || b_kind == 0) oracle_set_vnni_factor(b_kind == 4 ? 4 : 2);
  const int64_t flags = (beta0 ? 4 : 0) | (dt == tpp::DT_BF16 && b_kind != 2 ? 2048 : 0) | (vnni_c ? 8192 : 0);
  return oracle_fused_brgemm(dt, m, n, k, lda, ldb, ldc, sa, sb, flags, 0, relu ? 5 : 0, bias ? 4 : 0, bias ? 1 : 0, A, B, C, D, br);
}

// THE COUNTER MODEL. arrivals[l][tm]: what this launch adds to cnt[l][tm]; expected[l]: what the launch's consumers wait for there.
struct Seams {
  int tiles_m;
  std::vector<std::vector<unsigned>> arrivals; // [nlayers - 1][tiles_m]
  std::vector<unsigned> expected;              // [nlayers - 1]
};
void run_counter_model(const char *form, const tpp::ChainArgs &a, const Seams &s) {
  uintptr_t base = 0;
  size_t size = 0;
  const bool known = find_alloc(a.cnt, &base, &size);
  for (int l = 0; l + 1 < a.nlayers; ++l)
    for (int tm = 0; tm < s.tiles_m; ++tm) {
      unsigned *c = a.cnt + ((size_t)l * s.tiles_m + tm) * tpp::CHAIN_CNT_STRIDE;
      if (!known || (uintptr_t)(c + 1) > base + size) {
        if (g_mismatches++ < 8) fprintf(stderr, "COUNTER MODEL: %s launch: counter [%d][%d] lies outside its block\n", form, l, tm);
        continue;
      }
      const unsigned arr = s.arrivals[l][tm];
      if (*c + arr != s.expected[l]) {
        if (g_mismatches++ < 8)
          fprintf(stderr, "COUNTER MODEL: %s launch (m %d n %d layers %d groups %d target %u): cnt[%d][%d] = %u, + %u arrivals != %u waited for\n", form,
                  a.m, a.n, a.nlayers, a.groups, a.target, l, tm, *c, arr, s.expected[l]);
      }
      *c += arr;
    }
}
Seams uniform_seams(const tpp::ChainArgs &a, int tiles_m, unsigned per_counter) {
  Seams s{tiles_m, {}, {}};
  for (int l = 0; l + 1 < a.nlayers; ++l) {
    s.arrivals.push_back(std::vector<unsigned>(tiles_m, per_counter));
    s.expected.push_back(a.target);
  }
  return s;
}
// row rounds (brgemm_bf16_lw_chain_rounds.h; the 256x256 tile's chain walks the same way): every resident workgroup (g, tn) walks
// chain_rounds_next from (tm = g, l = 0) and arrives once per step of a layer that is not the last
Seams row_round_seams(const tpp::ChainArgs &a, int tiles_m, int tiles_n, int G) {
  Seams s = uniform_seams(a, tiles_m, 0);
  for (int g = 0; g < G && g < tiles_m; ++g)
    for (int tn = 0; tn < tiles_n; ++tn) {
      int tm = g, l = 0, steps = 0;
      while (l < a.nlayers && steps++ < 1 << 24) {
        if (l + 1 < a.nlayers) ++s.arrivals[l][tm];
        tpp::chain_rounds_next(tm, l, G, tiles_m);
      }
    }
  return s;
}

struct Starve { bool now; int layer; };
Starve take_starve() {
  if (g_starve_in > 0 && --g_starve_in == 0) return Starve{true, g_starve_layer};
  return Starve{false, 0};
}

// the layers of a launch from the argument block alone; n_of(l): the layer's columns
hipError_t run_chain(int form, int tile, int b_kind, int bm, int bn, int tiles_m, int grid_n, long long grid, const tpp::ChainArgs &a, const Seams &seams, int64_t dt) {
  FakeChainLaunch rec{form, tile, b_kind, bm, bn, tiles_m, grid_n, grid, a, 0};
  const Starve st = take_starve();
  if (st.now) {
    rec.starved = 1;
    g_launches.push_back(rec);
    *a.err = 1u + (unsigned)st.layer;
    return hipSuccess;
  }
  g_launches.push_back(rec);
  run_counter_model(fake_chain_form_name(form), a, seams);
  if (!g_compute) return hipSuccess;
  for (int l = 0; l < a.nlayers; ++l) {
    const tpp::ChainLayer &L = a.L[l];
    const void *A = l == 0 ? a.A : a.L[l - 1].C;
    const int64_t lda = l == 0 ? a.lda : a.L[l - 1].ldc;
    const int n_l = L.pad ? L.pad : a.n;
    if (oracle_layer(dt, b_kind, a.m, n_l, L.k, lda, L.ldb, L.ldc, L.stride_a, L.stride_b, (L.ep & tpp::EP_BETA0) != 0, (L.ep & tpp::EP_BIAS) != 0,
                     (L.ep & tpp::EP_RELU) != 0, (L.ep & tpp::EP_VNNI_C) != 0, A, L.B, L.C, L.D, L.br))
      return hipErrorInvalidValue;
  }
  return hipSuccess;
}
tpp::BlwShape blw_shape(const tpp::ChainArgs &a) {
  tpp::BlwShape s{};
  s.chain = true;
  s.m = a.m, s.n = a.n, s.nlayers = a.nlayers, s.groups = a.groups;
  for (int l = 0; l < a.nlayers && l < tpp::BLW_MAXL; ++l) s.k[l] = a.L[l].k, s.br[l] = a.L[l].br;
  return s;
}
tpp::BlwWidthsShape blw_widths_shape(const tpp::ChainArgs &a) {
  tpp::BlwWidthsShape s{};
  s.m = a.m, s.nlayers = a.nlayers;
  for (int l = 0; l < a.nlayers && l < tpp::BLW_MAXL; ++l) s.n[l] = a.L[l].pad, s.k[l] = a.L[l].k, s.br[l] = a.L[l].br;
  return s;
}
} // namespace

extern "C" {
int fake_chain_launches(void) { return (int)g_launches.size(); }
const FakeChainLaunch *fake_chain_launch(int i) { return i >= 0 && i < (int)g_launches.size() ? &g_launches[i] : nullptr; }
int fake_gemm_launches(void) { return (int)g_gemms.size(); }
const FakeGemmLaunch *fake_gemm_launch(int i) { return i >= 0 && i < (int)g_gemms.size() ? &g_gemms[i] : nullptr; }
void fake_chain_clear(void) { g_launches.clear(); g_gemms.clear(); }
void fake_chain_set_compute(int on) { g_compute = on != 0; }
void fake_chain_starve(int nth, int layer) { g_starve_in = nth; g_starve_layer = layer; }
int fake_chain_counter_mismatches(void) { return g_mismatches; }
int fake_hip_compute_units(void) { return fake_hip_cus(); }
}

namespace tpp {

static GemmPlanEnv fake_plan_env() { // (brgemm_f32.hip gemm_plan_env, with the fake device's compute units)
  return gemm_plan_env_of(fake_hip_cus(), strict_kernels(), g_forced_split.load(std::memory_order_relaxed));
}
bool plan_gemm(GemmDesc &d, int forced_variant) { return plan_gemm(d, forced_variant, fake_plan_env()); }
bool gemm_quads_pay(const GemmDesc &d, int n_items, int64_t br) { return gemm_quads_pay(d, n_items, br, fake_plan_env()); }
int force_gemm_split(int v) { return g_forced_split.exchange(v < -1 ? -1 : v); }
int set_strict_kernels(int on) { return g_strict_kernels.exchange(on != 0); }
bool strict_kernels() { return g_strict_kernels.load(std::memory_order_relaxed) != 0; }
const char *last_grouped_kernel() { return ""; }
const char *last_refined_kernel() { return ""; }

// a single call, from its descriptor (the transposed siblings of deferred transposes never reach this build's drivers)
hipError_t launch_gemm(const GemmDesc &d, const void *A, const void *B, void *C, const void *D, int64_t br, hipStream_t) {
  if (d.b_trans || d.a_trans) return hipErrorNotSupported;
  g_gemms.push_back(FakeGemmLaunch{&d, A, B, D, C, (long long)br});
  if (!g_compute) return hipSuccess;
  const int b_kind = d.dtype == DT_BF16 ? (d.vnni_b ? (d.vnni_factor == 4 ? 4 : 0) : 2) : 2;
  return oracle_layer(d.dtype, b_kind, d.m, d.n, d.k, d.lda, d.ldb, d.ldc, d.stride_a, d.stride_b, d.beta0, d.bias, d.relu, d.vnni_c, A, B, C, D, br) ? hipErrorInvalidValue
                                                                                                                                                       : hipSuccess;
}
hipError_t launch_gemm_grouped(const GemmDesc &d, const WorkItem *it, int n, bool, bool, bool, int64_t, hipStream_t s) {
  for (int i = 0; i < n; ++i)
    if (launch_gemm(d, it[i].A, it[i].B, it[i].C, it[i].D, it[i].br, s) != hipSuccess) return hipErrorInvalidValue;
  return hipSuccess;
}
hipError_t launch_gemm_quads(const GemmDesc &, const QuadItem *, int, int64_t, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_unary(const UnaryDesc &, const void *, float, bool, void *, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_unary_grouped(const UnaryDesc &, const WorkItem *, int, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_binary(const BinaryDesc &, const void *, const void *, void *, hipStream_t) { return hipErrorNotSupported; }
hipError_t launch_binary_grouped(const BinaryDesc &, const WorkItem *, int, hipStream_t) { return hipErrorNotSupported; }

// ---- the chain launchers -------------------------------------------------------------------------------------------------------
hipError_t launch_bf16_chain(int mode, int tile, int b_kind, const ChainArgs &a, hipStream_t) {
  if (!blw_launch_ok(mode, tile, b_kind, blw_shape(a))) return hipErrorInvalidValue;
  const int bm = BLW_TILES[tile].bm(), bn = BLW_TILES[tile].bn();
  if (mode == BLW_LAYER) {
    // (the plain chain: whole tiles both ways - the launcher's own refusal of a shape its grid does not cover)
    if (a.nlayers < 2 || a.nlayers > CH_MAXL || a.m % bm || a.n % bn) return hipErrorInvalidValue;
    const int tiles_m = a.m / bm, tiles_n = a.n / bn;
    return run_chain(FC_PLAIN, tile, b_kind, bm, bn, tiles_m, tiles_n, (long long)tiles_m * tiles_n, a, uniform_seams(a, tiles_m, (unsigned)tiles_n), DT_BF16);
  }
  if (mode == BLW_CHAIN_EDGE) {
    const int tiles_m = chain_edge_tiles_m(a.m, bm), tiles_n = a.n / bn;
    return run_chain(FC_EDGE, tile, b_kind, bm, bn, tiles_m, tiles_n, (long long)tiles_m * tiles_n, a, uniform_seams(a, tiles_m, (unsigned)tiles_n), DT_BF16);
  }
  if (mode == BLW_CHAIN_ROUNDS) {
    const int tiles_m = a.m / bm, tiles_n = a.n / bn;
    return run_chain(FC_ROUNDS, tile, b_kind, bm, bn, tiles_m, tiles_n, (long long)a.groups * tiles_n, a, row_round_seams(a, tiles_m, tiles_n, a.groups), DT_BF16);
  }
  return hipErrorInvalidValue;
}
hipError_t launch_bf16_chain_ragged(int tile, int b_kind, const ChainArgs &a, hipStream_t) {
  if (!blw_chain_ragged_launch_ok(tile, b_kind, blw_shape(a))) return hipErrorInvalidValue;
  const int bm = BLW_TILES[tile].bm(), bn = BLW_TILES[tile].bn();
  const int tiles_m = chain_edge_tiles_m(a.m, bm), tiles_n = chain_ragged_tiles_n(a.n, bn);
  return run_chain(FC_RAGGED, tile, b_kind, bm, bn, tiles_m, tiles_n, (long long)tiles_m * tiles_n, a, uniform_seams(a, tiles_m, (unsigned)tiles_n), DT_BF16);
}
hipError_t launch_bf16_chain_widths(int tile, int b_kind, const ChainArgs &a, hipStream_t) {
  if (!blw_chain_widths_launch_ok(tile, b_kind, blw_widths_shape(a))) return hipErrorInvalidValue;
  const int bm = BLW_TILES[tile].bm(), bn = BLW_TILES[tile].bn();
  const int tiles_m = a.m / bm, grid_n = chain_widths_grid(a.nlayers, bn, [&](int l) { return a.L[l].pad; });
  Seams s{tiles_m, {}, {}};
  for (int l = 0; l + 1 < a.nlayers; ++l) {
    unsigned act = 0;
    for (int tn = 0; tn < grid_n; ++tn) act += chain_widths_active(tn, a.L[l].pad, bn) && chain_widths_signals(l, a.nlayers);
    s.arrivals.push_back(std::vector<unsigned>(tiles_m, act));
    s.expected.push_back(chain_widths_target(a.target, a.L[l].pad, bn));
  }
  return run_chain(FC_WIDTHS, tile, b_kind, bm, bn, tiles_m, grid_n, (long long)tiles_m * grid_n, a, s, DT_BF16);
}
hipError_t launch_bf16_chain_wrounds(int tile, int b_kind, const ChainArgs &a, hipStream_t) {
  if (!blw_chain_wrounds_launch_ok(tile, b_kind, blw_widths_shape(a), a.groups)) return hipErrorInvalidValue;
  const int bm = BLW_TILES[tile].bm(), bn = BLW_TILES[tile].bn();
  const int tiles_m = a.m / bm, W = a.groups;
  Seams s{tiles_m, {}, {}};
  std::vector<unsigned> steps(a.nlayers, 0); // steps of layer l over all column groups, by the walk
  for (int c = 0; c < W; ++c) {
    int tn = c, l = 0, guard = 0;
    while (l < a.nlayers && guard++ < 1 << 24) {
      const int T = chain_widths_tiles(a.L[l].pad, bn);
      if (tn < T) ++steps[l]; // (c >= T: the layer is sat out)
      chain_wrounds_next(tn, l, W, T);
    }
  }
  for (int l = 0; l + 1 < a.nlayers; ++l) {
    s.arrivals.push_back(std::vector<unsigned>(tiles_m, steps[l]));
    s.expected.push_back(chain_widths_target(a.target, a.L[l].pad, bn));
  }
  return run_chain(FC_WROUNDS, tile, b_kind, bm, bn, tiles_m, W, (long long)tiles_m * W, a, s, DT_BF16);
}
hipError_t launch_bf16_chain_wragged(int tile, int b_kind, const ChainArgs &a, hipStream_t) {
  if (!blw_chain_wragged_launch_ok(tile, b_kind, blw_widths_shape(a))) return hipErrorInvalidValue;
  const int bm = BLW_TILES[tile].bm(), bn = BLW_TILES[tile].bn();
  const int tiles_m = chain_edge_tiles_m(a.m, bm), grid_n = chain_wragged_grid(a.nlayers, bn, [&](int l) { return a.L[l].pad; });
  Seams s{tiles_m, {}, {}};
  for (int l = 0; l + 1 < a.nlayers; ++l) {
    unsigned act = 0;
    for (int tn = 0; tn < grid_n; ++tn) act += chain_wragged_active(tn, a.L[l].pad, bn);
    s.arrivals.push_back(std::vector<unsigned>(tiles_m, act));
    s.expected.push_back(chain_wragged_target(a.target, a.L[l].pad, bn));
  }
  return run_chain(FC_WRAGGED, tile, b_kind, bm, bn, tiles_m, grid_n, (long long)tiles_m * grid_n, a, s, DT_BF16);
}
hipError_t launch_bf16_dma256_chain(int b_kind, const ChainArgs &a, hipStream_t) {
  const int G = a.groups ? a.groups : a.m / D256C_BM;
  if (!blw_b_kind_ok(b_kind) || !d256c_shape_ok(a.m, a.n, a.nlayers, CH_MAXL, G)) return hipErrorInvalidValue;
  for (int l = 0; l < a.nlayers; ++l)
    if (!d256c_k_ok(a.L[l].k, a.L[l].br) || !(a.L[l].ep & EP_BETA0)) return hipErrorInvalidValue;
  const int tiles_m = a.m / D256C_BM, tiles_n = a.n / D256C_BN;
  // the walk of every workgroup of the one-dimensional grid, through the launch's own map
  Seams s = uniform_seams(a, tiles_m, 0);
  for (int wg = 0; wg < (int)d256c_grid(G, tiles_n); ++wg) {
    int tm = d256c_group(wg, G, tiles_n), l = 0, guard = 0;
    while (l < a.nlayers && guard++ < 1 << 24) {
      if (l + 1 < a.nlayers) ++s.arrivals[l][tm];
      chain_rounds_next(tm, l, G, tiles_m);
    }
  }
  return run_chain(FC_DMA256, 3, b_kind, D256C_BM, D256C_BN, tiles_m, tiles_n, d256c_grid(G, tiles_n), a, s, DT_BF16);
}
hipError_t launch_f32_chain(int tile, const ChainArgs &a, hipStream_t) {
  int bm = 0, bn = 0;
  (void)f32_chain_tile_dims(tile, &bm, &bn);
  if ((tile != 1 && tile != 2) || a.nlayers < 2 || a.nlayers > CH_MAXL || bm <= 0 || bn <= 0 || a.m % bm || a.n % bn) return hipErrorInvalidValue;
  const int tiles_m = a.m / bm, tiles_n = a.n / bn;
  return run_chain(FC_F32, tile, 0, bm, bn, tiles_m, tiles_n, (long long)tiles_m * tiles_n, a, uniform_seams(a, tiles_m, (unsigned)tiles_n), DT_F32);
}

} // namespace tpp
