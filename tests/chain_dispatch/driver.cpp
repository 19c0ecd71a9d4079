// driver.cpp - TEST INFRASTRUCTURE for tests/test_chain_dispatch.py, never part of the product library.
//
// The layer-chain launch decision (rt_chain.h try_chain_launch) on a CPU, driven through the C-ABI only: xsmm_fused_brgemm_dispatch,
// xsmm_hip_set_*, xsmm_hip_fused_brgemm_chain_invoke, the *_stats calls, xsmm_hip_synchronize, xsmm_hip_chain_status. Linked against
// runtime.cpp + host_cache.cpp + gemm_plan.cpp (unchanged) and fake_chain.cpp, whose launch stand-ins compute through the oracle,
// record every launch and keep a model of the hand-off counters. One process = one (compute units, strict) pair: descriptors are
// planned once at dispatch. FAKE_HIP_CUS sets the compute units (default 256).
//
//   driver table [strict]     the decision table: per chain and B image D({}), the seven D({x}) and D(all)   (check f)
//   driver sweep [strict]     all 128 switch sets x contexts: switch independence + precedence (a), per-launch invariants (b),
//                             the excluded chains stay call by call, coverage of the nine forms (256 CUs, strict off)
//   driver arith              one small chain per form and B image: bit equality with the calls one by one, gap columns intact (c)
//   driver sequence           chains whose counter blocks coincide, interleaved in shuffled order over several epochs (d)
//   driver probation <form>   the first launch of a block is starved (e)         - a process of its own: the shared flag is sticky
//   driver journal            a journaled launch is starved after a verified one (e)
//   driver sanitize           the 1- / 2- / 8- / 9-call chains and one chain per form, decisions and arithmetic (g: built with sanitizers)
//   driver cus                how often a chain invoke asks for its stream's compute units: D({}), the seven D({x}) and D(all)   (check h)
// Exit code 0 and a last line "OK" = every check passed.
#include "../../include/tpp_xsmm_abi.h"
#include "../../tpp-mlir_amd/csrc/gemm_plan.h"
#include "fake_chain.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

// (hipMalloc / hipFree below are the fake device allocator of tests/tsan/fake_hip_host.h)

namespace {
int g_fail = 0;
#define FAIL(...)                                      \
  do {                                                 \
    if (g_fail++ < 200) {                               \
      fprintf(stdout, "FAIL: " __VA_ARGS__);           \
      fprintf(stdout, "\n");                           \
    }                                                  \
  } while (0)

// ---- the seven chain switches ---------------------------------------------------------------------------------------------------
enum Sw : int { SW_EDGE, SW_ROUNDS, SW_RAGGED, SW_WIDTHS, SW_WROUNDS, SW_WRAGGED, SW_DMA256, SW_N };
const char *const SW_NAME[SW_N] = {"edge", "rounds", "ragged", "widths", "wrounds", "wragged", "dma256"};
int set_sw(int sw, int v) {
  switch (sw) {
  case SW_EDGE: return xsmm_hip_set_chain_edge(v);
  case SW_ROUNDS: return xsmm_hip_set_chain_rounds(v);
  case SW_RAGGED: return xsmm_hip_set_chain_ragged(v);
  case SW_WIDTHS: return xsmm_hip_set_chain_widths(v);
  case SW_WROUNDS: return xsmm_hip_set_chain_width_rounds(v);
  case SW_WRAGGED: return xsmm_hip_set_chain_widths_ragged(v);
  default: return xsmm_hip_set_chain_dma256(v);
  }
}
void get_stats(int sw, int64_t out[4]) {
  switch (sw) {
  case SW_EDGE: return xsmm_hip_chain_edge_stats(out);
  case SW_ROUNDS: return xsmm_hip_chain_rounds_stats(out);
  case SW_RAGGED: return xsmm_hip_chain_ragged_stats(out);
  case SW_WIDTHS: return xsmm_hip_chain_widths_stats(out);
  case SW_WROUNDS: return xsmm_hip_chain_width_rounds_stats(out);
  case SW_WRAGGED: return xsmm_hip_chain_widths_ragged_stats(out);
  default: return xsmm_hip_chain_dma256_stats(out);
  }
}
// the *_stats counter of a launch form (-1: the plain and the f32 chain have none)
int form_stats(int form) {
  switch (form) {
  case FC_EDGE: return SW_EDGE;
  case FC_ROUNDS: return SW_ROUNDS;
  case FC_RAGGED: return SW_RAGGED;
  case FC_WIDTHS: return SW_WIDTHS;
  case FC_WROUNDS: return SW_WROUNDS;
  case FC_WRAGGED: return SW_WRAGGED;
  case FC_DMA256: return SW_DMA256;
  default: return -1;
  }
}
// A context: the value each switch has when it is in the set, and the modes of other switches the chain rules read (or must not read)
struct Ctx {
  const char *name;
  int val[SW_N];
  int edge_tiles, images, edge_k_bf16, edge_k8_bf16;
  bool same_as_base; // every decision must be the base context's (the single-call ragged switches change no chain decision)
};
const Ctx CTXS[] = {
    {"base", {1, 1, 1, 1, 1, 1, 1}, 0, 0, 0, 0, false},
    {"forced", {1, 1002, 1, 1, 1002, 1, 2}, 0, 0, 0, 0, false},      // rounds 1000 + G, width rounds 1000 + W, every eligible chain on the 256x256 tile
    {"forced-g1", {1, 1001, 1, 1, 1001, 1, 1001}, 0, 0, 0, 0, false}, // G = W = 1; the 256x256 chain on one row group
    {"tile20", {1, 1, 1, 1, 1, 1, 1}, 20, 0, 0, 0, false},           // forcing edge-tile modes: the ragged rules read them
    {"tile21", {1, 1, 1, 1, 1, 1, 1}, 21, 0, 0, 0, false},
    {"tile22", {1, 1, 1, 1, 1, 1, 1}, 22, 0, 0, 0, false},
    {"tile23", {1, 1, 1, 1, 1, 1, 1}, 23, 0, 0, 0, false},
    {"images", {1, 1, 1, 1, 1, 1, 1}, 0, 1, 0, 0, false},            // mode 1 of the 256x256 chain reads xsmm_hip_set_dma256_images
    {"singles", {1, 1, 1, 1, 1, 1, 1}, 2, 0, 1, 1, true},            // the three single-call ragged switches on
};
const int N_CTX = sizeof(CTXS) / sizeof(CTXS[0]);
void apply(const Ctx &c, unsigned mask) {
  for (int s = 0; s < SW_N; ++s)
    if (set_sw(s, mask >> s & 1 ? c.val[s] : 0) < 0) FAIL("xsmm_hip_set_chain_%s refused %d", SW_NAME[s], c.val[s]);
  xsmm_hip_set_edge_tiles(c.edge_tiles);
  xsmm_hip_set_dma256_images(c.images);
  xsmm_hip_set_edge_k_bf16(c.edge_k_bf16);
  xsmm_hip_set_edge_k8_bf16(c.edge_k8_bf16);
}
void all_off() { apply(CTXS[0], 0); }

// THE ONE PRECEDENCE LIST (from the comments of try_chain_launch): the 256x256 tile is asked first; a forced 1000 + G / 1000 + W in front
// of the one-round rules; mixed widths in front of column rounds; the one-round ragged-m launch in front of several rounds; ragged width
// and then ragged mixed widths where the others refuse.
std::vector<int> precedence(const Ctx &c) {
  std::vector<int> p = {SW_DMA256};
  if (tpp::chain_rounds_mode_forced(c.val[SW_ROUNDS])) p.push_back(SW_ROUNDS);
  if (tpp::chain_width_rounds_mode_forced(c.val[SW_WROUNDS])) p.push_back(SW_WROUNDS);
  for (int s : {SW_WIDTHS, SW_WROUNDS, SW_EDGE, SW_ROUNDS, SW_RAGGED, SW_WRAGGED})
    if (std::find(p.begin(), p.end(), s) == p.end()) p.push_back(s);
  return p;
}

// ---- chains -------------------------------------------------------------------------------------------------------------------------
enum Quirk : int {
  Q_NONE, Q_BETA1, Q_VNNI_C, Q_GENERIC, Q_IMAGES_DIFFER, Q_ROW_STRIDE, Q_NOT_A_CHAIN, Q_MISALIGNED_B, Q_MISALIGNED_BIAS, Q_OVERLAP, Q_HOST_OPERAND, Q_DIFFER_M,
};
struct Spec {
  const char *name;
  int rows;
  std::vector<int> sizes; // the input's width and every layer's: layer l is [rows x sizes[l]] @ [sizes[l] x sizes[l + 1]]
  int br = 1;             // batch elements per layer, walking along k: k(l) = sizes[l] / br
  int quirk = Q_NONE;
  bool excluded = false;  // the chain contract or a rule excludes it under EVERY switch set: call by call
  int f32_variant = 0;    // > 0: an f32 chain dispatched with this variant forced (6 = 64x64 + K2, 7 = 64x32 + K4)
  int gap = 0;            // gap columns behind every row of the input, the weights and the outputs (the device tests' layout: 8)
  int k_all = 0;          // > 0: every layer reads only the first k_all columns of its input (sizes[0] = k_all)
  int bf16_tile = -1;     // 0 .. 3: every call dispatched with that loader-wave tile forced (of the chain's B image)
};
constexpr uint16_t POISON16 = 0x7fc1;
constexpr uint32_t POISON32 = 0x7fc00001u;

struct Chain {
  Spec s;
  int image = 0; // 0 VNNI-2, 2 flat, 4 VNNI-4
  int n = 0;
  int64_t dtype = 2;
  int64_t h[16], off[16], br[16];
  void *a[16], *b[16], *c[16], *d[16];
  int64_t nl[16], kl[16], lda[16], ldb[16], ldc[16], sa[16], sb[16];
  bool bias[16], relu[16];
  size_t c_bytes[16];
  std::vector<void *> dev;
  std::vector<void *> host;
  size_t es() const { return dtype == 1 ? 4 : 2; }
};
void *dev_alloc(Chain &ch, size_t bytes) {
  void *p = nullptr;
  if (hipMalloc(&p, bytes + 64) != hipSuccess || !p) {
    fprintf(stderr, "out of memory\n");
    exit(2);
  }
  ch.dev.push_back(p);
  return p;
}
uint32_t g_lcg = 12345;
uint32_t lcg() { return g_lcg = g_lcg * 1664525u + 1013904223u; }
// small exactly representable values: j / 8, j = -4 .. 4
void fill(const Chain &ch, void *p, size_t elems) {
  static const uint16_t bf[9] = {0xbf00, 0xbec0, 0xbe80, 0xbe00, 0x0000, 0x3e00, 0x3e80, 0x3ec0, 0x3f00};
  for (size_t i = 0; i < elems; ++i) {
    const uint16_t w = bf[(lcg() >> 16) % 9];
    if (ch.dtype == 1) ((uint32_t *)p)[i] = (uint32_t)w << 16;
    else ((uint16_t *)p)[i] = w;
  }
}
void poison(const Chain &ch, void *p, size_t bytes) {
  if (ch.dtype == 1) for (size_t i = 0; i < bytes / 4; ++i) ((uint32_t *)p)[i] = POISON32;
  else for (size_t i = 0; i < bytes / 2; ++i) ((uint16_t *)p)[i] = POISON16;
}
void poison_outputs(Chain &ch) {
  for (int i = 0; i < ch.n; ++i)
    if (ch.s.quirk != Q_OVERLAP || i != 2) poison(ch, ch.c[i], ch.c_bytes[i]);
}

// dispatches the calls and allocates the operands; with_data: inputs filled, outputs poisoned (the computing checks)
Chain build(const Spec &s, int image, bool with_data) {
  Chain ch;
  ch.s = s;
  ch.image = s.f32_variant ? 2 : image;
  ch.n = (int)s.sizes.size() - 1;
  ch.dtype = s.f32_variant ? 1 : 2;
  const size_t es = ch.es();
  for (int i = 0; i < ch.n; ++i) {
    const int64_t rows = s.quirk == Q_DIFFER_M && i == 1 ? s.rows / 2 : s.rows;
    ch.nl[i] = s.sizes[i + 1];
    ch.kl[i] = (s.k_all ? s.k_all : s.sizes[i]) / s.br;
    ch.br[i] = s.br;
    ch.sa[i] = s.quirk == Q_ROW_STRIDE && i == 1 ? 8 * (i ? ch.ldc[i - 1] : s.sizes[0]) : ch.kl[i];
    ch.lda[i] = i ? ch.ldc[i - 1] : s.sizes[0] + s.gap;
    ch.ldb[i] = ch.nl[i] + s.gap;
    ch.ldc[i] = ch.nl[i] + s.gap;
    ch.sb[i] = ch.kl[i] * ch.ldb[i];
    ch.bias[i] = i != 1;
    ch.relu[i] = i + 1 < ch.n;
    ch.off[i] = 0;
    int img = ch.image;
    if (s.quirk == Q_IMAGES_DIFFER && i == 1) img = image == 2 ? 0 : 2;
    int64_t flags = XSMM_GEMM_FLAG_BETA_0;
    if (s.quirk == Q_BETA1 && i == 1) flags = 0;
    if (ch.dtype == 2 && img != 2) flags |= XSMM_GEMM_WIRE_VNNI_B;
    if (s.quirk == Q_VNNI_C && i == 1) flags |= XSMM_GEMM_FLAG_VNNI_C;
    xsmm_hip_set_vnni_factor(img == 4 ? 4 : 2);
    if (s.f32_variant) xsmm_hip_force_variant(s.f32_variant);
    if (s.bf16_tile >= 0) xsmm_hip_force_variant(tpp::blw_variant(s.bf16_tile, img));
    if (s.quirk == Q_GENERIC && i == 1) xsmm_hip_force_variant(8);
    ch.h[i] = xsmm_fused_brgemm_dispatch(ch.dtype, rows, ch.nl[i], ch.kl[i], ch.lda[i], ch.ldb[i], ch.ldc[i], ch.sa[i], ch.sb[i], flags, 0,
                                         ch.relu[i] ? XSMM_UNARY_RELU : XSMM_UNARY_NONE, ch.bias[i] ? XSMM_BINARY_FLAG_BCAST_COL_IN_0 : 0,
                                         ch.bias[i] ? XSMM_BINARY_ADD : XSMM_BINARY_NONE);
    xsmm_hip_force_variant(-1);
    xsmm_hip_set_vnni_factor(2);
    const size_t b_elems = (size_t)ch.br[i] * ch.kl[i] * ch.ldb[i];
    ch.b[i] = dev_alloc(ch, b_elems * es + 16);
    ch.d[i] = ch.bias[i] ? dev_alloc(ch, (size_t)ch.nl[i] * es + 16) : nullptr;
    ch.c_bytes[i] = (size_t)s.rows * ch.ldc[i] * es;
    ch.c[i] = dev_alloc(ch, ch.c_bytes[i]);
    if (with_data) {
      fill(ch, ch.b[i], b_elems);
      if (ch.d[i]) fill(ch, ch.d[i], (size_t)ch.nl[i]);
    }
    if (s.quirk == Q_HOST_OPERAND && i == 1) {
      ch.b[i] = aligned_alloc(256, (b_elems * es + 255) & ~(size_t)255);
      memset(ch.b[i], 0, b_elems * es);
      ch.host.push_back(ch.b[i]);
    }
    if (s.quirk == Q_MISALIGNED_B && i == 1) ch.b[i] = (char *)ch.b[i] + es;
    if (s.quirk == Q_MISALIGNED_BIAS && i == 0) ch.d[i] = (char *)ch.d[i] + es;
  }
  const size_t a_elems = (size_t)s.rows * ch.lda[0];
  void *a0 = dev_alloc(ch, a_elems * es);
  if (with_data) fill(ch, a0, a_elems);
  for (int i = 0; i < ch.n; ++i) ch.a[i] = i ? ch.c[i - 1] : a0;
  if (s.quirk == Q_NOT_A_CHAIN) {
    ch.a[1] = dev_alloc(ch, (size_t)s.rows * ch.lda[1] * es);
    if (with_data) fill(ch, ch.a[1], (size_t)s.rows * ch.lda[1]);
  }
  if (s.quirk == Q_OVERLAP) ch.c[2] = ch.c[0];
  if (with_data) poison_outputs(ch);
  return ch;
}
void destroy(Chain &ch) {
  xsmm_hip_synchronize();
  for (void *p : ch.dev) (void)hipFree(p);
  for (void *p : ch.host) free(p);
  ch.dev.clear();
  ch.host.clear();
}

// ---- one invoke, its decision and the per-launch invariants (check b) ------------------------------------------------------------
struct Decision {
  std::string text;
  int form = -1; // -1: call by call
};
int g_cus = 256;
long g_forms_seen[3][FC_FORMS];
int image_index(int image) { return image == 0 ? 0 : image == 2 ? 1 : 2; }

void check_launch(const Chain &ch, const FakeChainLaunch &r, const char *what) {
  const tpp::ChainArgs &a = r.a;
  const bool mixed = r.form == FC_WIDTHS || r.form == FC_WROUNDS || r.form == FC_WRAGGED;
  const bool ceil_m = r.form == FC_EDGE || r.form == FC_RAGGED || r.form == FC_WRAGGED;
  const bool ceil_n = r.form == FC_RAGGED || r.form == FC_WRAGGED;
  int64_t widest = 0;
  for (int i = 0; i < ch.n; ++i) widest = ch.nl[i] > widest ? ch.nl[i] : widest;
  // residency: every workgroup of the launch on a compute unit of its own
  if (r.grid > g_cus || r.grid < 1) FAIL("%s: %s launch of %lld workgroups on %d compute units", what, fake_chain_form_name(r.form), r.grid, g_cus);
  if (a.m != ch.s.rows || a.nlayers != ch.n || a.n != widest) FAIL("%s: m %d n %d nlayers %d in the argument block", what, a.m, a.n, a.nlayers);
  if (r.form != FC_F32 && r.b_kind != ch.image) FAIL("%s: launched with B image %d, the calls have %d", what, r.b_kind, ch.image);
  // the tile divides, or ceil-divides, m and every n as the form says
  if (ceil_m ? a.m < r.bm : a.m % r.bm != 0) FAIL("%s: %s launch, %d rows on tiles of %d", what, fake_chain_form_name(r.form), a.m, r.bm);
  if (r.tiles_m != (a.m + r.bm - 1) / r.bm) FAIL("%s: row blocks %d", what, r.tiles_m);
  int64_t grid_n = 0;
  for (int i = 0; i < ch.n; ++i) {
    const int64_t n_i = ch.nl[i];
    if (!mixed && n_i != widest) FAIL("%s: %s launch of calls that differ in n", what, fake_chain_form_name(r.form));
    if (ceil_n ? n_i < r.bn || n_i % 8 != 0 : n_i % r.bn != 0) FAIL("%s: %s launch, layer %d has %ld columns on tiles of %d", what, fake_chain_form_name(r.form), i, (long)n_i, r.bn);
    if ((n_i + r.bn - 1) / r.bn > grid_n) grid_n = (n_i + r.bn - 1) / r.bn;
    const int64_t k = ch.kl[i];
    const bool k_ok = r.form == FC_F32 ? k % 64 == 0 : r.form == FC_DMA256 ? k % 32 == 0 && k >= 32 : ceil_n ? k >= 64 && k % 8 == 0 : k >= 64 && k % 64 == 0;
    if (!k_ok) FAIL("%s: %s launch with k = %ld in layer %d", what, fake_chain_form_name(r.form), (long)k, i);
    const tpp::ChainLayer &L = a.L[i];
    if (L.pad != (mixed ? (int)n_i : 0)) FAIL("%s: layer %d pad %d", what, i, L.pad);
    const int ep = tpp::EP_BETA0 | (ch.bias[i] ? tpp::EP_BIAS : 0) | (ch.relu[i] ? tpp::EP_RELU : 0);
    if (L.B != ch.b[i] || L.C != ch.c[i] || L.D != ch.d[i] || L.ldb != ch.ldb[i] || L.ldc != ch.ldc[i] || L.stride_a != ch.sa[i] || L.stride_b != ch.sb[i] ||
        L.k != ch.kl[i] || L.br != ch.br[i] || L.ep != ep)
      FAIL("%s: layer %d of the argument block is not call %d (B %d C %d D %d ldb %ld ldc %ld sa %ld sb %ld k %d br %d ep %d)", what, i, i, L.B == ch.b[i], L.C == ch.c[i],
           L.D == ch.d[i], (long)L.ldb, (long)L.ldc, (long)L.stride_a, (long)L.stride_b, L.k, L.br, L.ep);
  }
  if (a.A != ch.a[0] || a.lda != ch.lda[0]) FAIL("%s: A / lda of the argument block are not call 0's", what);
  const bool rounds = r.form == FC_ROUNDS || r.form == FC_WROUNDS || r.form == FC_DMA256;
  if (rounds ? a.groups <= 0 : a.groups != 0) FAIL("%s: %s launch with groups = %d", what, fake_chain_form_name(r.form), a.groups);
  if (r.form == FC_ROUNDS && (a.groups >= r.tiles_m || r.grid != (long long)a.groups * grid_n)) FAIL("%s: rounds launch G %d of %d row blocks", what, a.groups, r.tiles_m);
  if (r.form == FC_WROUNDS && (a.groups >= grid_n || r.grid != (long long)a.groups * r.tiles_m)) FAIL("%s: column rounds W %d of %ld column tiles", what, a.groups, (long)grid_n);
  if (r.form == FC_DMA256 && a.groups > r.tiles_m) FAIL("%s: 256x256 chain G %d of %d row blocks", what, a.groups, r.tiles_m);
  if (!rounds && r.grid != (long long)r.tiles_m * grid_n) FAIL("%s: grid %lld != %d x %ld", what, r.grid, r.tiles_m, (long)grid_n);
  if (!a.cnt || !a.err || !a.target) FAIL("%s: cnt / err / target missing", what);
}

Decision invoke(Chain &ch, const char *what, int *ret_out = nullptr) {
  int64_t before[SW_N][4], after[SW_N][4];
  for (int s = 0; s < SW_N; ++s) get_stats(s, before[s]);
  fake_chain_clear();
  const int ret = xsmm_hip_fused_brgemm_chain_invoke(ch.dtype, ch.n, ch.h, ch.a, ch.off, ch.b, ch.off, ch.c, ch.off, ch.d, ch.off, ch.br);
  for (int s = 0; s < SW_N; ++s) get_stats(s, after[s]);
  if (ret_out) *ret_out = ret;
  Decision d;
  const int nl = fake_chain_launches(), ng = fake_gemm_launches();
  if (ret == 1) {
    if (nl != 1 || ng != 0) FAIL("%s: returned 1 with %d chain launches and %d single launches", what, nl, ng);
  } else if (nl != 0 || ng != ch.n) FAIL("%s: returned 0 with %d chain launches and %d single launches of %d calls", what, nl, ng, ch.n);
  int moved = -1, n_moved = 0;
  for (int s = 0; s < SW_N; ++s)
    if (after[s][0] != before[s][0]) moved = s, ++n_moved;
  if (nl == 1 && ret == 1) {
    const FakeChainLaunch &r = *fake_chain_launch(0);
    check_launch(ch, r, what);
    d.form = r.form;
    char buf[160];
    snprintf(buf, sizeof(buf), "%s:%dx%d:b%d:%dx%d:g%d", fake_chain_form_name(r.form), r.bm, r.bn, r.b_kind, r.tiles_m, r.grid_n, r.a.groups);
    d.text = buf;
    ++g_forms_seen[image_index(ch.image)][r.form];
    // exactly one *_stats counter moved by one, the form's, and its other words are the launch's grid and tile
    const int want = form_stats(r.form);
    if (want < 0 ? n_moved != 0 : n_moved != 1 || moved != want || after[want][0] != before[want][0] + 1)
      FAIL("%s: %s launch, %d counters moved (the last: %s)", what, fake_chain_form_name(r.form), n_moved, moved >= 0 ? SW_NAME[moved] : "-");
    else if (want >= 0) {
      const int64_t *w = after[want];
      const int64_t variant = tpp::blw_variant(r.tile, r.b_kind);
      bool ok = true;
      if (r.form == FC_ROUNDS) ok = w[1] == r.a.groups && w[2] == (r.tiles_m + r.a.groups - 1) / r.a.groups && w[3] == variant;
      else if (r.form == FC_WROUNDS) ok = w[1] == r.tiles_m && w[2] == r.a.groups && w[3] == variant;
      else if (r.form == FC_DMA256) ok = w[1] == r.a.groups && w[2] == (r.tiles_m + r.a.groups - 1) / r.a.groups && w[3] == r.b_kind;
      else ok = w[1] == r.tiles_m && w[2] == r.grid_n && w[3] == variant;
      if (!ok) FAIL("%s: %s stats {%ld, %ld, %ld} do not describe the launch %s", what, SW_NAME[want], (long)w[1], (long)w[2], (long)w[3], d.text.c_str());
    }
  } else {
    d.text = "calls";
    if (n_moved) FAIL("%s: call by call, yet the %s counter moved", what, SW_NAME[moved]);
  }
  xsmm_hip_synchronize();
  return d;
}

// ---- the lattice ---------------------------------------------------------------------------------------------------------------------
Spec mk(const char *name, int rows, std::vector<int> sizes) {
  Spec s;
  s.name = name, s.rows = rows, s.sizes = std::move(sizes);
  return s;
}
Spec excl(const char *name, int rows, std::vector<int> sizes, int quirk) {
  Spec s = mk(name, rows, std::move(sizes));
  s.quirk = quirk, s.excluded = true;
  return s;
}
std::vector<Spec> lattice() {
  std::vector<Spec> v;
  static char names[16][48];
  int nn = 0;
  // the README's rows: three 1024-wide layers at every batch size it names (k = 1024: the tile a call is planned on depends on it)
  for (int rows : {64, 256, 1000, 1024, 1366, 2000, 4096, 4100, 4224, 8192, 16384, 32768}) {
    snprintf(names[nn], sizeof(names[nn]), "%dx[1024]*4", rows);
    v.push_back(mk(names[nn++], rows, {1024, 1024, 1024, 1024}));
  }
  v.push_back(mk("1000x[1000]*4", 1000, {1000, 1000, 1000, 1000}));
  v.push_back(mk("2000x[1000]*4", 2000, {1000, 1000, 1000, 1000}));
  v.push_back(mk("1024x[784,1000,1000,1000]", 1024, {784, 1000, 1000, 1000}));
  v.push_back(mk("1024x[1024,512,256,128]", 1024, {1024, 512, 256, 128}));
  v.push_back(mk("1000x[1024,512,256,128]", 1000, {1024, 512, 256, 128}));
  v.push_back(mk("1024x[784,512,256,128]", 1024, {784, 512, 256, 128}));
  v.push_back(mk("512x[784,256,64,256,784]", 512, {784, 256, 64, 256, 784}));
  v.push_back(mk("1000x[1000,504,248]", 1000, {1000, 504, 248}));
  v.push_back(mk("1000x[1000,500,250]", 1000, {1000, 500, 250}));
  v.push_back(mk("1024x[1024,4096,1024]", 1024, {1024, 4096, 1024}));
  v.push_back(mk("256x[1024,4096,1024]", 256, {1024, 4096, 1024}));
  v.push_back(mk("1024x[1024,2048,1024,2048,1024]", 1024, {1024, 2048, 1024, 2048, 1024}));
  v.push_back(mk("2048x[1024,2048,1024]", 2048, {1024, 2048, 1024}));
  v.push_back(mk("1000x[1000,2000,1000]", 1000, {1000, 2000, 1000}));
  v.push_back(mk("200x[200]*4", 200, {200, 200, 200, 200}));
  v.push_back(mk("200x[200,136,72,200]", 200, {200, 136, 72, 200}));
  v.push_back(mk("256x[256,512,128,256]", 256, {256, 512, 128, 256}));
  v.push_back(mk("4096x[4096]*4", 4096, {4096, 4096, 4096, 4096}));
  // column rounds by rule need a tile all calls were dispatched on: the feed-forward block with the 64x64 tile forced
  v.push_back(mk("1024x[1024,4096,1024] on 64x64", 1024, {1024, 4096, 1024}));
  v.back().bf16_tile = 1;
  // the smallest shapes of each form (the device test's candidates)
  v.push_back(mk("64x[64]*4", 64, {64, 64, 64, 64}));
  v.push_back(mk("100x[128]*4", 100, {128, 128, 128, 128}));
  v.push_back(mk("8224x[64]*3", 32 * 257, {64, 64, 64}));
  v.push_back(mk("256x[256]*4", 256, {256, 256, 256, 256}));
  v.push_back(mk("512x[256]*3", 512, {256, 256, 256}));
  v.push_back(mk("64x[128,256,64,128]", 64, {128, 256, 64, 128}));
  // the device test's chains (tests/test_chain_switches_gpu.py), in its layout: 8 gap columns behind every row
  auto dev = [&](const char *name, int rows, std::vector<int> sizes, int k_all = 0) {
    v.push_back(mk(name, rows, std::move(sizes)));
    v.back().gap = 8, v.back().k_all = k_all;
  };
  dev("dev 64x[64]*3", 64, {64, 64, 64});
  dev("dev 100x[128]*3", 100, {128, 128, 128});
  dev("dev 200x[200]*4", 200, {200, 200, 200, 200});
  dev("dev 256x[256,512,128,256]", 256, {256, 512, 128, 256});
  dev("dev 200x[200,136,72,200]", 200, {200, 136, 72, 200});
  dev("dev 8224x[64]*3", 32 * 257, {64, 64, 64});
  dev("dev 16448x[64]*3", 64 * 257, {64, 64, 64});
  dev("dev 16384x[64,1024,1024] k64", 16384, {64, 1024, 1024}, 64);
  dev("dev 7680x[64,2048,2048] k64", 7680, {64, 2048, 2048}, 64);
  dev("dev 512x[64,256,256] k64", 512, {64, 256, 256}, 64);
  dev("dev 64x[64,100,64]", 64, {64, 100, 64});
  dev("dev 64x[64]*4", 64, {64, 64, 64, 64});
  dev("dev 40x[64]*4", 40, {64, 64, 64, 64});
  dev("dev 64x[64,128,64,128]", 64, {64, 128, 64, 128});
  dev("dev 40x[64,128,64,128]", 40, {64, 128, 64, 128});
  // chains of 1, 2, 8 and 9 calls
  v.push_back(mk("64x[64]*2 (1 call)", 64, {64, 64}));
  v.back().excluded = true;
  v.push_back(mk("64x[64]*3 (2 calls)", 64, {64, 64, 64}));
  v.push_back(mk("64x[64]*9 (8 calls)", 64, std::vector<int>(9, 64)));
  v.push_back(mk("64x[64]*10 (9 calls)", 64, std::vector<int>(10, 64)));
  v.back().excluded = true;
  // two batch elements per layer, k = 64 j
  v.push_back(mk("64x[128]*4 br2", 64, {128, 128, 128, 128}));
  v.back().br = 2;
  v.push_back(mk("100x[256]*3 br2", 100, {256, 256, 256}));
  v.back().br = 2;
  v.push_back(mk("256x[256,512,128] br2", 256, {256, 512, 128}));
  v.back().br = 2;
  // f32 chains on both K-split tiles
  v.push_back(mk("f32 1024x[512,1024,1024] 64x64+K2", 1024, {512, 1024, 1024}));
  v.back().f32_variant = 6;
  v.push_back(mk("f32 512x[1024]*4 64x32+K4", 512, {1024, 1024, 1024, 1024}));
  v.back().f32_variant = 7;
  // what the rules and the chain contract exclude
  v.push_back(excl("k%8: 64x[68,64,64]", 64, {68, 64, 64}, Q_NONE));
  v.push_back(excl("n%8: 64x[64,100,64]", 64, {64, 100, 64}, Q_NONE));
  v.push_back(excl("m<BM: 16x[64]*4", 16, {64, 64, 64, 64}, Q_NONE));
  v.push_back(excl("beta 1: 64x[64]*4", 64, {64, 64, 64, 64}, Q_BETA1));
  v.push_back(excl("VNNI C: 64x[64]*4", 64, {64, 64, 64, 64}, Q_VNNI_C));
  v.push_back(excl("forced generic: 64x[64]*4", 64, {64, 64, 64, 64}, Q_GENERIC));
  v.push_back(excl("images differ: 64x[64]*4", 64, {64, 64, 64, 64}, Q_IMAGES_DIFFER));
  v.push_back(excl("row-striding call: 64x[128]*4 br2", 64, {128, 128, 128, 128}, Q_ROW_STRIDE));
  v.back().br = 2;
  v.push_back(excl("not a chain: 64x[64]*4", 64, {64, 64, 64, 64}, Q_NOT_A_CHAIN));
  v.push_back(excl("misaligned B: 64x[64]*4", 64, {64, 64, 64, 64}, Q_MISALIGNED_B));
  v.push_back(excl("misaligned bias: 64x[64]*4", 64, {64, 64, 64, 64}, Q_MISALIGNED_BIAS));
  v.push_back(excl("outputs overlap: 64x[64]*4", 64, {64, 64, 64, 64}, Q_OVERLAP));
  v.push_back(excl("host operand: 64x[64]*4", 64, {64, 64, 64, 64}, Q_HOST_OPERAND));
  v.push_back(excl("calls differ in m: 64x[64]*4", 64, {64, 64, 64, 64}, Q_DIFFER_M));
  return v;
}
const int IMAGES[3] = {0, 2, 4};
const char *image_name(int image) { return image == 0 ? "vnni2" : image == 2 ? "flat" : "vnni4"; }

// ---- check f: the table ------------------------------------------------------------------------------------------------------------
int run_table(bool strict, bool all_images) {
  fake_chain_set_compute(0);
  printf("# chain | image cus strict | D({}) | D({edge}) D({rounds}) D({ragged}) D({widths}) D({wrounds}) D({wragged}) D({dma256}) | D(all)\n");
  printf("# a launch: form:tile:B image:row blocks x workgroup columns:groups\n");
  for (const Spec &s : lattice())
    for (int image : IMAGES) {
      if ((s.f32_variant || !all_images) && image != 0) continue;
      Chain ch = build(s, image, false);
      printf("%s | %s %d %d |", s.name, s.f32_variant ? "f32" : image_name(image), g_cus, (int)strict);
      for (int i = -1; i <= SW_N; ++i) {
        apply(CTXS[0], i < 0 ? 0u : i == SW_N ? 127u : 1u << i);
        printf("%s %s", i == 0 || i == SW_N ? " |" : "", invoke(ch, s.name).text.c_str());
      }
      printf("\n");
      all_off();
      destroy(ch);
    }
  return 0;
}

// ---- check a (+ b on every launch): the sweep -----------------------------------------------------------------------------------
int run_sweep(bool strict) {
  fake_chain_set_compute(0);
  long invokes = 0, launched = 0;
  for (const Spec &s : lattice())
    for (int image : IMAGES) {
      if (s.f32_variant && image != 0) continue;
      Chain ch = build(s, image, false);
      std::vector<std::string> base(128);
      for (int ci = 0; ci < N_CTX; ++ci) {
        const Ctx &c = CTXS[ci];
        std::vector<std::string> D(128);
        char what[200];
        for (unsigned mask = 0; mask < 128; ++mask) {
          apply(c, mask);
          snprintf(what, sizeof(what), "%s %s ctx %s set 0x%02x", s.name, image_name(ch.image), c.name, mask);
          const Decision d = invoke(ch, what);
          D[mask] = d.text;
          ++invokes;
          launched += d.form >= 0;
          if (s.excluded && d.form >= 0) FAIL("%s: an excluded chain was launched as %s", what, d.text.c_str());
        }
        if (ci == 0) base = D;
        const std::vector<int> prec = precedence(c);
        int shown = 0; // (every violation counts, two per chain and context are printed)
        for (unsigned mask = 0; mask < 128; ++mask) {
          int winner = -1;
          for (int sw : prec)
            if ((mask >> sw & 1) && D[1u << sw] != D[0]) {
              winner = sw;
              break;
            }
          const std::string &want = winner < 0 ? D[0] : D[1u << winner];
          if (D[mask] != want && shown++ >= 2) ++g_fail;
          else if (D[mask] != want)
            FAIL("SWITCH INDEPENDENCE: %s %s ctx %s: D(0x%02x) = %s, expected %s (%s%s); D({}) = %s", s.name, image_name(ch.image), c.name, mask, D[mask].c_str(), want.c_str(),
                 winner < 0 ? "no switch of the set changes the decision alone" : "by precedence the decision of ", winner < 0 ? "" : SW_NAME[winner], D[0].c_str());
          if (c.same_as_base && D[mask] != base[mask])
            FAIL("SINGLE-CALL SWITCHES: %s %s: D(0x%02x) = %s with the single-call ragged switches on, %s with them off", s.name, image_name(ch.image), mask, D[mask].c_str(),
                 base[mask].c_str());
        }
      }
      all_off();
      destroy(ch);
    }
  printf("sweep: %ld invokes, %ld launched as one kernel, %d compute units, strict %d\n", invokes, launched, g_cus, (int)strict);
  printf("forms launched (vnni2 / flat / vnni4):");
  for (int f = 0; f < FC_FORMS; ++f) printf(" %s %ld/%ld/%ld", fake_chain_form_name(f), g_forms_seen[0][f], g_forms_seen[1][f], g_forms_seen[2][f]);
  printf("\n");
  if (g_cus == 256 && !strict)
    for (int f = 0; f < FC_FORMS; ++f)
      for (int i = 0; i < (f == FC_F32 ? 1 : 3); ++i)
        if (!g_forms_seen[f == FC_F32 ? 1 : i][f]) FAIL("COVERAGE: the %s form was never launched with image %s", fake_chain_form_name(f), f == FC_F32 ? "f32" : image_name(IMAGES[i]));
  return 0;
}

// ---- check c: marshalling --------------------------------------------------------------------------------------------------------
struct Small {
  int form;
  Spec s;
  int sw, val, edge_tiles; // the switch that asks for the form (-1: none)
};
std::vector<Small> small_chains() {
  std::vector<Small> v;
  auto add = [&](int form, Spec s, int sw, int val, int et = 0) {
    s.gap = 8;
    v.push_back(Small{form, s, sw, val, et});
  };
  add(FC_PLAIN, mk("small plain", 64, {64, 64, 64, 64}), -1, 0);
  add(FC_EDGE, mk("small edge", 100, {128, 128, 128, 128}), SW_EDGE, 1);
  add(FC_ROUNDS, mk("small rounds", 128, {64, 64, 64}), SW_ROUNDS, 1001);
  add(FC_RAGGED, mk("small ragged", 200, {200, 200, 200, 200}), SW_RAGGED, 1);
  add(FC_WIDTHS, mk("small widths", 64, {128, 256, 64, 128}), SW_WIDTHS, 1);
  add(FC_WROUNDS, mk("small wrounds", 64, {128, 256, 64, 128}), SW_WROUNDS, 1002);
  add(FC_WRAGGED, mk("small wragged", 200, {200, 136, 72, 200}), SW_WRAGGED, 1);
  add(FC_DMA256, mk("small dma256", 512, {64, 256, 256}), SW_DMA256, 1001);
  Spec b2 = mk("small plain br2", 64, {128, 128, 128});
  b2.br = 2;
  add(FC_PLAIN, b2, -1, 0);
  Spec f = mk("small f32", 128, {64, 64, 64});
  f.f32_variant = 6;
  add(FC_F32, f, -1, 0);
  return v;
}
bool gaps_intact(const Chain &ch, const char *what) {
  bool ok = true;
  for (int i = 0; i < ch.n; ++i)
    for (int64_t r = 0; r < ch.s.rows && ok; ++r)
      for (int64_t j = ch.nl[i]; j < ch.ldc[i] && ok; ++j) {
        const bool p = ch.dtype == 1 ? ((const uint32_t *)ch.c[i])[r * ch.ldc[i] + j] == POISON32 : ((const uint16_t *)ch.c[i])[r * ch.ldc[i] + j] == POISON16;
        if (!p) {
          FAIL("%s: gap column %ld of row %ld of layer %d was written", what, (long)j, (long)r, i);
          ok = false;
        }
      }
  return ok;
}
// the chain as one invoke against the same calls one by one (both through the oracle: bit equality, no tolerance)
const unsigned *check_marshalling(Chain &ch, int want_form, const char *what) {
  poison_outputs(ch);
  const Decision d = invoke(ch, what);
  const unsigned *cnt = fake_chain_launches() == 1 ? fake_chain_launch(0)->a.cnt : nullptr; // (the launch's counter block)
  if (d.form != want_form) FAIL("%s: expected the %s form, got %s", what, fake_chain_form_name(want_form), d.text.c_str());
  gaps_intact(ch, what);
  std::vector<std::vector<char>> got(ch.n);
  for (int i = 0; i < ch.n; ++i) got[i].assign((char *)ch.c[i], (char *)ch.c[i] + ch.c_bytes[i]);
  poison_outputs(ch);
  for (int i = 0; i < ch.n; ++i) xsmm_fused_brgemm_invoke(ch.dtype, ch.h[i], ch.a[i], 0, ch.b[i], 0, ch.c[i], 0, ch.d[i], 0, ch.br[i]);
  xsmm_hip_synchronize();
  for (int i = 0; i < ch.n; ++i) {
    if (memcmp(got[i].data(), ch.c[i], ch.c_bytes[i])) FAIL("MARSHALLING: %s: layer %d of the one launch differs from the calls one by one", what, i);
    size_t poisoned = 0; // the reference itself must have computed something
    for (size_t e = 0; e < ch.c_bytes[i] / ch.es(); ++e)
      poisoned += ch.dtype == 1 ? ((const uint32_t *)ch.c[i])[e] == POISON32 : ((const uint16_t *)ch.c[i])[e] == POISON16;
    if (poisoned != (size_t)ch.s.rows * ch.s.gap) FAIL("%s: %zu poisoned words left in layer %d, %zu gap words", what, poisoned, i, (size_t)ch.s.rows * ch.s.gap);
  }
  return cnt;
}
int run_arith(bool every_image) {
  fake_chain_set_compute(1);
  for (const Small &sm : small_chains())
    for (int image : IMAGES) {
      if ((sm.s.f32_variant || !every_image) && image != 0) continue;
      Chain ch = build(sm.s, image, true);
      all_off();
      if (sm.sw >= 0) set_sw(sm.sw, sm.val);
      xsmm_hip_set_edge_tiles(sm.edge_tiles);
      char what[120];
      snprintf(what, sizeof(what), "%s %s", sm.s.name, sm.s.f32_variant ? "f32" : image_name(image));
      check_marshalling(ch, sm.form, what);
      printf("arith: %-24s one %s launch = the calls one by one, bit for bit\n", what, fake_chain_form_name(sm.form));
      all_off();
      destroy(ch);
    }
  return 0;
}

// ---- check d: counters across a sequence ---------------------------------------------------------------------------------------------
int run_sequence() {
  fake_chain_set_compute(1);
  struct Item { Small sm; Chain ch; };
  std::vector<Item> items;
  auto add = [&](int form, Spec s, int sw, int val) { items.push_back(Item{Small{form, s, sw, val, 0}, Chain()}); };
  // one grid of 2 x 1 tiles of 32x64, three layers: the plain chain, edge rows, two rounds on one group, ragged width (k0 = 72)
  add(FC_PLAIN, mk("seq plain 64x[64]*4", 64, {64, 64, 64, 64}), -1, 0);
  add(FC_EDGE, mk("seq edge 40x[64]*4", 40, {64, 64, 64, 64}), SW_EDGE, 1);
  add(FC_ROUNDS, mk("seq rounds 128x[64]*4", 128, {64, 64, 64, 64}), SW_ROUNDS, 1001); // (VNNI-2: 2 x 1 tiles of 64x64)
  add(FC_RAGGED, mk("seq ragged 64x[72,64,64,64]", 64, {72, 64, 64, 64}), SW_RAGGED, 1);
  // the same widest layer and grid, different inner widths: blocks of their own
  add(FC_WIDTHS, mk("seq widths 64x[64,128,64,128]", 64, {64, 128, 64, 128}), SW_WIDTHS, 1);
  add(FC_WIDTHS, mk("seq widths 64x[64,128,128,64]", 64, {64, 128, 128, 64}), SW_WIDTHS, 1);
  // mixed widths, column rounds and ragged mixed widths on one grid with the same tiles per layer
  add(FC_WROUNDS, mk("seq wrounds 64x[64,128,64,128]", 64, {64, 128, 64, 128}), SW_WROUNDS, 1001);
  add(FC_WRAGGED, mk("seq wragged 40x[64,128,64,128]", 40, {64, 128, 64, 128}), SW_WRAGGED, 1);
  add(FC_WRAGGED, mk("seq wragged 64x[72,128,64,128]", 64, {72, 128, 64, 128}), SW_WRAGGED, 1);
  add(FC_DMA256, mk("seq dma256 512x[64,256,256]", 512, {64, 256, 256}), SW_DMA256, 1001);
  add(FC_DMA256, mk("seq dma256 512x[64,256,256] G2", 512, {64, 256, 256}), SW_DMA256, 1002);
  for (Item &it : items) it.ch = build(it.sm.s, 0, true);
  std::vector<const unsigned *> cnt(items.size(), nullptr);
  const int EPOCHS = 5;
  g_lcg = 20240607;
  long launches = 0;
  for (int e = 0; e < EPOCHS; ++e) {
    std::vector<int> order(items.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
    for (size_t i = order.size(); i > 1; --i) std::swap(order[i - 1], order[(lcg() >> 8) % i]);
    for (int idx : order) {
      Item &it = items[idx];
      all_off();
      if (it.sm.sw >= 0) set_sw(it.sm.sw, it.sm.val);
      char what[120];
      snprintf(what, sizeof(what), "%s epoch %d", it.sm.s.name, e);
      const unsigned *c = check_marshalling(it.ch, it.sm.form, what); // (the outputs at every step, as well as the counters)
      if (c) cnt[idx] = c, ++launches;
    }
  }
  all_off();
  // which launches shared a counter block
  int shared_equal = 0, shared_mixed = 0;
  for (size_t i = 0; i < items.size(); ++i)
    for (size_t j = i + 1; j < items.size(); ++j)
      if (cnt[i] && cnt[i] == cnt[j]) {
        printf("sequence: '%s' and '%s' share a counter block\n", items[i].sm.s.name, items[j].sm.s.name);
        if (items[i].sm.form != items[j].sm.form) (items[i].sm.form <= FC_RAGGED ? shared_equal : shared_mixed) += 1;
      }
  if (cnt[4] && cnt[4] == cnt[5]) FAIL("SEQUENCE: two mixed-width chains with different inner widths share a counter block");
  if (shared_equal < 3) FAIL("SEQUENCE: only %d pairs of different equal-width forms shared a counter block (the plain / edge / rounds / ragged grid was meant to coincide)", shared_equal);
  if (shared_mixed < 2) FAIL("SEQUENCE: only %d pairs of different mixed-width forms shared a counter block", shared_mixed);
  printf("sequence: %ld launches over %d shuffled epochs, %d counter mismatches\n", launches, EPOCHS, fake_chain_counter_mismatches());
  for (Item &it : items) destroy(it.ch);
  return 0;
}

// ---- check e: degrading ---------------------------------------------------------------------------------------------------------------
void reference_outputs(Chain &ch, std::vector<std::vector<char>> &ref) {
  poison_outputs(ch);
  for (int i = 0; i < ch.n; ++i) xsmm_fused_brgemm_invoke(ch.dtype, ch.h[i], ch.a[i], 0, ch.b[i], 0, ch.c[i], 0, ch.d[i], 0, ch.br[i]);
  xsmm_hip_synchronize();
  ref.assign(ch.n, {});
  for (int i = 0; i < ch.n; ++i) ref[i].assign((char *)ch.c[i], (char *)ch.c[i] + ch.c_bytes[i]);
  poison_outputs(ch);
}
bool outputs_are(const Chain &ch, const std::vector<std::vector<char>> &ref) {
  for (int i = 0; i < ch.n; ++i)
    if (memcmp(ref[i].data(), ch.c[i], ch.c_bytes[i])) return false;
  return true;
}
int run_probation(int form) {
  fake_chain_set_compute(1);
  for (const Small &sm : small_chains()) {
    if (sm.form != form || sm.s.br != 1) continue;
    Chain ch = build(sm.s, 0, true);
    std::vector<std::vector<char>> ref;
    reference_outputs(ch, ref);
    all_off();
    if (sm.sw >= 0) set_sw(sm.sw, sm.val);
    fake_chain_clear();
    fake_chain_starve(1, 1);
    const int ret = xsmm_hip_fused_brgemm_chain_invoke(ch.dtype, ch.n, ch.h, ch.a, ch.off, ch.b, ch.off, ch.c, ch.off, ch.d, ch.off, ch.br);
    xsmm_hip_synchronize();
    if (ret != 0) FAIL("PROBATION %s: the starved first launch returned %d", sm.s.name, ret);
    if (fake_chain_launches() != 1 || !fake_chain_launch(0)->starved || fake_chain_launch(0)->form != form || fake_gemm_launches() != ch.n)
      FAIL("PROBATION %s: %d chain launches, %d single launches", sm.s.name, fake_chain_launches(), fake_gemm_launches());
    if (!outputs_are(ch, ref)) FAIL("PROBATION %s: the outputs are not the calls' one by one", sm.s.name);
    // every later chain invoke runs call by call
    poison_outputs(ch);
    int ret2 = -1;
    const Decision d = invoke(ch, "after a starved probation launch", &ret2);
    if (ret2 != 0 || d.form >= 0) FAIL("PROBATION %s: a later chain invoke was launched (%s)", sm.s.name, d.text.c_str());
    if (!outputs_are(ch, ref)) FAIL("PROBATION %s: the later invoke's outputs are wrong", sm.s.name);
    if (xsmm_hip_chain_status() != 0) FAIL("PROBATION %s: xsmm_hip_chain_status counts %ld repairs (nothing was journaled)", sm.s.name, (long)xsmm_hip_chain_status());
    printf("probation: %s - starved first launch ran call by call, chains off afterwards\n", sm.s.name);
    all_off();
    destroy(ch);
    return 0;
  }
  FAIL("no small chain of form %d", form);
  return 0;
}
int run_journal() {
  fake_chain_set_compute(1);
  const std::vector<Small> sm = small_chains();
  Chain c1 = build(sm[0].s, 0, true), c2 = build(sm[1].s, 0, true);
  std::vector<std::vector<char>> r1, r2;
  reference_outputs(c1, r1);
  reference_outputs(c2, r2);
  all_off();
  set_sw(SW_EDGE, 1);
  int ret = 0;
  // the first launch of each block: probation, verified
  if (invoke(c1, "journal: first launch of chain 1", &ret).form != FC_PLAIN) FAIL("JOURNAL: chain 1 did not launch");
  if (invoke(c2, "journal: first launch of chain 2", &ret).form != FC_EDGE) FAIL("JOURNAL: chain 2 did not launch");
  poison_outputs(c1), poison_outputs(c2);
  fake_chain_clear();
  // a journaled healthy launch, a journaled STARVED one, a journaled healthy successor - no synchronisation in between
  const int a = xsmm_hip_fused_brgemm_chain_invoke(c1.dtype, c1.n, c1.h, c1.a, c1.off, c1.b, c1.off, c1.c, c1.off, c1.d, c1.off, c1.br);
  fake_chain_starve(1, 2);
  const int b = xsmm_hip_fused_brgemm_chain_invoke(c2.dtype, c2.n, c2.h, c2.a, c2.off, c2.b, c2.off, c2.c, c2.off, c2.d, c2.off, c2.br);
  const int c = xsmm_hip_fused_brgemm_chain_invoke(c1.dtype, c1.n, c1.h, c1.a, c1.off, c1.b, c1.off, c1.c, c1.off, c1.d, c1.off, c1.br);
  if (a != 1 || b != 1 || c != 1 || fake_chain_launches() != 3 || fake_gemm_launches() != 0) FAIL("JOURNAL: the three journaled invokes returned %d %d %d, %d launches", a, b, c, fake_chain_launches());
  if (outputs_are(c2, r2)) FAIL("JOURNAL: the starved stand-in stored outputs");
  xsmm_hip_synchronize();
  // exactly the starved launch and its successor were re-run, call by call, in launch order
  const int ng = fake_gemm_launches();
  if (ng != c2.n + c1.n) FAIL("JOURNAL: %d single launches at the synchronisation, expected %d", ng, c2.n + c1.n);
  for (int i = 0; i < ng && i < c2.n + c1.n; ++i) {
    const void *want = i < c2.n ? c2.c[i] : c1.c[i - c2.n];
    if (fake_gemm_launch(i)->C != want) FAIL("JOURNAL: re-run call %d writes another output than launch order asks", i);
  }
  if (!outputs_are(c1, r1) || !outputs_are(c2, r2)) FAIL("JOURNAL: outputs after the re-run are not the calls' one by one");
  if (xsmm_hip_chain_status() != 2) FAIL("JOURNAL: xsmm_hip_chain_status = %ld, expected 2 (the starved launch and its successor)", (long)xsmm_hip_chain_status());
  int ret2 = -1;
  if (invoke(c1, "journal: after the repair", &ret2).form >= 0 || ret2 != 0) FAIL("JOURNAL: a chain was launched after a starved one");
  printf("journal: a starved journaled launch and its successor re-run in order, status %ld\n", (long)xsmm_hip_chain_status());
  all_off();
  destroy(c1), destroy(c2);
  return 0;
}

// ---- check g: what the sanitizer build runs ---------------------------------------------------------------------------------------
int run_sanitize() {
  fake_chain_set_compute(0);
  for (const Spec &s : lattice()) {
    if (!strstr(s.name, "call")) continue; // the 1- / 2- / 8- / 9-call chains
    Chain ch = build(s, 0, false);
    for (unsigned mask : {0u, 127u}) {
      apply(CTXS[0], mask);
      const Decision d = invoke(ch, s.name);
      printf("sanitize: %s set 0x%02x -> %s\n", s.name, mask, d.text.c_str());
    }
    all_off();
    destroy(ch);
  }
  return run_arith(false);
}

// ---- check h: the stream's compute units are asked for at most once per chain invoke ----------------------------------------------
// (three runtime calls behind every question: hipExtStreamGetCUMask counts them.) Never where the chain contract refuses - the call count,
// a call that does not read its predecessor's output, a row-striding batch, a misaligned or a host operand: those are checked in front of
// the decision (two outputs that overlap are found behind it) -, and never where column rounds by rule are asked about calls that differ
// in n and share no tile they were all dispatched on, with the mixed-width switch off: that answer needs no compute units.
int run_cus() {
  fake_chain_set_compute(0);
  long invokes = 0, asked = 0, contract = 0, gated = 0;
  for (const Spec &s : lattice())
    for (int image : IMAGES) {
      if (s.f32_variant && image != 0) continue;
      Chain ch = build(s, image, false);
      const bool by_contract = ch.n < 2 || ch.n > 8 || s.quirk == Q_ROW_STRIDE || s.quirk == Q_NOT_A_CHAIN || s.quirk == Q_MISALIGNED_B ||
                               s.quirk == Q_MISALIGNED_BIAS || s.quirk == Q_HOST_OPERAND;
      bool differ_n = false;
      for (int i = 1; i < ch.n; ++i) differ_n = differ_n || ch.nl[i] != ch.nl[0];
      for (int i = -1; i <= SW_N; ++i) {
        apply(CTXS[0], i < 0 ? 0u : i == SW_N ? 127u : 1u << i);
        char what[200];
        snprintf(what, sizeof(what), "%s %s set %s", s.name, image_name(ch.image), i < 0 ? "{}" : i == SW_N ? "all" : SW_NAME[i]);
        const long before = fake_hip_cu_mask_queries();
        const Decision d = invoke(ch, what);
        const long q = fake_hip_cu_mask_queries() - before;
        ++invokes, asked += q;
        if (q > 1) FAIL("COMPUTE UNITS: %s: asked %ld times in one invoke (%s)", what, q, d.text.c_str());
        if (by_contract && ++contract && q) FAIL("COMPUTE UNITS: %s: the chain contract refuses the chain, yet the compute units were asked for", what);
        if (i == SW_WROUNDS && differ_n && d.form < 0 && fake_gemm_launches() == ch.n && ch.n <= 8) {
          const tpp::GemmDesc *descs[8];
          for (int l = 0; l < ch.n; ++l) descs[l] = fake_gemm_launch(l)->d;
          if (tpp::chain_rounds_planned_tile(ch.n, descs) < 0 && ++gated && q)
            FAIL("COMPUTE UNITS: %s: column rounds by rule without a tile all calls were dispatched on, yet the compute units were asked for", what);
        }
      }
      all_off();
      destroy(ch);
    }
  printf("cus: %ld invokes asked %ld times, %ld invokes refused by the contract and %ld gated column-round invokes asked 0 times\n", invokes, asked, contract, gated);
  if (!contract || !gated) FAIL("COMPUTE UNITS: no contract-refused or no gated column-round chain in the lattice");
  return 0;
}
} // namespace

int main(int argc, char **argv) {
  const char *mode = argc > 1 ? argv[1] : "";
  const bool strict = argc > 2 && !strcmp(argv[2], "strict");
  setvbuf(stdout, nullptr, _IOLBF, 0);
  g_cus = fake_hip_compute_units();
  xsmm_hip_set_async(1);
  if (strict && xsmm_hip_set_strict(1) < 0) return 2;
  all_off();
  if (!strcmp(mode, "table")) run_table(strict, argc > 3 && !strcmp(argv[3], "images"));
  else if (!strcmp(mode, "sweep")) run_sweep(strict);
  else if (!strcmp(mode, "arith")) run_arith(true);
  else if (!strcmp(mode, "sequence")) run_sequence();
  else if (!strcmp(mode, "probation")) run_probation(argc > 2 ? atoi(argv[2]) : 0);
  else if (!strcmp(mode, "journal")) run_journal();
  else if (!strcmp(mode, "sanitize")) run_sanitize();
  else if (!strcmp(mode, "cus")) run_cus();
  else {
    fprintf(stderr, "usage: driver table|sweep [strict [images]] | arith | sequence | probation <form> | journal | sanitize | cus\n");
    return 2;
  }
  if (fake_chain_counter_mismatches()) FAIL("COUNTER MODEL: %d mismatches", fake_chain_counter_mismatches());
  if (g_fail) {
    printf("%d checks FAILED\n", g_fail);
    return 1;
  }
  printf("OK\n");
  return 0;
}
