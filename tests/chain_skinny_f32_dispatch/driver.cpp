// driver.cpp - TEST INFRASTRUCTURE for tests/test_chain_skinny_f32_dispatch.py, never part of the product library.
//
// The skinny-batch f32 chain form of the layer-chain launch decision (rt_chain.h try_chain_launch, case CF_SKINNY_F32) on a CPU, driven through
// the C-ABI only. Linked against runtime.cpp + host_cache.cpp + gemm_plan.cpp, tests/chain_dispatch/fake_chain.cpp and
// tests/chain_skinny_dispatch/fake_skinny_chain.cpp (all unchanged) and fake_skinny_f32_chain.cpp, the stand-in of launch_f32_skinny_chain with
// its counter model. FAKE_HIP_CUS sets the compute units (default 256).
//   driver args        the six chains of tests/test_chain_skinny_f32_cpu.py chains(bn) at BN 16 / 32 / 64 and m 1 / 16 / 17 / 31 under a forced BN,
//                      the forced_G chain also under G 1 / 3 / 7, and a chain of 65 column blocks of BN 16 whose G the compute units cap: the
//                      argument block is the calls' (pointers, leading dimensions, strides, k, br, epilogue bits, pad = n_l, groups = G),
//                      target = epoch * G and grows by G per launch of a counter block, exactly the new counter moves and reads (G, BN, the
//                      deepest layer's waves), the one launch equals the calls one by one bit for bit through the oracle
//   driver sequence    an f32 skinny chain, a bf16 skinny chain and a plain bf16 chain with one row block, the same G and layer count share a
//                      counter block; interleaved in shuffled order over six epochs no counter is unexpected in any stand-in
//   driver probation   a starved first launch degrades to call by call - a process of its own: the shared flag is sticky
//   driver sanitize    a reduced args pass (BN 32, m 16 / 17) + sequence (built with sanitizers)
// Exit code 0 and a last line "OK" = every check passed.
#include "../../include/tpp_xsmm_abi.h"
#include "../../tpp-mlir_amd/csrc/gemm_plan.h"
#include "../chain_dispatch/fake_chain.h"
#include "../chain_skinny_dispatch/fake_skinny_chain.h"
#include "fake_skinny_f32_chain.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

namespace {
int g_fail = 0;
#define FAIL(...)                            \
  do {                                       \
    if (g_fail++ < 100) {                    \
      fprintf(stdout, "FAIL: " __VA_ARGS__); \
      fprintf(stdout, "\n");                 \
    }                                        \
  } while (0)

constexpr int F32 = 1, BF16 = 2; // the C-ABI's data types
constexpr uint16_t POISON16 = 0x7fc1;
constexpr uint32_t POISON32 = 0x7fc00001u;
constexpr int GAP = 8;
uint32_t g_lcg = 12345;
uint32_t lcg() { return g_lcg = g_lcg * 1664525u + 1013904223u; }

struct Chain {
  int rows = 0, dt = F32, image = 2, n = 0; // image (bf16): 0 VNNI-2, 2 flat, 4 VNNI-4; f32 is flat
  size_t es = 4;                            // bytes per element
  int64_t h[8], off[8], br[8];
  void *a[8], *b[8], *c[8], *d[8];
  int64_t nl[8], kl[8], lda[8], ldb[8], ldc[8], sa[8], sb[8];
  bool bias[8], relu[8];
  size_t c_bytes[8];
  std::vector<void *> dev;
};
void *dev_alloc(Chain &ch, size_t bytes) {
  void *p = nullptr;
  if (hipMalloc(&p, bytes + 64) != hipSuccess || !p) exit(2);
  ch.dev.push_back(p);
  return p;
}
void fill(const Chain &ch, void *p, size_t elems) { // small exactly representable values: j / 8, j = -4 .. 4
  static const uint16_t bf[9] = {0xbf00, 0xbec0, 0xbe80, 0xbe00, 0x0000, 0x3e00, 0x3e80, 0x3ec0, 0x3f00};
  for (size_t i = 0; i < elems; ++i) {
    const int j = (int)((lcg() >> 16) % 9);
    if (ch.dt == F32) ((float *)p)[i] = (float)(j - 4) / 8.0f;
    else ((uint16_t *)p)[i] = bf[j];
  }
}
void poison_outputs(Chain &ch) {
  for (int i = 0; i < ch.n; ++i)
    for (size_t e = 0; e < ch.c_bytes[i] / ch.es; ++e) {
      if (ch.dt == F32) ((uint32_t *)ch.c[i])[e] = POISON32;
      else ((uint16_t *)ch.c[i])[e] = POISON16;
    }
}
// layer l has ns[l] columns and reads brs[l] batch elements of ks[l] columns along k; tile >= 0 (bf16): that loader-wave tile forced
Chain build(int rows, int dt, const std::vector<int> &ns, const std::vector<int> &ks, const std::vector<int> &brs, int tile = -1) {
  Chain ch;
  ch.rows = rows, ch.dt = dt, ch.image = 2, ch.n = (int)ns.size(), ch.es = dt == F32 ? 4 : 2;
  for (int i = 0; i < ch.n; ++i) {
    ch.nl[i] = ns[i], ch.kl[i] = ks[i], ch.br[i] = brs[i], ch.sa[i] = ks[i];
    ch.lda[i] = i ? ch.ldc[i - 1] : (int64_t)ks[0] * brs[0] + GAP;
    ch.ldb[i] = ch.ldc[i] = ns[i] + GAP;
    ch.sb[i] = ch.kl[i] * ch.ldb[i];
    ch.bias[i] = i != 1, ch.relu[i] = i + 1 < ch.n, ch.off[i] = 0;
    if (tile >= 0) xsmm_hip_force_variant(tpp::blw_variant(tile, ch.image));
    ch.h[i] = xsmm_fused_brgemm_dispatch(dt, rows, ch.nl[i], ch.kl[i], ch.lda[i], ch.ldb[i], ch.ldc[i], ch.sa[i], ch.sb[i], XSMM_GEMM_FLAG_BETA_0, 0,
                                         ch.relu[i] ? XSMM_UNARY_RELU : XSMM_UNARY_NONE, ch.bias[i] ? XSMM_BINARY_FLAG_BCAST_COL_IN_0 : 0,
                                         ch.bias[i] ? XSMM_BINARY_ADD : XSMM_BINARY_NONE);
    xsmm_hip_force_variant(-1);
    const size_t b_elems = (size_t)ch.br[i] * ch.kl[i] * ch.ldb[i];
    ch.b[i] = dev_alloc(ch, b_elems * ch.es + 16);
    ch.d[i] = ch.bias[i] ? dev_alloc(ch, (size_t)ch.nl[i] * ch.es + 16) : nullptr;
    ch.c_bytes[i] = (size_t)rows * ch.ldc[i] * ch.es;
    ch.c[i] = dev_alloc(ch, ch.c_bytes[i]);
    fill(ch, ch.b[i], b_elems);
    if (ch.d[i]) fill(ch, ch.d[i], (size_t)ch.nl[i]);
  }
  void *a0 = dev_alloc(ch, (size_t)rows * ch.lda[0] * ch.es);
  fill(ch, a0, (size_t)rows * ch.lda[0]);
  for (int i = 0; i < ch.n; ++i) ch.a[i] = i ? ch.c[i - 1] : a0;
  poison_outputs(ch);
  return ch;
}
void destroy(Chain &ch) {
  xsmm_hip_synchronize();
  for (void *p : ch.dev) (void)hipFree(p);
  ch.dev.clear();
}

// the counters an f32 skinny chain launch must leave alone: every other chain switch's and the four single-call skinny switches'
struct Others { int64_t v[12][5]; };
Others others() {
  Others o;
  memset(&o, 0, sizeof(o));
  xsmm_hip_chain_edge_stats(o.v[0]), xsmm_hip_chain_rounds_stats(o.v[1]), xsmm_hip_chain_ragged_stats(o.v[2]), xsmm_hip_chain_widths_stats(o.v[3]);
  xsmm_hip_chain_width_rounds_stats(o.v[4]), xsmm_hip_chain_widths_ragged_stats(o.v[5]), xsmm_hip_chain_dma256_stats(o.v[6]), xsmm_hip_chain_skinny_stats(o.v[7]);
  xsmm_hip_skinny_bf16_stats(o.v[8]), xsmm_hip_skinny_split_stats(o.v[9]), xsmm_hip_skinny_f32_stats(o.v[10]), xsmm_hip_skinny_f32_split_stats(o.v[11]);
  return o;
}

int invoke(Chain &ch) { return xsmm_hip_fused_brgemm_chain_invoke(ch.dt, ch.n, ch.h, ch.a, ch.off, ch.b, ch.off, ch.c, ch.off, ch.d, ch.off, ch.br); }

// the same calls one by one (every switch 0: the single-call stand-in, through the oracle from each call's descriptor)
void reference(Chain &ch, std::vector<std::vector<char>> &ref) {
  poison_outputs(ch);
  for (int i = 0; i < ch.n; ++i) xsmm_fused_brgemm_invoke(ch.dt, ch.h[i], ch.a[i], 0, ch.b[i], 0, ch.c[i], 0, ch.d[i], 0, ch.br[i]);
  xsmm_hip_synchronize();
  ref.assign(ch.n, {});
  for (int i = 0; i < ch.n; ++i) ref[i].assign((char *)ch.c[i], (char *)ch.c[i] + ch.c_bytes[i]);
  poison_outputs(ch);
}
bool outputs_are(const Chain &ch, const std::vector<std::vector<char>> &ref, const char *what) {
  bool ok = true;
  for (int i = 0; i < ch.n; ++i) {
    if (memcmp(ref[i].data(), ch.c[i], ch.c_bytes[i])) ok = false;
    size_t poisoned = 0; // the gap columns, and only they, still hold the poison
    for (size_t e = 0; e < ch.c_bytes[i] / ch.es; ++e)
      poisoned += ch.dt == F32 ? ((const uint32_t *)ref[i].data())[e] == POISON32 : ((const uint16_t *)ref[i].data())[e] == POISON16;
    if (poisoned != (size_t)ch.rows * GAP) FAIL("%s: %zu poisoned words in layer %d of the reference, %zu gap words", what, poisoned, i, (size_t)ch.rows * GAP);
  }
  return ok;
}

// TARGETS: the last target seen per counter block, whichever form launched on it. A launch's target is the block's epoch * G, so on one
// block - one (stream, 1, G, layers) - it grows by exactly G from launch to launch and is G on the block's first.
std::map<const unsigned *, unsigned> g_last_target;
void check_target(const unsigned *cnt, unsigned target, int G, const char *what) {
  const auto it = g_last_target.find(cnt);
  const unsigned want = (it == g_last_target.end() ? 0u : it->second) + (unsigned)G;
  if (target != want) FAIL("TARGET: %s: target %u, expected %u (the block's last target + G = %d)", what, target, want, G);
  g_last_target[cnt] = target;
}

// one skinny f32 launch: the record, the counters, the bits. Returns the launch's counter block
const unsigned *check_skinny_f32(Chain &ch, int mode, int want_bn, int want_g, const char *what) {
  std::vector<std::vector<char>> ref;
  reference(ch, ref);
  xsmm_hip_set_chain_skinny_f32(mode);
  int64_t before[4], after[4];
  xsmm_hip_chain_skinny_f32_stats(before);
  const Others o0 = others();
  fake_chain_clear(), fake_skinny_clear(), fake_skinny_f32_clear();
  const int ret = invoke(ch);
  xsmm_hip_synchronize();
  xsmm_hip_set_chain_skinny_f32(0);
  xsmm_hip_chain_skinny_f32_stats(after);
  const Others o1 = others();
  if (ret != 1 || fake_skinny_f32_launches() != 1 || fake_skinny_launches() != 0 || fake_chain_launches() != 0 || fake_gemm_launches() != 0) {
    FAIL("%s: returned %d with %d skinny f32 launches, %d bf16 skinny launches, %d other chain launches, %d single launches", what, ret, fake_skinny_f32_launches(),
         fake_skinny_launches(), fake_chain_launches(), fake_gemm_launches());
    return nullptr;
  }
  const FakeSkinnyF32Launch &r = *fake_skinny_f32_launch(0);
  const tpp::ChainArgs &a = r.a;
  if (r.bn != want_bn || a.groups != want_g) FAIL("%s: launched with BN %d G %d, expected %d %d", what, r.bn, a.groups, want_bn, want_g);
  int64_t widest = 0, waves = 1;
  for (int i = 0; i < ch.n; ++i) {
    widest = std::max(widest, ch.nl[i]);
    waves = std::max<int64_t>(waves, std::min<int64_t>(8, ch.br[i] * ((ch.kl[i] + 15) / 16))); // (restated, not read from the header under test)
  }
  if (a.m != ch.rows || a.nlayers != ch.n || a.n != widest || a.A != ch.a[0] || a.lda != ch.lda[0]) FAIL("%s: m %d n %d nlayers %d A / lda of the argument block", what, a.m, a.n, a.nlayers);
  for (int i = 0; i < ch.n; ++i) {
    const tpp::ChainLayer &L = a.L[i];
    const int ep = tpp::EP_BETA0 | (ch.bias[i] ? tpp::EP_BIAS : 0) | (ch.relu[i] ? tpp::EP_RELU : 0);
    if (L.B != ch.b[i] || L.C != ch.c[i] || L.D != ch.d[i] || L.ldb != ch.ldb[i] || L.ldc != ch.ldc[i] || L.stride_a != ch.sa[i] || L.stride_b != ch.sb[i] || L.k != ch.kl[i] ||
        L.br != ch.br[i] || L.ep != ep || L.pad != ch.nl[i])
      FAIL("%s: layer %d of the argument block is not call %d (pad %d, k %d, br %d, ep %d)", what, i, i, L.pad, L.k, L.br, L.ep);
  }
  if (!a.cnt || !a.err) FAIL("%s: no counters or no error word", what);
  else check_target(a.cnt, a.target, want_g, what);
  if (r.waves != waves) FAIL("%s: the launch has %d waves, the deepest layer %ld", what, r.waves, (long)waves);
  if (after[0] != before[0] + 1 || after[1] != want_g || after[2] != want_bn || after[3] != waves)
    FAIL("STATS: %s: {%ld, %ld, %ld, %ld}, expected {%ld, %d, %d, %ld}", what, (long)after[0], (long)after[1], (long)after[2], (long)after[3], (long)before[0] + 1, want_g, want_bn, (long)waves);
  if (memcmp(&o0, &o1, sizeof(o0))) FAIL("%s: another counter moved", what);
  if (!outputs_are(ch, ref, what)) FAIL("MARSHALLING: %s: the one launch differs from the calls one by one", what);
  return a.cnt;
}

struct Spec { const char *name; std::vector<int> ns, ks, brs; };
// tests/test_chain_skinny_f32_cpu.py chains(bn), the list the GPU file runs
std::vector<Spec> chains(int bn) {
  std::vector<int> n8, k8 = {32};
  for (int i = 0; i < 4; ++i) n8.push_back(2 * bn + 4), n8.push_back(bn + 4);
  for (int i = 0; i < 3; ++i) k8.push_back(2 * bn + 4), k8.push_back(bn + 4);
  k8.push_back(2 * bn + 4);
  return {{"ragged_k", {3 * bn + 4, 3 * bn + 4, 3 * bn + 4}, {36, 3 * bn + 4, 3 * bn + 4}, {1, 1, 1}},
          {"sit_out", {4 * bn, bn, 2 * bn + 4}, {32, 4 * bn, bn}, {1, 1, 1}},
          {"waves_1_8", {132, std::max(36, bn), bn}, {16, 132, 16}, {1, 1, 1}},
          {"batches", {144, 96, 64}, {20, 36, 16}, {2, 2, 3}},
          {"eight_layers", n8, k8, std::vector<int>(8, 1)},
          {"forced_G", {6 * bn + 4, 6 * bn + 4}, {36, 6 * bn + 4}, {1, 1}}};
}
int rule_g(const Spec &s, int bn) { // G under a forced BN: a workgroup per column block of the widest layer, at most the compute units
  int blocks = 0;
  for (int n : s.ns) blocks = std::max(blocks, (n + bn - 1) / bn);
  return std::min(blocks, fake_hip_compute_units());
}

int run_args(bool reduced) {
  fake_chain_set_compute(1);
  char what[160];
  for (int bn : {16, 32, 64}) {
    if (reduced && bn != 32) continue;
    for (int m : {1, 16, 17, 31}) {
      if (reduced && m != 16 && m != 17) continue;
      const std::vector<Spec> all = chains(bn);
      for (size_t i = 0; i < all.size(); ++i) {
        const Spec &s = all[i];
        Chain ch = build(m, F32, s.ns, s.ks, s.brs);
        snprintf(what, sizeof(what), "%s, BN %d, m %d", s.name, bn, m);
        check_skinny_f32(ch, bn, bn, rule_g(s, bn), what);
        if (i == 5)
          for (int G : {1, 3, 7}) {
            snprintf(what, sizeof(what), "%s, BN %d, m %d, forced G %d", s.name, bn, m, G);
            check_skinny_f32(ch, 1000 * G + bn, bn, G, what);
            check_skinny_f32(ch, 1000 * G + bn, bn, G, what); // (a second launch of the same block: the target grows by G)
          }
        destroy(ch);
      }
    }
  }
  { // 65 column blocks of BN 16 in the widest layer: G is the compute units where they are fewer (64 of them: workgroup 0 owns two blocks)
    const Spec wide{"65 blocks", {65 * 16, 48}, {20, 65 * 16}, {1, 1}};
    Chain ch = build(17, F32, wide.ns, wide.ks, wide.brs);
    const int G = rule_g(wide, 16);
    if (G != (fake_hip_compute_units() == 64 ? 64 : 65)) FAIL("65 blocks: G %d on %d compute units", G, fake_hip_compute_units());
    check_skinny_f32(ch, 16, 16, G, "65 blocks of BN 16");
    check_skinny_f32(ch, 16, 16, G, "65 blocks of BN 16, again");
    destroy(ch);
  }
  return 0;
}

int run_sequence() {
  fake_chain_set_compute(1);
  // all three on counter blocks keyed (stream, 1, 2, 2 layers). Plain: flat B, a 32-row call on the 32x64 loader-wave tile, 1 x 2 tiles;
  // the skinny chains: G = 2 forced
  Chain plain = build(32, BF16, {128, 128}, {64, 128}, {1, 1}, 0);
  Chain skinny = build(16, BF16, {104, 64}, {72, 104}, {1, 1});
  Chain skinny_f32 = build(16, F32, {100, 64}, {36, 100}, {1, 1});
  std::vector<std::vector<char>> ref_plain, ref_skinny;
  reference(plain, ref_plain), reference(skinny, ref_skinny);
  const unsigned *cnt_plain = nullptr, *cnt_skinny = nullptr, *cnt_f32 = nullptr;
  g_lcg = 20240607;
  long launches = 0;
  for (int e = 0; e < 6; ++e) {
    int order[3] = {0, 1, 2}; // every epoch runs all three, in a shuffled order
    for (int j = 2; j > 0; --j) std::swap(order[j], order[(lcg() >> 9) % (unsigned)(j + 1)]);
    for (int j = 0; j < 3; ++j) {
      char what[64];
      if (order[j] == 0) {
        snprintf(what, sizeof(what), "sequence: skinny f32, epoch %d", e);
        if (const unsigned *c = check_skinny_f32(skinny_f32, 2032, 32, 2, what)) cnt_f32 = c, ++launches;
      } else if (order[j] == 1) {
        snprintf(what, sizeof(what), "sequence: skinny bf16, epoch %d", e);
        poison_outputs(skinny);
        fake_chain_clear(), fake_skinny_clear(), fake_skinny_f32_clear();
        xsmm_hip_set_chain_skinny(2032);
        const int ret = invoke(skinny);
        xsmm_hip_synchronize();
        xsmm_hip_set_chain_skinny(0);
        if (ret != 1 || fake_skinny_launches() != 1 || fake_skinny_f32_launches() != 0 || fake_skinny_launch(0)->a.groups != 2)
          FAIL("%s: did not launch on G = 2 (returned %d, %d launches)", what, ret, fake_skinny_launches());
        else cnt_skinny = fake_skinny_launch(0)->a.cnt, check_target(cnt_skinny, fake_skinny_launch(0)->a.target, 2, what), ++launches;
        if (!outputs_are(skinny, ref_skinny, what)) FAIL("%s: the outputs differ from the calls one by one", what);
      } else {
        snprintf(what, sizeof(what), "sequence: plain, epoch %d", e);
        poison_outputs(plain);
        fake_chain_clear(), fake_skinny_clear(), fake_skinny_f32_clear();
        const int ret = invoke(plain);
        xsmm_hip_synchronize();
        if (ret != 1 || fake_chain_launches() != 1 || fake_chain_launch(0)->form != FC_PLAIN || fake_chain_launch(0)->tiles_m != 1 || fake_chain_launch(0)->grid_n != 2)
          FAIL("%s: did not launch as 1 x 2 tiles (returned %d, %d launches)", what, ret, fake_chain_launches());
        else cnt_plain = fake_chain_launch(0)->a.cnt, check_target(cnt_plain, fake_chain_launch(0)->a.target, 2, what), ++launches;
        if (!outputs_are(plain, ref_plain, what)) FAIL("%s: the outputs differ from the calls one by one", what);
      }
    }
  }
  const bool shared = cnt_f32 && cnt_f32 == cnt_skinny && cnt_f32 == cnt_plain;
  if (!shared) FAIL("SEQUENCE: the f32 skinny chain, the bf16 skinny chain and the plain chain with the same G and layer count do not share a counter block");
  if (launches != 18) FAIL("SEQUENCE: %ld of 18 launches", launches);
  printf("sequence: %ld launches, shared block %d, %d + %d + %d counter mismatches\n", launches, (int)shared, fake_chain_counter_mismatches(), fake_skinny_counter_mismatches(),
         fake_skinny_f32_counter_mismatches());
  destroy(plain), destroy(skinny), destroy(skinny_f32);
  return 0;
}

int run_probation() {
  fake_chain_set_compute(1);
  const Spec s = chains(32)[0];
  Chain ch = build(17, F32, s.ns, s.ks, s.brs);
  std::vector<std::vector<char>> ref;
  reference(ch, ref);
  xsmm_hip_set_chain_skinny_f32(32);
  fake_chain_clear(), fake_skinny_clear(), fake_skinny_f32_clear();
  fake_skinny_f32_starve(1, 1);
  const int ret = invoke(ch);
  xsmm_hip_synchronize();
  if (ret != 0) FAIL("PROBATION: the starved first launch returned %d", ret);
  if (fake_skinny_f32_launches() != 1 || !fake_skinny_f32_launch(0)->starved || fake_gemm_launches() != ch.n)
    FAIL("PROBATION: %d skinny f32 launches, %d single launches", fake_skinny_f32_launches(), fake_gemm_launches());
  if (!outputs_are(ch, ref, "probation")) FAIL("PROBATION: the outputs are not the calls' one by one");
  poison_outputs(ch);
  fake_chain_clear(), fake_skinny_clear(), fake_skinny_f32_clear();
  int64_t before[4], after[4];
  xsmm_hip_chain_skinny_f32_stats(before);
  const Others o0 = others();
  const int ret2 = invoke(ch); // every later chain invoke runs call by call
  xsmm_hip_synchronize();
  xsmm_hip_chain_skinny_f32_stats(after);
  const Others o1 = others();
  if (ret2 != 0 || fake_skinny_f32_launches() != 0 || fake_chain_launches() != 0 || fake_gemm_launches() != ch.n) FAIL("PROBATION: a later chain invoke was launched");
  if (memcmp(before, after, sizeof(before)) || memcmp(&o0, &o1, sizeof(o0))) FAIL("PROBATION: the later invoke moved a chain counter");
  if (!outputs_are(ch, ref, "after probation")) FAIL("PROBATION: the later invoke's outputs are wrong");
  if (xsmm_hip_chain_status() != 0) FAIL("PROBATION: xsmm_hip_chain_status counts %ld repairs (nothing was journaled)", (long)xsmm_hip_chain_status());
  xsmm_hip_set_chain_skinny_f32(0);
  printf("probation: starved first launch ran call by call, chains off afterwards\n");
  destroy(ch);
  return 0;
}
} // namespace

int main(int argc, char **argv) {
  const char *mode = argc > 1 ? argv[1] : "";
  setvbuf(stdout, nullptr, _IOLBF, 0);
  xsmm_hip_set_async(1);
  if (!strcmp(mode, "args")) run_args(false);
  else if (!strcmp(mode, "sequence")) run_sequence();
  else if (!strcmp(mode, "probation")) run_probation();
  else if (!strcmp(mode, "sanitize")) run_args(true), run_sequence();
  else {
    fprintf(stderr, "usage: driver args | sequence | probation | sanitize\n");
    return 2;
  }
  const int mismatches = fake_chain_counter_mismatches() + fake_skinny_counter_mismatches() + fake_skinny_f32_counter_mismatches();
  if (mismatches) FAIL("COUNTER MODEL: %d mismatches", mismatches);
  if (g_fail) {
    printf("%d checks FAILED\n", g_fail);
    return 1;
  }
  printf("OK\n");
  return 0;
}
