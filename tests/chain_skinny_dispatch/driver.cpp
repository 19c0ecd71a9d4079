// driver.cpp - TEST INFRASTRUCTURE for tests/test_chain_skinny_dispatch.py, never part of the product library.
//
// The skinny-batch chain form of the layer-chain launch decision (rt_chain.h try_chain_launch, case CF_SKINNY) on a CPU, driven through the
// C-ABI only. Linked against runtime.cpp + host_cache.cpp + gemm_plan.cpp and tests/chain_dispatch/fake_chain.cpp (all unchanged) and
// fake_skinny_chain.cpp, the stand-in of launch_bf16_skinny_chain with its counter model. FAKE_HIP_CUS sets the compute units (default 256).
//   driver args        the argument block is the calls' (pointers, leading dimensions, strides, k, br, epilogue bits, pad = n_l, groups = G),
//                      exactly the new counter moves and describes the launch, the one launch equals the calls one by one bit for bit
//                      through the oracle; the three B images, equal and mixed widths, batches along k, a forced G
//   driver sequence    a skinny chain and a plain chain with one row block, the same G and layer count share a counter block; interleaved
//                      in shuffled order over several epochs no counter is unexpected
//   driver probation   a starved first launch degrades to call by call - a process of its own: the shared flag is sticky
//   driver sanitize    args + sequence (built with sanitizers)
// Exit code 0 and a last line "OK" = every check passed.
#include "../../include/tpp_xsmm_abi.h"
#include "../../tpp-mlir_amd/csrc/gemm_plan.h"
#include "../chain_dispatch/fake_chain.h"
#include "fake_skinny_chain.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

constexpr uint16_t POISON16 = 0x7fc1;
constexpr int GAP = 8;
uint32_t g_lcg = 12345;
uint32_t lcg() { return g_lcg = g_lcg * 1664525u + 1013904223u; }

struct Chain {
  int rows = 0, image = 0, n = 0; // image: 0 VNNI-2, 2 flat, 4 VNNI-4
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
void fill(void *p, size_t elems) { // small exactly representable values: j / 8, j = -4 .. 4
  static const uint16_t bf[9] = {0xbf00, 0xbec0, 0xbe80, 0xbe00, 0x0000, 0x3e00, 0x3e80, 0x3ec0, 0x3f00};
  for (size_t i = 0; i < elems; ++i) ((uint16_t *)p)[i] = bf[(lcg() >> 16) % 9];
}
void poison_outputs(Chain &ch) {
  for (int i = 0; i < ch.n; ++i)
    for (size_t e = 0; e < ch.c_bytes[i] / 2; ++e) ((uint16_t *)ch.c[i])[e] = POISON16;
}
// sizes: the input's width and every layer's n; layer l reads brs[l] batch elements of ks[l] columns along k; tile >= 0: that loader-wave tile forced
Chain build(int rows, int image, const std::vector<int> &ns, const std::vector<int> &ks, const std::vector<int> &brs, int tile = -1) {
  Chain ch;
  ch.rows = rows, ch.image = image, ch.n = (int)ns.size();
  for (int i = 0; i < ch.n; ++i) {
    ch.nl[i] = ns[i], ch.kl[i] = ks[i], ch.br[i] = brs[i], ch.sa[i] = ks[i];
    ch.lda[i] = i ? ch.ldc[i - 1] : (int64_t)ks[0] * brs[0] + GAP;
    ch.ldb[i] = ch.ldc[i] = ns[i] + GAP;
    ch.sb[i] = ch.kl[i] * ch.ldb[i];
    ch.bias[i] = i != 1, ch.relu[i] = i + 1 < ch.n, ch.off[i] = 0;
    int64_t flags = XSMM_GEMM_FLAG_BETA_0 | (image != 2 ? XSMM_GEMM_WIRE_VNNI_B : 0);
    xsmm_hip_set_vnni_factor(image == 4 ? 4 : 2);
    if (tile >= 0) xsmm_hip_force_variant(tpp::blw_variant(tile, image));
    ch.h[i] = xsmm_fused_brgemm_dispatch(2, rows, ch.nl[i], ch.kl[i], ch.lda[i], ch.ldb[i], ch.ldc[i], ch.sa[i], ch.sb[i], flags, 0, ch.relu[i] ? XSMM_UNARY_RELU : XSMM_UNARY_NONE,
                                         ch.bias[i] ? XSMM_BINARY_FLAG_BCAST_COL_IN_0 : 0, ch.bias[i] ? XSMM_BINARY_ADD : XSMM_BINARY_NONE);
    xsmm_hip_force_variant(-1);
    xsmm_hip_set_vnni_factor(2);
    const size_t b_elems = (size_t)ch.br[i] * ch.kl[i] * ch.ldb[i];
    ch.b[i] = dev_alloc(ch, b_elems * 2 + 16);
    ch.d[i] = ch.bias[i] ? dev_alloc(ch, (size_t)ch.nl[i] * 2 + 16) : nullptr;
    ch.c_bytes[i] = (size_t)rows * ch.ldc[i] * 2;
    ch.c[i] = dev_alloc(ch, ch.c_bytes[i]);
    fill(ch.b[i], b_elems);
    if (ch.d[i]) fill(ch.d[i], (size_t)ch.nl[i]);
  }
  void *a0 = dev_alloc(ch, (size_t)rows * ch.lda[0] * 2);
  fill(a0, (size_t)rows * ch.lda[0]);
  for (int i = 0; i < ch.n; ++i) ch.a[i] = i ? ch.c[i - 1] : a0;
  poison_outputs(ch);
  return ch;
}
void destroy(Chain &ch) {
  xsmm_hip_synchronize();
  for (void *p : ch.dev) (void)hipFree(p);
  ch.dev.clear();
}

// the counters a skinny chain launch must leave alone: the seven other chain switches' and the two skinny switches'
struct Others { int64_t v[9][5]; };
Others others() {
  Others o;
  memset(&o, 0, sizeof(o));
  xsmm_hip_chain_edge_stats(o.v[0]), xsmm_hip_chain_rounds_stats(o.v[1]), xsmm_hip_chain_ragged_stats(o.v[2]), xsmm_hip_chain_widths_stats(o.v[3]);
  xsmm_hip_chain_width_rounds_stats(o.v[4]), xsmm_hip_chain_widths_ragged_stats(o.v[5]), xsmm_hip_chain_dma256_stats(o.v[6]);
  xsmm_hip_skinny_bf16_stats(o.v[7]), xsmm_hip_skinny_split_stats(o.v[8]);
  return o;
}

int invoke(Chain &ch) { return xsmm_hip_fused_brgemm_chain_invoke(2, ch.n, ch.h, ch.a, ch.off, ch.b, ch.off, ch.c, ch.off, ch.d, ch.off, ch.br); }

void reference(Chain &ch, std::vector<std::vector<char>> &ref) {
  poison_outputs(ch);
  for (int i = 0; i < ch.n; ++i) xsmm_fused_brgemm_invoke(2, ch.h[i], ch.a[i], 0, ch.b[i], 0, ch.c[i], 0, ch.d[i], 0, ch.br[i]);
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
    for (size_t e = 0; e < ch.c_bytes[i] / 2; ++e) poisoned += ((const uint16_t *)ref[i].data())[e] == POISON16;
    if (poisoned != (size_t)ch.rows * GAP) FAIL("%s: %zu poisoned words in layer %d of the reference, %zu gap words", what, poisoned, i, (size_t)ch.rows * GAP);
  }
  return ok;
}

// one skinny launch: the record, the counters, the bits. Returns the launch's counter block
const unsigned *check_skinny(Chain &ch, int mode, int want_bn, int want_g, const char *what) {
  std::vector<std::vector<char>> ref;
  reference(ch, ref);
  xsmm_hip_set_chain_skinny(mode);
  int64_t before[4], after[4];
  xsmm_hip_chain_skinny_stats(before);
  const Others o0 = others();
  fake_chain_clear(), fake_skinny_clear();
  const int ret = invoke(ch);
  xsmm_hip_synchronize();
  xsmm_hip_set_chain_skinny(0);
  xsmm_hip_chain_skinny_stats(after);
  const Others o1 = others();
  if (ret != 1 || fake_skinny_launches() != 1 || fake_chain_launches() != 0 || fake_gemm_launches() != 0) {
    FAIL("%s: returned %d with %d skinny launches, %d other chain launches, %d single launches", what, ret, fake_skinny_launches(), fake_chain_launches(), fake_gemm_launches());
    return nullptr;
  }
  const FakeSkinnyLaunch &r = *fake_skinny_launch(0);
  const tpp::ChainArgs &a = r.a;
  if (r.b_kind != ch.image || r.bn != want_bn || a.groups != want_g) FAIL("%s: launched with image %d BN %d G %d, expected %d %d %d", what, r.b_kind, r.bn, a.groups, ch.image, want_bn, want_g);
  int64_t widest = 0;
  for (int i = 0; i < ch.n; ++i) widest = std::max(widest, ch.nl[i]);
  if (a.m != ch.rows || a.nlayers != ch.n || a.n != widest || a.A != ch.a[0] || a.lda != ch.lda[0]) FAIL("%s: m %d n %d nlayers %d A / lda of the argument block", what, a.m, a.n, a.nlayers);
  for (int i = 0; i < ch.n; ++i) {
    const tpp::ChainLayer &L = a.L[i];
    const int ep = tpp::EP_BETA0 | (ch.bias[i] ? tpp::EP_BIAS : 0) | (ch.relu[i] ? tpp::EP_RELU : 0);
    if (L.B != ch.b[i] || L.C != ch.c[i] || L.D != ch.d[i] || L.ldb != ch.ldb[i] || L.ldc != ch.ldc[i] || L.stride_a != ch.sa[i] || L.stride_b != ch.sb[i] || L.k != ch.kl[i] ||
        L.br != ch.br[i] || L.ep != ep || L.pad != ch.nl[i])
      FAIL("%s: layer %d of the argument block is not call %d (pad %d, k %d, br %d, ep %d)", what, i, i, L.pad, L.k, L.br, L.ep);
  }
  if (!a.cnt || !a.err || a.target == 0 || a.target % (unsigned)want_g) FAIL("%s: cnt / err / target %u (a multiple of G = %d)", what, a.target, want_g);
  if (after[0] != before[0] + 1 || after[1] != want_g || after[2] != want_bn || after[3] != ch.image) FAIL("%s: stats {%ld, %ld, %ld, %ld}", what, (long)after[0], (long)after[1], (long)after[2], (long)after[3]);
  if (memcmp(&o0, &o1, sizeof(o0))) FAIL("%s: another counter moved", what);
  if (!outputs_are(ch, ref, what)) FAIL("MARSHALLING: %s: the one launch differs from the calls one by one", what);
  return a.cnt;
}

int run_args() {
  fake_chain_set_compute(1);
  for (int image : {0, 2, 4}) {
    const int bn = 32;
    char what[120];
    {
      Chain ch = build(8, image, {104, 104, 104}, {72, 104, 104}, {1, 1, 1});
      snprintf(what, sizeof(what), "equal widths, image %d", image);
      check_skinny(ch, bn, bn, 4, what);
      if (image == 0) check_skinny(ch, 1, 16, 7, what); // the rule: a VNNI-2 chain of small layers on BN 16
      destroy(ch);
    }
    {
      Chain ch = build(31, image, {128, 32, 72}, {64, 128, 32}, {1, 1, 1});
      snprintf(what, sizeof(what), "mixed widths, image %d", image);
      check_skinny(ch, bn, bn, 4, what);
      check_skinny(ch, 3000 + bn, bn, 3, what); // a forced G
      destroy(ch);
    }
    {
      Chain ch = build(16, image, {144, 96, 64}, {40, 72, 32}, {2, 2, 3});
      snprintf(what, sizeof(what), "batches along k, image %d", image);
      check_skinny(ch, 64, 64, 3, what);
      destroy(ch);
    }
  }
  return 0;
}

int run_sequence() {
  fake_chain_set_compute(1);
  // flat B: a 32-row call runs on the 32x64 loader-wave tile. Plain: 1 x 2 tiles, two layers; skinny: G = 2, two layers
  Chain plain = build(32, 2, {128, 128}, {64, 128}, {1, 1}, 0);
  Chain skinny = build(16, 2, {104, 64}, {72, 104}, {1, 1});
  std::vector<std::vector<char>> ref;
  reference(plain, ref);
  const unsigned *cnt_plain = nullptr, *cnt_skinny = nullptr;
  g_lcg = 20240607;
  long launches = 0;
  for (int e = 0; e < 6; ++e)
    for (int j = 0; j < 3; ++j) {
      if ((lcg() >> 9) & 1) {
        char what[64];
        snprintf(what, sizeof(what), "sequence: skinny, epoch %d", e);
        if (const unsigned *c = check_skinny(skinny, 2032, 32, 2, what)) cnt_skinny = c, ++launches;
      } else {
        poison_outputs(plain);
        fake_chain_clear(), fake_skinny_clear();
        const int ret = invoke(plain);
        xsmm_hip_synchronize();
        if (ret != 1 || fake_chain_launches() != 1 || fake_chain_launch(0)->form != FC_PLAIN || fake_chain_launch(0)->tiles_m != 1 || fake_chain_launch(0)->grid_n != 2)
          FAIL("sequence: the plain chain did not launch as 1 x 2 tiles (returned %d, %d launches)", ret, fake_chain_launches());
        else cnt_plain = fake_chain_launch(0)->a.cnt, ++launches;
        if (!outputs_are(plain, ref, "sequence: plain")) FAIL("sequence: the plain chain's outputs differ in epoch %d", e);
      }
    }
  if (!cnt_plain || cnt_plain != cnt_skinny) FAIL("SEQUENCE: the skinny chain and the plain chain with the same G and layer count do not share a counter block");
  printf("sequence: %ld launches, shared block %d, %d + %d counter mismatches\n", launches, cnt_plain == cnt_skinny, fake_chain_counter_mismatches(), fake_skinny_counter_mismatches());
  destroy(plain), destroy(skinny);
  return 0;
}

int run_probation() {
  fake_chain_set_compute(1);
  Chain ch = build(8, 0, {104, 104, 104}, {72, 104, 104}, {1, 1, 1});
  std::vector<std::vector<char>> ref;
  reference(ch, ref);
  xsmm_hip_set_chain_skinny(32);
  fake_chain_clear(), fake_skinny_clear();
  fake_skinny_starve(1, 1);
  const int ret = invoke(ch);
  xsmm_hip_synchronize();
  if (ret != 0) FAIL("PROBATION: the starved first launch returned %d", ret);
  if (fake_skinny_launches() != 1 || !fake_skinny_launch(0)->starved || fake_gemm_launches() != ch.n) FAIL("PROBATION: %d skinny launches, %d single launches", fake_skinny_launches(), fake_gemm_launches());
  if (!outputs_are(ch, ref, "probation")) FAIL("PROBATION: the outputs are not the calls' one by one");
  poison_outputs(ch);
  fake_chain_clear(), fake_skinny_clear();
  const int ret2 = invoke(ch); // every later chain invoke runs call by call
  xsmm_hip_synchronize();
  if (ret2 != 0 || fake_skinny_launches() != 0 || fake_gemm_launches() != ch.n) FAIL("PROBATION: a later chain invoke was launched");
  if (!outputs_are(ch, ref, "after probation")) FAIL("PROBATION: the later invoke's outputs are wrong");
  if (xsmm_hip_chain_status() != 0) FAIL("PROBATION: xsmm_hip_chain_status counts %ld repairs (nothing was journaled)", (long)xsmm_hip_chain_status());
  xsmm_hip_set_chain_skinny(0);
  printf("probation: starved first launch ran call by call, chains off afterwards\n");
  destroy(ch);
  return 0;
}
} // namespace

int main(int argc, char **argv) {
  const char *mode = argc > 1 ? argv[1] : "";
  setvbuf(stdout, nullptr, _IOLBF, 0);
  xsmm_hip_set_async(1);
  if (!strcmp(mode, "args")) run_args();
  else if (!strcmp(mode, "sequence")) run_sequence();
  else if (!strcmp(mode, "probation")) run_probation();
  else if (!strcmp(mode, "sanitize")) run_args(), run_sequence();
  else {
    fprintf(stderr, "usage: driver args | sequence | probation | sanitize\n");
    return 2;
  }
  if (fake_chain_counter_mismatches() || fake_skinny_counter_mismatches()) FAIL("COUNTER MODEL: %d + %d mismatches", fake_chain_counter_mismatches(), fake_skinny_counter_mismatches());
  if (g_fail) {
    printf("%d checks FAILED\n", g_fail);
    return 1;
  }
  printf("OK\n");
  return 0;
}
