// driver.cpp - TEST INFRASTRUCTURE for tests/test_split_scratch.py, never part of the product library: a walk of split_scratch_for
// (tpp-mlir_amd/csrc/split_scratch.h, the per (device, stream) scratch block of the split kernels) on a CPU, over the fake HIP host entry
// points of tests/tsan/fake_hip_host.h. The blocks are per process and never freed, so the walk is ONE sequence; every step checks what the
// header promises and how many "device" allocations are live (a block is two: its counters and its partial area).
//   1 first use: a 1 MiB partial area, SPLIT_MAX_TILES zeroed counters; the same stream again: the same block, nothing allocated
//   2 growth: the area doubles to the launch (2, 4 MiB), the block and its counters stay, the old area is freed
//   3 the cap: a launch of exactly SPLIT_SCRATCH_FLOATS fits (32 MiB); one float more is refused and changes nothing
//   4 tiles: SPLIT_MAX_TILES fit, one more is refused and changes nothing
//   5 a stream that is being captured: nullptr, for a stream that has a block and for one that has none, and nothing is allocated;
//     after the capture the block is the one from before
//   6 sixteen (device, stream) pairs - the null stream is one of them - get a block each, all distinct; the 17th is refused and
//     allocates nothing, also when asked again; the sixteen keep their blocks, and one of them may still grow
#include <hip/hip_runtime.h>

#include <cstdio>
#include <set>

#include "../../tpp-mlir_amd/csrc/split_scratch.h"
#include "../tsan/fake_hip_host.h"

using tpp::SplitScratch;
using tpp::split_scratch_for;

static int g_fail = 0, g_checks = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    ++g_checks;                                                              \
    if (!(cond)) {                                                           \
      ++g_fail;                                                              \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);                 \
    }                                                                        \
  } while (0)

static size_t live() { // "device" allocations of the fake
  std::lock_guard<std::mutex> lk(g_mu);
  return g_dev.size();
}
static size_t size_of(const void *p) { // ... and the bytes of the one that starts at p (0: none does)
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_dev.find((uintptr_t)p);
  return it == g_dev.end() ? 0 : it->second;
}
static hipStream_t stream(int i) { return (hipStream_t)(uintptr_t)(0x1000 + 0x100 * i); } // (the fake never looks inside a stream)

int main() {
  const size_t MiB = (size_t)1 << 18; // floats
  const hipStream_t s0 = stream(0);
  CHECK(live() == 0);

  // 1 first use and reuse (the fake's default answer: no stream is being captured)
  const SplitScratch *b0 = split_scratch_for(s0, 1, 1);
  CHECK(b0 != nullptr);
  if (!b0) return printf("FAIL: no block at all\n"), 1;
  CHECK(b0->device == 0 && b0->stream == s0 && b0->floats == MiB && live() == 2);
  CHECK(size_of(b0->partial) == MiB * sizeof(float) && size_of(b0->cnt) == tpp::SPLIT_MAX_TILES * sizeof(unsigned));
  bool zero = true;
  for (int i = 0; i < tpp::SPLIT_MAX_TILES; ++i) zero = zero && b0->cnt[i] == 0;
  CHECK(zero);
  const unsigned *cnt0 = b0->cnt;
  const float *area = b0->partial;
  CHECK(split_scratch_for(s0, 7, (long long)MiB) == b0 && b0->partial == area && b0->floats == MiB && live() == 2);
  printf("first use: 1 MiB, %d zeroed counters, reused\n", tpp::SPLIT_MAX_TILES);

  // 2 growth by doubling: same block, same counters, a new area of the next power of two, the old one freed
  CHECK(split_scratch_for(s0, 1, (long long)MiB + 1) == b0 && b0->floats == 2 * MiB && b0->cnt == cnt0 && live() == 2);
  CHECK(size_of(b0->partial) == 2 * MiB * sizeof(float));
  CHECK(split_scratch_for(s0, 1, 3 * (long long)MiB) == b0 && b0->floats == 4 * MiB && b0->cnt == cnt0 && live() == 2);
  CHECK(size_of(b0->partial) == 4 * MiB * sizeof(float));
  area = b0->partial;
  CHECK(split_scratch_for(s0, 1, 1) == b0 && b0->partial == area && b0->floats == 4 * MiB && live() == 2); // (never shrinks)
  printf("growth: 2 MiB, 4 MiB, one area live\n");

  // 3 the cap
  CHECK(split_scratch_for(s0, 1, (long long)tpp::SPLIT_SCRATCH_FLOATS + 1) == nullptr && b0->floats == 4 * MiB && b0->partial == area && live() == 2);
  CHECK(split_scratch_for(s0, 1, (long long)tpp::SPLIT_SCRATCH_FLOATS) == b0 && b0->floats == tpp::SPLIT_SCRATCH_FLOATS && live() == 2);
  CHECK(size_of(b0->partial) == tpp::SPLIT_SCRATCH_FLOATS * sizeof(float));
  CHECK(split_scratch_for(s0, 1, (long long)tpp::SPLIT_SCRATCH_FLOATS + 1) == nullptr && b0->floats == tpp::SPLIT_SCRATCH_FLOATS && live() == 2);
  printf("cap: %zu floats fit, one more is refused\n", (size_t)tpp::SPLIT_SCRATCH_FLOATS);

  // 4 arrival counters
  CHECK(split_scratch_for(s0, tpp::SPLIT_MAX_TILES, 1) == b0 && live() == 2);
  CHECK(split_scratch_for(s0, tpp::SPLIT_MAX_TILES + 1, 1) == nullptr && live() == 2);
  CHECK(split_scratch_for(stream(1), tpp::SPLIT_MAX_TILES + 1, 1) == nullptr && live() == 2); // (a refused launch takes no block either)
  printf("tiles: %d fit, one more is refused\n", tpp::SPLIT_MAX_TILES);

  // 5 a capturing stream
  area = b0->partial;
  CHECK(fake_hip_set_capturing(1) == 0);
  CHECK(split_scratch_for(s0, 1, 1) == nullptr && live() == 2);        // it has a block: the captured launch still must not use it
  CHECK(split_scratch_for(stream(1), 1, 1) == nullptr && live() == 2); // it has none: and gets none
  CHECK(fake_hip_set_capturing(0) == 1);
  CHECK(split_scratch_for(s0, 1, 1) == b0 && b0->partial == area && b0->cnt == cnt0 && live() == 2);
  printf("capture: nullptr, nothing allocated\n");

  // 6 sixteen pairs, then none: stream(1) .. stream(14) and the null stream join s0
  std::set<const SplitScratch *> blocks{b0};
  std::set<const void *> areas{b0->partial, b0->cnt};
  const SplitScratch *mine[tpp::SPLIT_MAX_BLOCKS] = {b0};
  for (int i = 1; i < tpp::SPLIT_MAX_BLOCKS; ++i) {
    const hipStream_t s = i == tpp::SPLIT_MAX_BLOCKS - 1 ? (hipStream_t) nullptr : stream(i);
    const SplitScratch *b = split_scratch_for(s, 1, 1);
    CHECK(b != nullptr);
    if (!b) break;
    mine[i] = b;
    CHECK(b->stream == s && b->floats == MiB && live() == 2 * (size_t)(i + 1));
    CHECK(blocks.insert(b).second && areas.insert(b->partial).second && areas.insert(b->cnt).second);
  }
  const size_t full = live();
  CHECK(full == 2 * (size_t)tpp::SPLIT_MAX_BLOCKS);
  CHECK(split_scratch_for(stream(40), 1, 1) == nullptr && live() == full); // pair 17
  CHECK(split_scratch_for(stream(40), 1, 1) == nullptr && live() == full); // ... however often it asks
  CHECK(split_scratch_for(stream(41), 1, 1) == nullptr && live() == full);
  for (int i = 0; i < tpp::SPLIT_MAX_BLOCKS; ++i) {
    const hipStream_t s = i == tpp::SPLIT_MAX_BLOCKS - 1 ? (hipStream_t) nullptr : stream(i);
    CHECK(split_scratch_for(s, 1, 1) == mine[i]);
  }
  CHECK(split_scratch_for(stream(3), 1, (long long)MiB + 1) == mine[3] && mine[3]->floats == 2 * MiB && live() == full); // a holder still grows
  printf("pairs: %d blocks, the next stream is refused\n", tpp::SPLIT_MAX_BLOCKS);

  printf("%d checks, %d failed\n", g_checks, g_fail);
  if (g_fail) return 1;
  printf("OK\n");
  return 0;
}
