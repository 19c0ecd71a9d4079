// driver.cpp - TEST INFRASTRUCTURE (tests/test_host_cache.py): the host cache of csrc/host_cache.cpp, driven through the C-ABI on
// HOST buffers the way an unmodified tpp-run would (memref globals / malloc'ed intermediates, lib/TPP/Runner/MLIRBench.cpp:207-246),
// with runtime.cpp + host_cache.cpp compiled unchanged against tests/tsan/fake_hip.cpp ("device" memory = malloc'ed blocks, kernels =
// scalar loops on the launching thread). The REAL kernel interface is used: userfaultfd async write-protect + PAGEMAP_SCAN.
// Every scenario runs twice - cache off (the plain per-invoke mirror) and cache on - and the host-visible results must be identical
// bit for bit; the counters say whether the cache did what it claims (no upload when nothing changed, one page when one page changed).
// Exit code 0 + a last line "OK"; 77 = the kernel lacks the interface (the test skips).
#include "../../include/tpp_xsmm_abi.h"
#include <cstddef>
extern "C" int hipMalloc(void **, size_t); // the fake device allocator of tests/tsan/fake_hip.cpp (hipError_t is an int-sized enum)
extern "C" int hipFree(void *);
#include <fcntl.h>
#include <malloc.h>
#include <sys/mman.h>
#include <unistd.h>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

static int g_fail = 0;
#define EXPECT(c, ...)                                  \
  do {                                                  \
    if (!(c)) {                                         \
      ++g_fail;                                         \
      printf("FAIL %s:%d: %s - ", __FILE__, __LINE__, #c); \
      printf(__VA_ARGS__);                              \
      printf("\n");                                     \
    }                                                   \
  } while (0)

static void fill(float *p, size_t n, unsigned seed) {
  for (size_t i = 0; i < n; ++i) {
    seed = seed * 1664525u + 1013904223u;
    p[i] = (float)((int)((seed >> 16) & 7) - 3) * 0.25f;
  }
}
struct Stats {
  int64_t v[10];
  Stats() { xsmm_hip_host_cache_stats(v); }
  int64_t extents() const { return v[0]; }
  int64_t uploaded() const { return v[2]; }
  int64_t written_back() const { return v[4]; }
  int64_t skipped() const { return v[5]; }
  int64_t fast() const { return v[7]; }
  int64_t dropped() const { return v[9]; }
};

// an allocation that is deliberately NOT page aligned (memref.alloc: 64-byte alignment inside malloc(n + 64))
// HC_ALIGNED=1 (the ThreadSanitizer run): whole pages instead - uploads are page-granular, and the bytes of a shared edge page that
// belong to somebody else's live heap object would read as a (harmless, by design) race to the sanitizer
static const bool g_aligned = getenv("HC_ALIGNED") != nullptr;
static float *host_alloc(size_t n_floats, std::vector<void *> &keep) {
  if (g_aligned) {
    void *p = aligned_alloc(4096, (n_floats * 4 + 4095) & ~(size_t)4095);
    keep.push_back(p);
    return (float *)p;
  }
  char *raw = (char *)malloc(n_floats * 4 + 64 + 192);
  keep.push_back(raw);
  return (float *)((((uintptr_t)raw + 63) & ~(uintptr_t)63) + 192);
}

// ---- scenario 1: synchronous mode (the reference's contract): a loop of whole-matrix BRGEMMs, the host edits inputs in between
static void scenario_sync(bool cache, std::vector<float> &result, int64_t *uploaded_steady, int64_t *uploaded_one_page) {
  xsmm_hip_set_async(0);
  xsmm_hip_set_host_cache(cache ? 1 : 0);
  const int M = 96, N = 160, K = 64, BR = 4;
  std::vector<void *> keep;
  float *A = host_alloc((size_t)M * K * BR, keep), *B = host_alloc((size_t)K * BR * N, keep), *C = host_alloc((size_t)M * N, keep);
  float *bias = host_alloc(N, keep);
  fill(A, (size_t)M * K * BR, 1);
  fill(B, (size_t)K * BR * N, 2);
  fill(C, (size_t)M * N, 3);
  fill(bias, N, 4);
  const int64_t h = xsmm_brgemm_dispatch(XSMM_DTYPE_F32, M, N, K, K * BR, N, N, K, (int64_t)K * N, 0); // C += sum_b A_b B_b
  const int64_t hf = xsmm_fused_brgemm_dispatch(XSMM_DTYPE_F32, M, N, K, K * BR, N, N, K, (int64_t)K * N, XSMM_GEMM_FLAG_BETA_0, 0, XSMM_UNARY_RELU,
                                                XSMM_BINARY_FLAG_BCAST_COL_IN_0, XSMM_BINARY_ADD);
  const int64_t hr = xsmm_unary_dispatch(XSMM_UNARY_RELU, XSMM_DTYPE_F32, M, N, N, N, 0);
  xsmm_brgemm_invoke(XSMM_DTYPE_F32, h, A, 0, B, 0, C, 0, BR);
  result.insert(result.end(), C, C + M * N); // visible on return
  xsmm_brgemm_invoke(XSMM_DTYPE_F32, h, A, 0, B, 0, C, 0, BR); // nothing changed on the host: no upload
  const Stats s0;
  xsmm_brgemm_invoke(XSMM_DTYPE_F32, h, A, 0, B, 0, C, 0, BR);
  const Stats s1;
  *uploaded_steady = s1.uploaded() - s0.uploaded();
  result.insert(result.end(), C, C + M * N);
  // the host edits one element of A (one page), and a stretch of B through a system call (read(2) straight into the operand)
  A[(size_t)M * K * BR / 2] = 7.0f;
  const Stats s2;
  xsmm_brgemm_invoke(XSMM_DTYPE_F32, h, A, 0, B, 0, C, 0, BR);
  const Stats s3;
  *uploaded_one_page = s3.uploaded() - s2.uploaded();
  result.insert(result.end(), C, C + M * N);
  int z = open("/dev/zero", O_RDONLY);
  if (read(z, B + 1000, 8192) != 8192) abort();
  close(z);
  xsmm_brgemm_invoke(XSMM_DTYPE_F32, h, A, 0, B, 0, C, 0, BR);
  result.insert(result.end(), C, C + M * N);
  // the host edits the OUTPUT between two accumulating invokes
  for (int i = 0; i < M * N; i += 97) C[i] = -1.0f;
  xsmm_brgemm_invoke(XSMM_DTYPE_F32, h, A, 0, B, 0, C, 0, BR);
  result.insert(result.end(), C, C + M * N);
  // fused (BETA_0 + bias + relu), then an in-place relu on the output, then the host reads it
  xsmm_fused_brgemm_invoke(XSMM_DTYPE_F32, hf, A, 0, B, 0, C, 0, bias, 0, BR);
  bias[5] = 100.0f;
  xsmm_fused_brgemm_invoke(XSMM_DTYPE_F32, hf, A, 0, B, 0, C, 0, bias, 0, BR);
  for (int i = 0; i < M * N; i += 5) C[i] = -C[i];
  xsmm_unary_invoke(XSMM_DTYPE_F32, hr, C, 0, C, 0);
  result.insert(result.end(), C, C + M * N);
  // tiles of one row-major matrix from four threads (adjacent tiles share pages and rows): zero + brgemm per tile
  {
    const int TS = 32, KB = 32;
    const int64_t hz = xsmm_unary_dispatch(XSMM_UNARY_ZERO, XSMM_DTYPE_F32, TS, TS, N, N, 0);
    const int64_t hg = xsmm_brgemm_dispatch(XSMM_DTYPE_F32, TS, TS, KB, K * BR, N, N, KB, (int64_t)KB * N, 0);
    std::vector<std::thread> th;
    for (int t = 0; t < 4; ++t)
      th.emplace_back([&, t] {
        const int tiles_n = N / TS, tiles = (M / TS) * tiles_n;
        for (int q = t; q < tiles; q += 4) {
          const int i = q / tiles_n, j = q % tiles_n;
          xsmm_unary_invoke(XSMM_DTYPE_F32, hz, C, 0, C, (int64_t)i * TS * N + j * TS);
          xsmm_brgemm_invoke(XSMM_DTYPE_F32, hg, A, (int64_t)i * TS * K * BR, B, j * TS, C, (int64_t)i * TS * N + j * TS, (K * BR) / KB);
        }
      });
    for (auto &x : th) x.join();
    result.insert(result.end(), C, C + M * N);
  }
  xsmm_hip_set_host_cache(0);
  for (void *p : keep) free(p);
}

// ---- scenario 2: asynchronous mode + tile queue: a 3-layer MLP as 32x32x32 tile invokes on HOST buffers (what the compiler emits,
// pass-convert-mlp-to-parallel-tile.mlir:80-88), several timing-loop iterations per synchronisation epoch
static void scenario_async(bool cache, int threads, std::vector<float> &result, int64_t *uploaded_epoch2, int64_t *uploaded_after_edit, int64_t *fast_invokes) {
  xsmm_hip_set_host_cache(cache ? 1 : 0);
  xsmm_hip_set_async(1);
  xsmm_hip_set_tile_queue(getenv("HC_NOQUEUE") ? 0 : 1);
  const int M = 128, W = 128, TS = 32, L = 3, NB = W / TS, MB = M / TS, KBk = W / TS;
  std::vector<void *> keep;
  float *act[L + 1], *Wt[L], *bias[L];
  for (int l = 0; l <= L; ++l) act[l] = host_alloc((size_t)M * W, keep); // packed [MB][KB][32][32]
  for (int l = 0; l < L; ++l) {
    Wt[l] = host_alloc((size_t)W * W, keep); // packed [NB][KB][32][32]
    bias[l] = host_alloc(W, keep);
    fill(Wt[l], (size_t)W * W, 10 + l);
    fill(bias[l], W, 20 + l);
  }
  fill(act[0], (size_t)M * W, 5);
  for (int l = 1; l <= L; ++l) memset(act[l], 0, (size_t)M * W * 4);
  const int64_t h = xsmm_fused_brgemm_dispatch(XSMM_DTYPE_F32, TS, TS, TS, TS, TS, TS, TS * TS, TS * TS, XSMM_GEMM_FLAG_BETA_0, 0, XSMM_UNARY_RELU,
                                               XSMM_BINARY_FLAG_BCAST_COL_IN_0, XSMM_BINARY_ADD);
  auto iteration = [&]() {
    for (int l = 0; l < L; ++l) {
      auto tile = [&](int q) {
        const int i = q / NB, j = q % NB;
        xsmm_fused_brgemm_invoke(XSMM_DTYPE_F32, h, act[l], (int64_t)i * KBk * TS * TS, Wt[l], (int64_t)j * KBk * TS * TS, act[l + 1], (int64_t)(i * NB + j) * TS * TS,
                                 bias[l], j * TS, KBk);
      };
      if (threads <= 1) {
        for (int q = 0; q < MB * NB; ++q) tile(q);
      } else {
        std::vector<std::thread> th;
        for (int t = 0; t < threads; ++t)
          th.emplace_back([&, t] {
            for (int q = t; q < MB * NB; q += threads) tile(q);
          });
        for (auto &x : th) x.join();
      }
    }
  };
  // epoch 1: warm-up + a timed loop, like TppRunnerWrapper.cpp:115-130
  iteration();
  xsmm_hip_synchronize();
  result.insert(result.end(), act[L], act[L] + M * W);
  const Stats s0;
  int64_t t0 = perf_start_timer();
  for (int it = 0; it < 5; ++it) iteration();
  (void)perf_stop_timer(t0);
  const Stats s1;
  *uploaded_epoch2 = s1.uploaded() - s0.uploaded();
  *fast_invokes = s1.fast() - s0.fast();
  result.insert(result.end(), act[L], act[L] + M * W);
  result.insert(result.end(), act[1], act[1] + M * W);
  // between two epochs the host edits one weight and the input
  Wt[1][777] = 3.0f;
  act[0][1] = -2.0f;
  const Stats s2;
  t0 = perf_start_timer();
  for (int it = 0; it < 3; ++it) iteration();
  (void)perf_stop_timer(t0);
  const Stats s3;
  *uploaded_after_edit = s3.uploaded() - s2.uploaded();
  result.insert(result.end(), act[L], act[L] + M * W);
  xsmm_hip_set_tile_queue(0);
  xsmm_hip_set_async(0);
  xsmm_hip_set_host_cache(0);
  for (void *p : keep) free(p);
}

// ---- scenario 3: lifetime without a hook: buffers are freed and their addresses come back with other contents
static void scenario_lifetime(bool cache, std::vector<float> &result, int64_t *dropped_or_reuploaded) {
  xsmm_hip_set_async(0);
  xsmm_hip_set_host_cache(cache ? 1 : 0);
  const int M = 256, N = 256, K = 256;
  const int64_t h = xsmm_gemm_dispatch(XSMM_DTYPE_F32, M, N, K, K, N, N, XSMM_GEMM_FLAG_BETA_0);
  const Stats s0;
  for (int round = 0; round < 4; ++round) {
    // large chunks: glibc serves them with mmap and gives the pages back on free (the next malloc usually returns the same address)
    mallopt(M_MMAP_THRESHOLD, round < 2 ? 128 * 1024 : 64 * 1024 * 1024); // rounds 2-3: from the brk heap instead (free keeps the pages)
    float *A = (float *)malloc((size_t)M * K * 4), *B = (float *)malloc((size_t)K * N * 4), *C = (float *)malloc((size_t)M * N * 4);
    fill(A, (size_t)M * K, 100 + round);
    fill(B, (size_t)K * N, 200 + round);
    xsmm_gemm_invoke(XSMM_DTYPE_F32, h, A, 0, B, 0, C, 0);
    result.insert(result.end(), C, C + M * N);
    free(A);
    free(B);
    free(C);
  }
  // an mmap'ed buffer replaced in place by a file mapping (cannot be tracked: plain path), then by anonymous memory again
  {
    const size_t bytes = (size_t)M * K * 4;
    float *A = (float *)mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    float *B = (float *)malloc((size_t)K * N * 4), *C = (float *)malloc((size_t)M * N * 4);
    fill(A, (size_t)M * K, 300);
    fill(B, (size_t)K * N, 301);
    xsmm_gemm_invoke(XSMM_DTYPE_F32, h, A, 0, B, 0, C, 0);
    result.insert(result.end(), C, C + M * N);
    char name[] = "/tmp/hc_driver_XXXXXX";
    int fd = mkstemp(name);
    unlink(name);
    if (ftruncate(fd, (off_t)bytes) != 0) abort();
    float *A2 = (float *)mmap(A, bytes, PROT_READ | PROT_WRITE, MAP_SHARED | MAP_FIXED, fd, 0);
    if (A2 != A) abort();
    fill(A, (size_t)M * K, 302);
    xsmm_gemm_invoke(XSMM_DTYPE_F32, h, A, 0, B, 0, C, 0);
    result.insert(result.end(), C, C + M * N);
    float *A3 = (float *)mmap(A, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_FIXED, -1, 0);
    if (A3 != A) abort();
    fill(A, (size_t)M * K, 303);
    xsmm_gemm_invoke(XSMM_DTYPE_F32, h, A, 0, B, 0, C, 0);
    result.insert(result.end(), C, C + M * N);
    close(fd);
    munmap(A, bytes);
    free(B);
    free(C);
  }
  const Stats s1;
  *dropped_or_reuploaded = (s1.dropped() - s0.dropped()) + (s1.uploaded() - s0.uploaded());
  mallopt(M_MMAP_THRESHOLD, 128 * 1024);
  xsmm_hip_set_host_cache(0);
}

// ---- scenario 4 (cache on only): the asynchronous contract broken - an output is unmapped before the synchronisation point. The
// write-back must notice (the kernel no longer vouches for the range) and leave the address alone instead of faulting.
static void scenario_freed_before_sync() {
  xsmm_hip_set_host_cache(1);
  xsmm_hip_set_async(1);
  const int M = 128, N = 128, K = 128;
  const int64_t h = xsmm_gemm_dispatch(XSMM_DTYPE_F32, M, N, K, K, N, N, XSMM_GEMM_FLAG_BETA_0);
  const size_t bytes = (size_t)M * N * 4;
  float *A = (float *)mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
  float *B = (float *)mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
  float *C = (float *)mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
  float *C2 = (float *)mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
  fill(A, (size_t)M * K, 1);
  fill(B, (size_t)K * N, 2);
  xsmm_gemm_invoke(XSMM_DTYPE_F32, h, A, 0, B, 0, C, 0);
  xsmm_gemm_invoke(XSMM_DTYPE_F32, h, A, 0, B, 0, C2, 0);
  munmap(C, bytes); // too early: the contract says after the synchronisation point
  const Stats s0;
  xsmm_hip_synchronize();
  const Stats s1;
  EXPECT(s1.skipped() - s0.skipped() >= (int64_t)(bytes / 4096), "pages not written back: %ld", (long)(s1.skipped() - s0.skipped()));
  float ref = 0.0f;
  for (int k = 0; k < K; ++k) ref += A[k] * B[(size_t)k * N];
  EXPECT(C2[0] == ref, "the surviving output was written back: %g vs %g", C2[0], ref);
  xsmm_hip_set_async(0);
  xsmm_hip_set_host_cache(0);
  munmap(A, bytes);
  munmap(B, bytes);
  munmap(C2, bytes);
}

// ---- scenario 5: a timing loop of ONE whole-matrix BRGEMM in asynchronous mode (BASELINE config 2 on host buffers), then the same
// handle on device pointers with the cache still on, then everything switched off
static void scenario_c2_async() {
  xsmm_hip_set_host_cache(1);
  xsmm_hip_set_async(1);
  const int M = 256, N = 256, K = 64, BR = 4;
  std::vector<void *> keep;
  float *A = host_alloc((size_t)M * K * BR, keep), *B = host_alloc((size_t)K * BR * N, keep), *C = host_alloc((size_t)M * N, keep);
  fill(A, (size_t)M * K * BR, 1);
  fill(B, (size_t)K * BR * N, 2);
  memset(C, 0, (size_t)M * N * 4);
  const int64_t h = xsmm_brgemm_dispatch(XSMM_DTYPE_F32, M, N, K, K * BR, N, N, K, (int64_t)K * N, XSMM_GEMM_FLAG_BETA_0);
  xsmm_brgemm_invoke(XSMM_DTYPE_F32, h, A, 0, B, 0, C, 0, BR);
  xsmm_hip_synchronize();
  const Stats s0;
  const int64_t t0 = perf_start_timer();
  for (int i = 0; i < 200; ++i) xsmm_brgemm_invoke(XSMM_DTYPE_F32, h, A, 0, B, 0, C, 0, BR);
  (void)perf_stop_timer(t0);
  const Stats s1;
  EXPECT(s1.fast() - s0.fast() >= 199, "lock-free translations: %ld", (long)(s1.fast() - s0.fast()));
  EXPECT(s1.uploaded() - s0.uploaded() <= 8 * 4096, "uploaded in the loop: %ld", (long)(s1.uploaded() - s0.uploaded()));
  float *dA, *dB, *dC;
  hipMalloc((void **)&dA, (size_t)M * K * BR * 4);
  hipMalloc((void **)&dB, (size_t)K * BR * N * 4);
  hipMalloc((void **)&dC, (size_t)M * N * 4);
  memcpy(dA, A, (size_t)M * K * BR * 4);
  memcpy(dB, B, (size_t)K * BR * N * 4);
  xsmm_brgemm_invoke(XSMM_DTYPE_F32, h, dA, 0, dB, 0, dC, 0, BR);
  xsmm_hip_synchronize();
  EXPECT(!memcmp(C, dC, (size_t)M * N * 4), "host-buffer result != device-pointer result");
  xsmm_hip_set_async(0);
  xsmm_hip_set_host_cache(0);
  hipFree(dA);
  hipFree(dB);
  hipFree(dC);
  for (void *p : keep) free(p);
}

// ---- scenario 6: seeded COHERENCE PROGRAMS. A program is a random sequence of invokes, host edits, synchronisation points and mode
// switches over a few small host buffers, inside the contract of tpp_xsmm_abi.h (asynchronous mode: the host touches operands only
// directly behind a synchronisation point). Every byte of every buffer's mapping - padding and guard bytes included - is compared
// with a SHADOW copy that this file updates with its own plain loops, invoke by invoke in program order: the expected bytes never come
// from the runtime. Data are small integers, so every sum is exact in f32 whatever the order of the additions (asserted).
namespace coh {
struct Rng {
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x2545F4914F6CDD1Dull) {}
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
  }
  int below(int n) { return (int)(next() % (uint32_t)n); }
  int small() { return below(7) - 3; }
};
static uint16_t bf16_of(float f) { // (exact for the small integers used here)
  uint32_t u;
  memcpy(&u, &f, 4);
  return (uint16_t)(u >> 16);
}
static float f32_of(uint16_t h) {
  const uint32_t u = (uint32_t)h << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
constexpr size_t OFF = 256;    // data start inside the mapping: 64-byte aligned, never page aligned (memref.alloc style)
constexpr size_t GUARD = 4096 + 320;
struct Buf {
  const char *name = "";
  int es = 4;
  size_t n = 0; // elements
  char *map = nullptr, *p = nullptr;
  size_t map_bytes = 0;
  std::vector<char> shadow; // of the whole mapping
  void create(const char *nm, int esz, size_t elems) {
    name = nm, es = esz, n = elems;
    map_bytes = (OFF + n * es + GUARD + 4095) & ~(size_t)4095;
    map = (char *)mmap(nullptr, map_bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
    if (map == MAP_FAILED) abort();
    p = map + OFF;
    memset(map, 0xA5, map_bytes);
    shadow.assign(map_bytes, (char)0xA5);
  }
  void destroy() { munmap(map, map_bytes); }
  char *sp() { return shadow.data() + OFF; }
  void set(size_t i, int v) { // the host writes element i - and the model with it
    if (es == 4) {
      const float f = (float)v;
      memcpy(p + i * 4, &f, 4);
      memcpy(sp() + i * 4, &f, 4);
    } else {
      const uint16_t h = bf16_of((float)v);
      memcpy(p + i * 2, &h, 2);
      memcpy(sp() + i * 2, &h, 2);
    }
  }
  float model(size_t i) {
    if (es == 4) {
      float f;
      memcpy(&f, sp() + i * 4, 4);
      return f;
    }
    uint16_t h;
    memcpy(&h, sp() + i * 2, 2);
    return f32_of(h);
  }
  float maxabs(size_t off, size_t rows, size_t cols, size_t ld) {
    float m = 0;
    for (size_t i = 0; i < rows; ++i)
      for (size_t j = 0; j < cols; ++j) m = std::max(m, std::fabs(model(off + i * ld + j)));
    return m;
  }
};

enum Kind { G_WHOLE, G_WHOLE_FUSED, G_TILE, U_RELU_SQ, U_RELU_TILE, U_ZERO_SQ, U_ZERO_TILE, U_IDENT_WIN, B_ADD_SQ, B_ADD_TILE, H_RELU, H_IDENT_WIN, H_ZERO_TILE, N_KINDS };
static const char *kind_name[N_KINDS] = {"brgemm", "fused_brgemm", "brgemm_tile", "relu_inplace", "relu_inplace_tile", "zero", "zero_tile", "identity_window",
                                         "add_bcast_col", "add_bcast_col_tile", "bf16_relu_inplace", "bf16_identity_window", "bf16_zero_tile"};
enum SyncKind { K_SYNCHRONIZE, K_PERF, K_ASYNC01, K_STREAM, K_CACHE, N_SYNC };
static const char *sync_name[N_SYNC] = {"synchronize", "perf_stop_timer", "set_async(0)+(1)", "set_stream", "set_host_cache(0)+(1)"};
constexpr int SQ = 64, KB = 32, BR = 2, FM = 64, FN = 192, TS = 32, WIN = 160, WIN_OFF = 16, HWIN = 48, HWIN_OFF = 8;
constexpr float IN_MAX = 16.0f;        // a GEMM input holds integers up to this ...
constexpr int MAX_ACCUMULATIONS = 6;   // ... and an output accumulates (beta 1) at most this often between two re-initialisations:
                                       // |C| <= 7 * (64 * 16 * 16 + 3) < 2^17, far below 2^24 (asserted on the model's values all the same)
// buffers: S0..S3 square f32 (inputs and outputs of whole-matrix GEMMs: one invoke's output is another's input), F the flat row-major
// f32 matrix whose tiles are narrow strided outputs, W a flat input, V the bias / broadcast row, H0 H1 bf16 squares
enum { S0, S1, S2, S3, F, W, V, H0, H1, N_BUFS };
struct Inv {
  int kind, a, b, c; // buffers: inputs a, b (or -1), output c
  int ti, tj, beta1;
};
struct Coverage {
  long pair[N_SYNC][3][2] = {}; // [sync kind in front of the segment][0: edit-then-invoke, 1: rewrite-an-output, 2: the host edits an output
                                // that a beta-1 invoke then reads][tile queue off / on]
  long kinds[N_KINDS] = {};
  long programs = 0, steps = 0, invokes = 0, edits = 0, syncs = 0, checks = 0;
};
static Coverage g_cov;

struct Program {
  uint64_t seed;
  bool cache;
  Rng rng;
  Buf buf[N_BUFS];
  int acc[N_BUFS] = {};
  int64_t h_whole[2], h_fused[2], h_tile[2], h_relu_sq, h_relu_tile, h_zero_sq, h_zero_tile, h_ident, h_add_sq, h_add_tile, h_hrelu, h_hident, h_hzero;
  bool async = false, other_stream = false, failed = false;
  int queue = 0, step = 0;
  std::vector<std::string> log;
  uint64_t digest = 1469598103934665603ull;
  Program(uint64_t sd, bool c) : seed(sd), cache(c), rng(sd) {}

  void note(const char *fmt, ...) {
    char line[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(line, sizeof line, fmt, ap);
    va_end(ap);
    char full[300];
    snprintf(full, sizeof full, "  step %d: %s", step, line);
    log.push_back(full);
    ++step;
    if (cache) ++g_cov.steps;
  }
  void fail(const char *what) {
    if (failed) return;
    failed = true;
    ++g_fail;
    printf("FAIL coherence program seed %llu (cache %s) at step %d: %s\n", (unsigned long long)seed, cache ? "on" : "off", step - 1, what);
    for (size_t i = log.size() > 14 ? log.size() - 14 : 0; i < log.size(); ++i) printf("%s\n", log[i].c_str());
  }
  void check() {
    if (cache) ++g_cov.checks;
    for (Buf &b : buf) {
      for (size_t i = 0; i < b.map_bytes; ++i) digest = (digest ^ (unsigned char)b.map[i]) * 1099511628211ull;
      if (!memcmp(b.map, b.shadow.data(), b.map_bytes)) continue;
      size_t i = 0;
      while (b.map[i] == b.shadow[i]) ++i;
      char what[200];
      const long e = ((long)i - (long)OFF) / b.es;
      snprintf(what, sizeof what, "buffer %s differs from the model at mapping byte %zu (element %ld of %zu: host %g, model %g)", b.name, i, e, b.n,
               i >= OFF && (size_t)e < b.n ? (b.es == 4 ? ((float *)b.p)[e] : f32_of(((uint16_t *)b.p)[e])) : 0.0, i >= OFF && (size_t)e < b.n ? b.model((size_t)e) : 0.0);
      fail(what);
      return;
    }
  }
  // ---- footprints (element offset, rows, cols, leading dimension) of an invoke's operands
  struct Fp {
    int b;
    size_t off, rows, cols, ld;
  };
  Fp out_fp(const Inv &v) {
    switch (v.kind) {
    case G_WHOLE: case G_WHOLE_FUSED: case U_RELU_SQ: case U_ZERO_SQ: case B_ADD_SQ: case H_RELU: return Fp{v.c, 0, SQ, SQ, SQ};
    case G_TILE: case U_RELU_TILE: case U_ZERO_TILE: case B_ADD_TILE: return Fp{v.c, (size_t)v.ti * TS * FN + v.tj * TS, TS, TS, FN};
    case U_IDENT_WIN: return Fp{v.c, WIN_OFF, FM, WIN, FN};
    case H_IDENT_WIN: return Fp{v.c, HWIN_OFF, SQ, HWIN, SQ};
    default: return Fp{v.c, (size_t)v.ti * TS * SQ + v.tj * TS, TS, TS, SQ}; // H_ZERO_TILE
    }
  }
  bool in_fp(const Inv &v, Fp *f) { // one input worth editing
    switch (v.kind) {
    case G_WHOLE: case G_WHOLE_FUSED: *f = Fp{v.a, 0, SQ, SQ, SQ}; return true;
    case G_TILE: *f = Fp{v.a, (size_t)v.ti * TS * SQ, TS, SQ, SQ}; return true;
    case U_RELU_SQ: case H_RELU: case U_RELU_TILE: *f = out_fp(v); return true;
    case U_IDENT_WIN: *f = Fp{v.a, 0, FM, WIN, FN}; return true;
    case H_IDENT_WIN: *f = Fp{v.a, 0, SQ, HWIN, SQ}; return true;
    case B_ADD_SQ: *f = Fp{v.a, 0, SQ, SQ, SQ}; return true;
    case B_ADD_TILE: *f = Fp{V, (size_t)v.tj * TS, 1, TS, TS}; return true;
    default: return false; // the zero ops read nothing
    }
  }
  // the exactness precondition: GEMM inputs are integers up to IN_MAX, an output accumulates a bounded number of times
  bool eligible(const Inv &v) {
    if (v.kind == G_WHOLE || v.kind == G_WHOLE_FUSED) {
      if (v.c == v.a || v.c == v.b) return false;
      if (buf[v.a].maxabs(0, SQ, SQ, SQ) > IN_MAX || buf[v.b].maxabs(0, SQ, SQ, SQ) > IN_MAX) return false;
      return !v.beta1 || acc[v.c] < MAX_ACCUMULATIONS;
    }
    if (v.kind == G_TILE) return buf[v.a].maxabs((size_t)v.ti * TS * SQ, TS, SQ, SQ) <= IN_MAX && (!v.beta1 || acc[F] < MAX_ACCUMULATIONS);
    if (v.kind == B_ADD_SQ) return acc[v.c] < MAX_ACCUMULATIONS && buf[v.a].maxabs(0, SQ, SQ, SQ) < 8388608.0f;
    if (v.kind == B_ADD_TILE) return acc[F] < MAX_ACCUMULATIONS;
    return true;
  }
  void model_gemm(const Inv &v, bool fused, size_t oa, size_t lda, size_t ob, Buf &B, size_t ldb, size_t sb, size_t oc, size_t ldc, int m, int n, int voff) {
    Buf &A = buf[v.a], &C = buf[v.c];
    std::vector<float> out((size_t)m * n);
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < n; ++j) {
        double s = v.beta1 ? (double)C.model(oc + (size_t)i * ldc + j) : 0.0;
        for (int b = 0; b < BR; ++b)
          for (int k = 0; k < KB; ++k) s += (double)A.model(oa + (size_t)b * KB + (size_t)i * lda + k) * (double)B.model(ob + (size_t)b * sb + (size_t)k * ldb + j);
        if (fused) {
          s += (double)buf[V].model((size_t)voff + j);
          if (!(s > 0.0)) s = 0.0;
        }
        if (std::fabs(s) >= 16777216.0 || s != std::floor(s)) fail("exactness precondition broken: a model value is not an integer below 2^24");
        out[(size_t)i * n + j] = (float)s;
      }
    for (int i = 0; i < m; ++i) memcpy(C.sp() + (oc + (size_t)i * ldc) * 4, &out[(size_t)i * n], (size_t)n * 4);
  }
  void issue(const Inv &v) {
    const int64_t f32 = XSMM_DTYPE_F32, b16 = XSMM_DTYPE_BF16;
    const Fp o = out_fp(v);
    Buf &C = buf[v.c];
    note("invoke %s a=%s b=%s out=%s tile (%d,%d) beta %d", kind_name[v.kind], v.a >= 0 ? buf[v.a].name : "-", v.b >= 0 ? buf[v.b].name : "-", C.name, v.ti, v.tj, v.beta1);
    if (cache) {
      ++g_cov.invokes;
      ++g_cov.kinds[v.kind];
    }
    switch (v.kind) {
    case G_WHOLE:
      xsmm_brgemm_invoke(f32, h_whole[v.beta1], buf[v.a].p, 0, buf[v.b].p, 0, C.p, 0, BR);
      model_gemm(v, false, 0, SQ, 0, buf[v.b], SQ, (size_t)KB * SQ, 0, SQ, SQ, SQ, 0);
      break;
    case G_WHOLE_FUSED:
      xsmm_fused_brgemm_invoke(f32, h_fused[v.beta1], buf[v.a].p, 0, buf[v.b].p, 0, C.p, 0, buf[V].p, 0, BR);
      model_gemm(v, true, 0, SQ, 0, buf[v.b], SQ, (size_t)KB * SQ, 0, SQ, SQ, SQ, 0);
      break;
    case G_TILE:
      xsmm_brgemm_invoke(f32, h_tile[v.beta1], buf[v.a].p, (int64_t)v.ti * TS * SQ, buf[W].p, v.tj * TS, C.p, (int64_t)o.off, BR);
      model_gemm(v, false, (size_t)v.ti * TS * SQ, SQ, (size_t)v.tj * TS, buf[W], FN, (size_t)KB * FN, o.off, FN, TS, TS, 0);
      break;
    case U_RELU_SQ: case U_RELU_TILE: case H_RELU: {
      const int64_t h = v.kind == U_RELU_SQ ? h_relu_sq : v.kind == U_RELU_TILE ? h_relu_tile : h_hrelu;
      xsmm_unary_invoke(C.es == 4 ? f32 : b16, h, C.p, (int64_t)o.off, C.p, (int64_t)o.off);
      for (size_t i = 0; i < o.rows; ++i)
        for (size_t j = 0; j < o.cols; ++j)
          if (!(C.model(o.off + i * o.ld + j) > 0.0f)) memset(C.sp() + (o.off + i * o.ld + j) * C.es, 0, C.es);
      break;
    }
    case U_ZERO_SQ: case U_ZERO_TILE: case H_ZERO_TILE: {
      const int64_t h = v.kind == U_ZERO_SQ ? h_zero_sq : v.kind == U_ZERO_TILE ? h_zero_tile : h_hzero;
      xsmm_unary_invoke(C.es == 4 ? f32 : b16, h, C.p, (int64_t)o.off, C.p, (int64_t)o.off);
      for (size_t i = 0; i < o.rows; ++i) memset(C.sp() + (o.off + i * o.ld) * C.es, 0, o.cols * C.es);
      break;
    }
    case U_IDENT_WIN: case H_IDENT_WIN: {
      Buf &I = buf[v.a];
      xsmm_unary_invoke(C.es == 4 ? f32 : b16, v.kind == U_IDENT_WIN ? h_ident : h_hident, I.p, 0, C.p, (int64_t)o.off);
      for (size_t i = 0; i < o.rows; ++i) memcpy(C.sp() + (o.off + i * o.ld) * C.es, I.sp() + i * o.ld * C.es, o.cols * C.es);
      break;
    }
    case B_ADD_SQ: case B_ADD_TILE: {
      Buf &L = buf[v.a];
      const size_t voff = v.kind == B_ADD_TILE ? (size_t)v.tj * TS : 0;
      const size_t loff = v.kind == B_ADD_TILE ? o.off : 0;
      xsmm_binary_invoke(f32, v.kind == B_ADD_SQ ? h_add_sq : h_add_tile, L.p, (int64_t)loff, buf[V].p, (int64_t)voff, C.p, (int64_t)o.off);
      for (size_t i = 0; i < o.rows; ++i)
        for (size_t j = 0; j < o.cols; ++j) {
          const float r = L.model(loff + i * o.ld + j) + buf[V].model(voff + j);
          if (std::fabs(r) >= 16777216.0f) fail("exactness precondition broken in add");
          memcpy(C.sp() + (o.off + i * o.ld + j) * 4, &r, 4);
        }
      break;
    }
    }
    const bool accumulates = v.beta1 || v.kind == B_ADD_SQ || v.kind == B_ADD_TILE;
    if (accumulates) ++acc[v.c];
    else if (v.kind == G_WHOLE || v.kind == G_WHOLE_FUSED || v.kind == U_ZERO_SQ) acc[v.c] = 0;
  }
  Inv random_inv() {
    for (;;) {
      Inv v{rng.below(N_KINDS), -1, -1, -1, rng.below(2), rng.below(FN / TS), rng.below(2)};
      switch (v.kind) {
      case G_WHOLE: case G_WHOLE_FUSED: v.a = S0 + rng.below(4), v.b = S0 + rng.below(4), v.c = S0 + rng.below(4); break;
      case G_TILE: v.a = S0 + rng.below(4), v.b = W, v.c = F; break;
      case U_RELU_SQ: case U_ZERO_SQ: v.c = S0 + rng.below(4); break;
      case U_RELU_TILE: case U_ZERO_TILE: v.c = F; break;
      case U_IDENT_WIN: v.a = W, v.c = F; break;
      case B_ADD_SQ: v.a = S0 + rng.below(4), v.b = V, v.c = S0 + rng.below(4); break;
      case B_ADD_TILE: v.a = F, v.b = V, v.c = F; break;
      case H_RELU: v.c = H0 + rng.below(2); break;
      case H_IDENT_WIN: v.a = H0, v.c = H1; break;
      case H_ZERO_TILE: v.c = H0 + rng.below(2), v.tj = rng.below(2); break;
      }
      if (v.kind == U_ZERO_SQ && rng.below(3)) continue; // (rarely: it wipes a whole buffer)
      if (eligible(v)) return v;
    }
  }
  // ---- host edits (the model follows): one element, a run of a few pages, a range written by a system call
  void edit_element(int b, size_t i) {
    Buf &x = buf[b];
    int nv = rng.small();
    if ((float)nv == x.model(i)) nv = nv == 3 ? -3 : nv + 1;
    note("host edit: %s[%zu] = %d", x.name, i, nv);
    x.set(i, nv);
    if (cache) ++g_cov.edits;
  }
  void edit_run(int b, size_t lo, size_t cnt) {
    Buf &x = buf[b];
    cnt = std::min(cnt, x.n - lo);
    note("host edit: %s[%zu .. %zu) refilled", x.name, lo, lo + cnt);
    for (size_t i = lo; i < lo + cnt; ++i) x.set(i, rng.small());
    if (cache) ++g_cov.edits;
  }
  void edit_syscall(int b, size_t lo, size_t cnt) {
    Buf &x = buf[b];
    cnt = std::min(cnt, x.n - lo);
    note("host edit: read(2) of %zu bytes into %s[%zu ..)", cnt * x.es, x.name, lo);
    const int z = open("/dev/zero", O_RDONLY);
    if (read(z, x.p + lo * x.es, cnt * x.es) != (ssize_t)(cnt * x.es)) abort();
    close(z);
    memset(x.sp() + lo * x.es, 0, cnt * x.es);
    if (cache) ++g_cov.edits;
  }
  void random_edit() {
    const int b = rng.below(N_BUFS);
    Buf &x = buf[b];
    const int how = rng.below(3);
    const size_t lo = (size_t)rng.below((int)x.n);
    if (how == 0) edit_element(b, lo);
    else if (how == 1) edit_run(b, lo, 1024 + (size_t)rng.below(2048)); // (f32: one to three pages)
    else edit_syscall(b, lo, 512 + (size_t)rng.below(2048));
    if (b <= S3 && how) acc[b] = 0;
  }
  void reinit_large_inputs() { // GEMM inputs that outgrew IN_MAX (they were outputs) are written afresh by the host - a run of a few pages
    for (int b = S0; b <= S3; ++b)
      if ((buf[b].maxabs(0, SQ, SQ, SQ) > IN_MAX || acc[b] >= MAX_ACCUMULATIONS) && rng.below(3)) {
        edit_run(b, 0, buf[b].n);
        acc[b] = 0;
      }
    if (acc[F] >= MAX_ACCUMULATIONS) {
      edit_run(F, 0, buf[F].n);
      acc[F] = 0;
    }
  }
  void sync_point(int kind, int64_t t0) {
    note("synchronisation point: %s", sync_name[kind]);
    if (cache) ++g_cov.syncs;
    switch (kind) {
    case K_SYNCHRONIZE: xsmm_hip_synchronize(); break;
    case K_PERF: (void)perf_stop_timer(t0); break;
    case K_ASYNC01:
      xsmm_hip_set_async(0);
      xsmm_hip_set_async(1);
      break;
    case K_STREAM:
      other_stream = !other_stream;
      xsmm_hip_set_stream(other_stream ? (void *)0x1000 : nullptr); // (the fake HIP: any non-null pointer is a stream)
      break;
    case K_CACHE:
      if (cache) {
        xsmm_hip_set_host_cache(0);
        xsmm_hip_set_host_cache(1);
      } else xsmm_hip_synchronize();
      break;
    }
  }
  void run() {
    if (cache) ++g_cov.programs;
    static const struct { const char *name; int es; size_t n; } shape[N_BUFS] = {{"S0", 4, SQ * SQ}, {"S1", 4, SQ * SQ}, {"S2", 4, SQ * SQ}, {"S3", 4, SQ * SQ}, {"F", 4, FM * FN},
                                                                             {"W", 4, FM * FN}, {"V", 4, FN}, {"H0", 2, SQ * SQ}, {"H1", 2, SQ * SQ}};
    for (int b = 0; b < N_BUFS; ++b) {
      buf[b].create(shape[b].name, shape[b].es, shape[b].n);
      for (size_t i = 0; i < buf[b].n; ++i) buf[b].set(i, rng.small());
    }
    const int64_t f32 = XSMM_DTYPE_F32, b16 = XSMM_DTYPE_BF16;
    for (int beta1 = 0; beta1 < 2; ++beta1) {
      const int64_t fl = beta1 ? 0 : XSMM_GEMM_FLAG_BETA_0;
      h_whole[beta1] = xsmm_brgemm_dispatch(f32, SQ, SQ, KB, SQ, SQ, SQ, KB, (int64_t)KB * SQ, fl);
      h_fused[beta1] = xsmm_fused_brgemm_dispatch(f32, SQ, SQ, KB, SQ, SQ, SQ, KB, (int64_t)KB * SQ, fl, 0, XSMM_UNARY_RELU, XSMM_BINARY_FLAG_BCAST_COL_IN_0, XSMM_BINARY_ADD);
      h_tile[beta1] = xsmm_brgemm_dispatch(f32, TS, TS, KB, SQ, FN, FN, KB, (int64_t)KB * FN, fl);
    }
    h_relu_sq = xsmm_unary_dispatch(XSMM_UNARY_RELU, f32, SQ, SQ, SQ, SQ, 0);
    h_relu_tile = xsmm_unary_dispatch(XSMM_UNARY_RELU, f32, TS, TS, FN, FN, 0);
    h_zero_sq = xsmm_unary_dispatch(XSMM_UNARY_ZERO, f32, SQ, SQ, SQ, SQ, 0);
    h_zero_tile = xsmm_unary_dispatch(XSMM_UNARY_ZERO, f32, TS, TS, FN, FN, 0);
    h_ident = xsmm_unary_dispatch(XSMM_UNARY_IDENTITY, f32, FM, WIN, FN, FN, 0);
    h_add_sq = xsmm_binary_dispatch(XSMM_BINARY_ADD, f32, SQ, SQ, SQ, SQ, SQ, XSMM_BINARY_FLAG_BCAST_COL_IN_1);
    h_add_tile = xsmm_binary_dispatch(XSMM_BINARY_ADD, f32, TS, TS, FN, TS, FN, XSMM_BINARY_FLAG_BCAST_COL_IN_1);
    h_hrelu = xsmm_unary_dispatch(XSMM_UNARY_RELU, b16, SQ, SQ, SQ, SQ, 0);
    h_hident = xsmm_unary_dispatch(XSMM_UNARY_IDENTITY, b16, SQ, HWIN, SQ, SQ, 0);
    h_hzero = xsmm_unary_dispatch(XSMM_UNARY_ZERO, b16, TS, TS, SQ, SQ, 0);
    xsmm_hip_set_async(0);
    xsmm_hip_set_tile_queue(0);
    xsmm_hip_set_host_cache(cache ? 1 : 0);
    std::vector<Inv> prev;
    int prev_kind = -1;
    bool prev_async = false;
    const int nseg = 7 + rng.below(4);
    for (int seg = 0; seg < nseg && !failed; ++seg) {
      const int mode = rng.below(5); // 0: synchronous, 1-2: asynchronous, 3-4: asynchronous + tile queue
      const int endkind = (int)((seed + (uint64_t)seg) % N_SYNC);
      std::vector<Inv> mine;
      if (mode == 0) {
        if (async) xsmm_hip_set_async(0);
        async = false;
        note("segment %d: synchronous", seg);
        const int64_t t0 = perf_start_timer();
        const int n = 4 + rng.below(5);
        for (int i = 0; i < n && !failed; ++i) {
          if (rng.below(3) == 0) {
            reinit_large_inputs();
            random_edit();
            continue;
          }
          Inv v = (!prev.empty() && rng.below(2)) ? prev[rng.below((int)prev.size())] : random_inv();
          if (!eligible(v)) v = random_inv();
          issue(v);
          mine.push_back(v);
          check(); // results visible on return
        }
        if (endkind != K_ASYNC01 && rng.below(2)) {
          sync_point(endkind, t0);
          check();
        }
        prev_async = false;
      } else {
        queue = mode >= 3;
        xsmm_hip_set_async(1);
        xsmm_hip_set_tile_queue(queue);
        async = true;
        note("segment %d: asynchronous, tile queue %d, behind %s", seg, queue, prev_kind >= 0 ? sync_name[prev_kind] : "the start");
        const int64_t t0 = perf_start_timer();
        // host phase: directly behind the synchronisation point, before the segment's first invoke
        reinit_large_inputs();
        for (int i = rng.below(3); i > 0; --i) random_edit();
        std::vector<Inv> plan;
        bool half[3] = {false, false, false};
        if (prev_async && !prev.empty()) {
          int want = 1 + rng.below(3); // bit 0: edit-then-invoke, bit 1: rewrite-an-output
          if (want & 1) { // the host edits an element an invoke of the last segment read (its mirror exists); the invoke runs again
            const Inv v = prev[rng.below((int)prev.size())];
            Fp f;
            if (in_fp(v, &f) && eligible(v)) {
              edit_element(f.b, f.off + (size_t)rng.below((int)f.rows) * f.ld + (size_t)rng.below((int)f.cols));
              if (eligible(v)) {
                plan.push_back(v);
                half[0] = true;
              }
            }
          }
          if (want & 2) { // an invoke of the last segment writes its output again; the host scribbles on that output first, so
                          // that a write-back that does not happen shows
            Inv v = prev[rng.below((int)prev.size())];
            const bool gemm = v.kind == G_WHOLE || v.kind == G_WHOLE_FUSED || v.kind == G_TILE;
            if (gemm && rng.below(3)) { // ... as the C of a beta-1 invoke, which READS the host's edit
              Inv v1 = v;
              v1.beta1 = 1;
              if (eligible(v1)) v = v1;
            }
            const Fp f = out_fp(v);
            if (eligible(v)) {
              edit_element(f.b, f.off + (size_t)rng.below((int)f.rows) * f.ld + (size_t)rng.below((int)f.cols));
              if (eligible(v)) {
                plan.push_back(v);
                half[1] = true;
                half[2] = gemm && v.beta1;
              }
            }
          }
        }
        for (const Inv &v : plan)
          if (eligible(v)) {
            issue(v);
            mine.push_back(v);
          } else half[0] = half[1] = half[2] = false; // (an earlier invoke of the plan changed what this one needs: not counted)
        for (int i = 2 + rng.below(5); i > 0; --i) {
          Inv v = (!mine.empty() && rng.below(3) == 0) ? mine[rng.below((int)mine.size())] : random_inv();
          if (!eligible(v)) v = random_inv();
          issue(v);
          mine.push_back(v);
        }
        sync_point(endkind, t0);
        check();
        if (cache && !failed && prev_kind >= 0)
          for (int hf = 0; hf < 3; ++hf)
            if (half[hf]) ++g_cov.pair[prev_kind][hf][queue];
        prev_async = true;
        prev_kind = endkind;
      }
      prev.swap(mine);
    }
    xsmm_hip_set_stream(nullptr);
    xsmm_hip_set_tile_queue(0);
    xsmm_hip_set_async(0);
    check();
    xsmm_hip_set_host_cache(0);
    check(); // ("switching it off writes everything back")
    for (Buf &b : buf) b.destroy();
  }
};

static void run_programs(int count, bool assert_coverage) {
  const Stats s0;
  for (int i = 0; i < count; ++i) {
    const uint64_t seed = 1000 + (uint64_t)i;
    Program off(seed, false), on(seed, true);
    off.run();
    on.run();
    EXPECT(off.failed || on.failed || off.digest == on.digest, "coherence program seed %llu: cache on != cache off", (unsigned long long)seed);
    if (g_fail > 8) break;
  }
  const Stats s1;
  const Coverage &c = g_cov;
  printf("coherence: %ld programs, %ld steps (%ld invokes, %ld host edits, %ld synchronisation points, %ld whole-memory checks)\n", c.programs, c.steps, c.invokes,
         c.edits, c.syncs, c.checks);
  printf("coverage (asynchronous segments behind each synchronisation kind; queue off / on):\n");
  for (int k = 0; k < N_SYNC; ++k) {
    static const char *half_name[3] = {"edit-then-invoke", "rewrite-an-output", "edit-an-output-a-beta-1-invoke-reads"};
    printf("  %-24s edit-then-invoke %3ld / %3ld   rewrite-an-output %3ld / %3ld   of them beta 1 (the edit is read) %3ld / %3ld\n", sync_name[k], c.pair[k][0][0],
           c.pair[k][0][1], c.pair[k][1][0], c.pair[k][1][1], c.pair[k][2][0], c.pair[k][2][1]);
    for (int hf = 0; hf < 3 && assert_coverage; ++hf)
      for (int q = 0; q < 2; ++q) EXPECT(c.pair[k][hf][q] > 0, "coverage: %s x %s x queue %d never occurred", sync_name[k], half_name[hf], q);
  }
  printf("  invoke kinds on host pointers, cache on:");
  for (int k = 0; k < N_KINDS; ++k) {
    printf(" %s %ld", kind_name[k], c.kinds[k]);
    if (assert_coverage) EXPECT(c.kinds[k] > 0, "coverage: invoke kind %s never ran", kind_name[k]);
  }
  printf("\n");
  EXPECT(s1.fast() - s0.fast() > 0, "no invoke was translated on the lock-free path");
  EXPECT(s1.skipped() - s0.skipped() == 0, "pages not written back: %ld", (long)(s1.skipped() - s0.skipped()));
  EXPECT(s1.written_back() - s0.written_back() > 0 && s1.uploaded() - s0.uploaded() > 0, "the cache moved no bytes");
  printf("  lock-free translations %ld, uploaded %ld B, written back %ld B, pages not written back %ld\n", (long)(s1.fast() - s0.fast()), (long)(s1.uploaded() - s0.uploaded()),
         (long)(s1.written_back() - s0.written_back()), (long)(s1.skipped() - s0.skipped()));
}
} // namespace coh

// ---- scenario 7: the size edges of the copy paths (copy_back / upload / the scratch output of complete(); Staging::SLOT = 4 MiB):
// one unary identity or relu per case, so the expected bytes need no arithmetic. The output mapping holds a sentinel that the host
// wrote: the gaps between rows and the guard bytes behind the last row must keep it.
namespace edges {
constexpr size_t SLOT = 4u << 20;
struct Case {
  const char *what;
  size_t rows, row_bytes, pitch; // of the OUTPUT (bytes); pitch == row_bytes: dense
  int op;                        // XSMM_UNARY_IDENTITY, or XSMM_UNARY_RELU in place (dense only)
  bool edit_input;               // a second invoke after the host edited the first, a middle and the last page of the input
};
static const Case cases[] = {
    // rows that fill most of their pitch (row_bytes * 4 >= pitch): whole pitches travel
    {"wide rows, pitch just below a slot", 3, SLOT - 256, SLOT - 64, XSMM_UNARY_IDENTITY, false},
    {"wide rows, pitch == slot", 3, SLOT - 128, SLOT, XSMM_UNARY_IDENTITY, false},
    {"wide rows, pitch just above a slot", 3, SLOT - 64, SLOT + 64, XSMM_UNARY_IDENTITY, false},
    {"wide rows, row and pitch above a slot", 3, SLOT + 64, SLOT + 256, XSMM_UNARY_IDENTITY, false},
    {"wide rows, pitch 5.2 MB (m 4, n 1 200 000, ldo 1 300 000 in f32)", 4, 4800000, 5200000, XSMM_UNARY_IDENTITY, false},
    {"one wide row behind a pitch above a slot", 1, 4800000, 5200000, XSMM_UNARY_IDENTITY, false},
    {"wide rows, one slot and a remainder in all", 17, 262144, 262208, XSMM_UNARY_IDENTITY, false},
    {"wide rows, two slots and a remainder in all", 33, 262144, 262208, XSMM_UNARY_IDENTITY, false},
    {"wide rows, three slots and a remainder in all", 49, 262144, 262208, XSMM_UNARY_IDENTITY, false},
    // narrow rows (row_bytes * 4 < pitch): the rows are gathered
    {"narrow rows, row just below a slot", 2, SLOT - 64, 4 * SLOT + 64, XSMM_UNARY_IDENTITY, false},
    {"narrow rows, row == slot", 2, SLOT, 4 * SLOT + 64, XSMM_UNARY_IDENTITY, false},
    {"narrow rows, row just above a slot", 2, SLOT + 64, 4 * SLOT + 512, XSMM_UNARY_IDENTITY, false},
    {"narrow rows, row 4.4 MB (m 3, n 1 100 000, ldo 4 600 000 in f32)", 3, 4400000, 18400000, XSMM_UNARY_IDENTITY, false},
    {"narrow rows, rows * row_bytes cross a slot", 17, 262144, 4 * 262144 + 64, XSMM_UNARY_IDENTITY, false},
    {"branch boundary: row_bytes * 4 == pitch (not narrow)", 1100, 4000, 16000, XSMM_UNARY_IDENTITY, false},
    {"branch boundary: row_bytes * 4 + 4 == pitch (narrow)", 1100, 4000, 16004, XSMM_UNARY_IDENTITY, false},
    // dense
    {"dense output of two slots and a half, start and end not page aligned", 1, 10 * 1048576 + 1000, 10 * 1048576 + 1000, XSMM_UNARY_IDENTITY, false},
    {"dense in-place relu of two slots and a half", 1, 10 * 1048576 + 1000, 10 * 1048576 + 1000, XSMM_UNARY_RELU, false},
    {"input of two slots and a half, first / middle / last page edited between invokes", 1, 10 * 1048576 + 1000, 10 * 1048576 + 1000, XSMM_UNARY_IDENTITY, true},
};
constexpr size_t OFF = 64 + 192, GUARD = 8192;
static char *map_bytes(size_t n) {
  char *m = (char *)mmap(nullptr, n, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
  if (m == MAP_FAILED) abort();
  return m;
}
template <typename T> static T value(size_t i);
template <> float value<float>(size_t i) { return (float)((long)(i % 1021) - 400); }
template <> uint16_t value<uint16_t>(size_t i) { return coh::bf16_of((float)((long)(i % 251) - 100)); }
template <typename T> static bool positive(T v);
template <> bool positive<float>(float v) { return v > 0.0f; }
template <> bool positive<uint16_t>(uint16_t v) { return !(v & 0x8000) && v != 0; }

static int g_ran = 0; // cases that actually ran
template <typename T> static void run_case(const Case &c, bool async) {
  const int64_t dt = sizeof(T) == 4 ? XSMM_DTYPE_F32 : XSMM_DTYPE_BF16;
  if (c.pitch % sizeof(T) || c.row_bytes % sizeof(T)) abort(); // (every listed size is a whole number of elements of both types)
  ++g_ran;
  const size_t n = c.row_bytes / sizeof(T), ld = c.pitch / sizeof(T), m = c.rows;
  printf("edge case [%s, %s] %s: m %zu n %zu ldo %zu\n", sizeof(T) == 4 ? "f32" : "bf16", async ? "asynchronous" : "synchronous", c.what, m, n, ld);
  fflush(stdout);
  xsmm_hip_set_host_cache(1);
  xsmm_hip_set_async(async ? 1 : 0);
  const bool inplace = c.op == XSMM_UNARY_RELU;
  const size_t in_elems = m * n, out_bytes = ((m - 1) * ld + n) * sizeof(T);
  const size_t xmap = (OFF + in_elems * sizeof(T) + GUARD + 4095) & ~(size_t)4095, omap = (OFF + out_bytes + GUARD + 4095) & ~(size_t)4095;
  char *xm = map_bytes(xmap), *om = inplace ? xm : map_bytes(omap);
  T *X = (T *)(xm + OFF), *O = (T *)(om + OFF);
  memset(xm, 0x5A, xmap);
  if (!inplace) memset(om, 0x5A, omap);
  for (size_t i = 0; i < in_elems; ++i) X[i] = value<T>(i);
  const int64_t h = xsmm_unary_dispatch(c.op, dt, (int64_t)m, (int64_t)n, (int64_t)n, (int64_t)ld, 0);
  const int passes = c.edit_input ? 2 : 1;
  for (int pass = 0; pass < passes; ++pass) {
    if (pass == 1) { // the host edits the first, one middle and the last page of the input (directly behind the synchronisation point)
      X[1] = value<T>(7777);
      X[in_elems / 2] = value<T>(8888);
      X[in_elems - 2] = value<T>(9999);
      memset(om, 0x5A, omap);
    }
    std::vector<T> want;
    if (inplace) {
      want.assign(X, X + in_elems);
      for (T &v : want)
        if (!positive<T>(v)) v = 0;
    }
    xsmm_unary_invoke(dt, h, X, 0, O, 0);
    if (async) xsmm_hip_synchronize();
    // every byte of the output mapping: rows = the input's, everything else the sentinel
    size_t bad = 0, first = 0;
    const unsigned char *ob = (const unsigned char *)om;
    const size_t omap_n = inplace ? xmap : omap;
    size_t at = 0;
    auto sentinel = [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi; ++i)
        if (ob[i] != 0x5A && !bad++) first = i;
    };
    sentinel(0, OFF);
    at = OFF;
    for (size_t r = 0; r < m; ++r) {
      const size_t lo = OFF + r * c.pitch;
      sentinel(at, lo);
      const T *src = inplace ? want.data() + r * n : X + r * n;
      if (memcmp(om + lo, src, c.row_bytes)) {
        for (size_t j = 0; j < n; ++j)
          if (memcmp(om + lo + j * sizeof(T), src + j, sizeof(T)) && !bad++) first = lo + j * sizeof(T);
      }
      at = lo + c.row_bytes;
    }
    sentinel(at, omap_n);
    EXPECT(bad == 0, "edge case [%s, %s] %s (pass %d): %zu wrong bytes / elements, the first at mapping byte %zu", sizeof(T) == 4 ? "f32" : "bf16",
           async ? "asynchronous" : "synchronous", c.what, pass, bad, first);
  }
  xsmm_hip_set_async(0);
  xsmm_hip_set_host_cache(0); // (forgets the mirrors: the mappings go away)
  munmap(xm, xmap);
  if (!inplace) munmap(om, omap);
}
static void run_all(int only) {
  int idx = 0;
  for (const Case &c : cases) {
    if (only < 0 || only == idx) {
      for (int async = 0; async < 2; ++async) {
        run_case<float>(c, async != 0);
        run_case<uint16_t>(c, async != 0);
      }
    }
    ++idx;
  }
  printf("copy-path edges: %d runs (%zu cases x synchronous / asynchronous x f32 / bf16)\n", g_ran, sizeof(cases) / sizeof(cases[0]));
}
} // namespace edges

static bool same(const std::vector<float> &a, const std::vector<float> &b) { return a.size() == b.size() && !memcmp(a.data(), b.data(), a.size() * 4); }

int main(int argc, char **argv) {
  // no argument: everything. "base": the hand-written scenarios; "coherence" [programs [nocoverage]]: the seeded programs (nocoverage:
  // a short run cannot reach every cell of the coverage table - everything else is still checked); "edges" [case]: the copy paths
  const std::string what = argc > 1 ? argv[1] : "all";
  const bool all = what == "all";
  const int prev = xsmm_hip_set_host_cache(1);
  if (prev < 0) {
    printf("SKIP: the kernel lacks userfaultfd WP_ASYNC / PAGEMAP_SCAN\n");
    return 77;
  }
  xsmm_hip_set_host_cache(0);
  if (all || what == "base") {
  {
    std::vector<float> off, on;
    int64_t u0, u1, v0, v1;
    scenario_sync(false, off, &u0, &u1);
    scenario_sync(true, on, &v0, &v1);
    EXPECT(same(off, on), "synchronous scenario: cache on != cache off (%zu values)", on.size());
    // (synchronous mode: the two edge pages of the output just written back - and a neighbour's page they are shared with - are not
    // trusted: other bytes of them may have been written meanwhile. Everything inside stays on the device.)
    EXPECT(v0 <= 4 * 4096, "steady state uploaded %ld bytes, expected at most the output's edge pages", (long)v0);
    EXPECT(v1 - v0 == 4096, "one edited element uploaded %ld bytes more than the steady state, expected one page", (long)(v1 - v0));
    printf("sync: identical to the plain mirror path (%zu values); steady-state upload %ld B, after a one-element edit %ld B\n", on.size(), (long)v0, (long)v1);
  }
  for (int threads : {1, 4}) {
    std::vector<float> off, on;
    int64_t a, b, c, x, y, z;
    scenario_async(false, threads, off, &a, &b, &c);
    scenario_async(true, threads, on, &x, &y, &z);
    EXPECT(same(off, on), "asynchronous scenario (%d threads): cache on != cache off", threads);
    // (an epoch starts with the edge pages of the runs written back at the synchronisation point - three outputs, two edges each - and
    // with whatever edge pages other heap objects were written in meanwhile; the buffers themselves are 112 pages)
    EXPECT(x <= 16 * 4096, "second epoch uploaded %ld bytes, expected at most a few edge pages", (long)x);
    EXPECT(y >= 2 * 4096 && y <= 24 * 4096, "two edited elements: %ld bytes uploaded (%ld without an edit)", (long)y, (long)x);
    EXPECT(z >= 5 * 3 * 16 - 3 * 16, "lock-free translations in the timed loop: %ld", (long)z);
    printf("async + tile queue, %d caller(s): identical; second-epoch upload %ld B; after two edits %ld B; %ld invokes translated lock-free\n", threads, (long)x, (long)y,
           (long)z);
  }
  {
    std::vector<float> off, on;
    int64_t a, b;
    scenario_lifetime(false, off, &a);
    scenario_lifetime(true, on, &b);
    EXPECT(same(off, on), "lifetime scenario: cache on != cache off");
    printf("lifetime: freed / re-mapped buffers never served from a stale mirror (%zu values identical)\n", on.size());
  }
  scenario_c2_async();
  printf("C2 loop, asynchronous: lock-free after the first invoke, nothing uploaded, equal to the device-pointer result\n");
  scenario_freed_before_sync();
  printf("freed before the synchronisation point: write-back skipped, no fault\n");
  }
  if (all || what == "coherence") coh::run_programs(argc > 2 ? atoi(argv[2]) : 60, !(argc > 3 && std::string(argv[3]) == "nocoverage"));
  if (all || what == "edges") edges::run_all(argc > 2 ? atoi(argv[2]) : -1);
  if (g_fail) {
    printf("%d FAILURE(S)\n", g_fail);
    return 1;
  }
  printf("OK\n");
  return 0;
}
