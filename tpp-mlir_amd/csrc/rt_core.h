// rt_core.h - error convention, configuration (environment switches), tracing
// One of the subsystem units of runtime.cpp (round 6, VERDICT r5 next 7: the 3 000-line file split by subsystem, no behaviour
// change). The units are INCLUDED into the one translation unit runtime.cpp, in dependence order, inside its anonymous namespace:
// the per-invoke host path (14-18 ns: enqueue_item -> join_window -> Segment::mark) crosses four of them and is inlined across
// their borders - as separate objects without LTO it would pay a call per border. Not a stand-alone header: include runtime.cpp's way only.


[[noreturn]] void die(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
  fflush(stderr);
  exit(-1); // XsmmRunnerUtils.cpp:132-137 convention
}

#define HIP_OK(expr)                                                                               \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) die("tpp-xsmm-hip: %s failed: %s (no CPU fallback exists)", #expr, hipGetErrorString(e_)); \
  } while (0)

inline void cpu_relax() {
#if defined(__x86_64__)
  __builtin_ia32_pause();
#else
  asm volatile("" ::: "memory");
#endif
}

struct Config {
  std::atomic<int> async{0};
  std::atomic<hipStream_t> stream{nullptr};
  std::atomic<int> forced_variant{-1};
  std::atomic<int> tile_queue{0};
  std::atomic<int> f32_precision{0}; // f32 arithmetic of descriptors dispatched from now on: 0 = exact, 6 = bf16x6 (xsmm_hip_set_f32_precision / TPP_HIP_F32_PRECISION)
  std::atomic<int> vnni_factor{2}; // blocking factor of VNNI B operands dispatched from now on (xsmm_hip_set_vnni_factor / TPP_HIP_VNNI_FACTOR)
  int trace = 0; // TPP_HIP_TRACE: 1 = one stderr line per dispatch + a roctx range per invoke, 2 = also one stderr line per invoke
  // TPP_HIP_FOLD_TRANSPOSE / xsmm_hip_set_fold_transpose: 0 = off, 1 = transposes that feed a gemm's B operand are folded into it, 2 (opt-in) =
  // also those that feed its A operand, and the folded gemms may read the source with 16-byte loads (rt_rewrites.h)
  std::atomic<int> fold_transpose{1};
  std::atomic<int> fold_epilogue{1};  // TPP_HIP_FOLD_EPILOGUE / xsmm_hip_set_fold_epilogue: element-wise invokes on a queued GEMM tile join its group (rt_tile_queue.h)
  std::atomic<int> relayout_grid{1};  // TPP_HIP_RELAYOUT_GRID / xsmm_hip_set_relayout_grid: replayed pack / unpack groups run as relayout grids (rt_relayout.h)
  // TPP_HIP_STRICT / xsmm_hip_set_strict (round 6): the kernel an invoke runs on is a function of its descriptor,
  // batch count and own pointer alignment only - no grid merge, no folded transposes, no kernel family chosen by the size of the
  // queued group, groups of one alignment class and one batch count only. The same invoke on the same data then returns the same
  // bits whether it runs alone, in the first pass of a queued group or in a replay (libxsmm's JIT'd kernel is a function of the
  // dispatch tuple: XsmmRunnerUtils.cpp:288-306).
  std::atomic<int> strict{0};
  Config() {
    if (const char *e = getenv("TPP_HIP_STRICT")) {
      strict = atoi(e) != 0;
      tpp::set_strict_kernels(strict.load());
    }
    if (const char *e = getenv("TPP_HIP_FOLD_TRANSPOSE")) {
      if (atoi(e) >= 0 && atoi(e) <= 2) fold_transpose = atoi(e);
      else fprintf(stderr, "[tpp-xsmm-hip] TPP_HIP_FOLD_TRANSPOSE=%s ignored: the mode is 0, 1 or 2\n", e);
    }
    if (const char *e = getenv("TPP_HIP_RELAYOUT_GRID")) relayout_grid = atoi(e) != 0;
    if (const char *e = getenv("TPP_HIP_FOLD_EPILOGUE")) fold_epilogue = atoi(e) != 0;
    if (const char *e = getenv("TPP_HIP_ASYNC")) async = atoi(e) != 0;
    if (const char *e = getenv("TPP_HIP_TRACE")) trace = atoi(e);
    if (const char *e = getenv("TPP_HIP_VARIANT")) forced_variant = atoi(e);
    if (const char *e = getenv("TPP_HIP_TILE_QUEUE")) tile_queue = atoi(e) < 0 ? 0 : atoi(e) > 2 ? 2 : atoi(e);
    if (const char *e = getenv("TPP_HIP_VNNI_FACTOR")) {
      if (atoi(e) == 2 || atoi(e) == 4) vnni_factor = atoi(e);
      else fprintf(stderr, "[tpp-xsmm-hip] TPP_HIP_VNNI_FACTOR=%s ignored: the factor is 2 or 4\n", e);
    }
    if (const char *e = getenv("TPP_HIP_F32_PRECISION")) {
      if (!strcmp(e, "bf16x6") || !strcmp(e, "6")) f32_precision = 6;
      if (trace)
        fprintf(stderr, "[tpp-xsmm-hip] TPP_HIP_F32_PRECISION=%s: f32 gemm arithmetic %s\n", e,
                f32_precision.load() == 6 ? "bf16x6 (split into three bf16 parts, six bf16 MFMA products)" : "exact f32 (the value is not bf16x6 / 6)");
    }
  }
};
Config &cfg() {
  static Config c;
  return c;
}
// what the layer-chain launch decision reads besides the calls and the stream's compute units (gemm_plan.h plan_chain): filled per invoke
inline tpp::ChainPlanEnv chain_plan_env() { return tpp::chain_plan_env_of(cfg().strict.load(std::memory_order_relaxed) != 0); }
// the stream an invoke of THIS thread launches on: the process-wide setting, unless the thread is re-running a journaled chain
// launch on that launch's stream (check_chain_errors; ADVICE r5: the re-run must not change the setting other threads read)
// (in the static TLS block - initial-exec: a %fs-relative load; the general-dynamic model of a shared library calls __tls_get_addr per
// access, twice per gemm invoke here. 16 bytes of the loader's static-TLS reserve; -DTPP_TLS_DEFAULT_MODEL: see rt_enqueue.h tl_fast)
struct TlHot {
  hipStream_t stream_override;
  bool has_stream_override;
};
#ifdef TPP_TLS_DEFAULT_MODEL
static __thread TlHot tl_hot = {nullptr, false};
#else
static __thread TlHot tl_hot __attribute__((tls_model("initial-exec"))) = {nullptr, false};
#endif
inline hipStream_t invoke_stream() { return tl_hot.has_stream_override ? tl_hot.stream_override : cfg().stream.load(std::memory_order_relaxed); }
// membarrier(PRIVATE_EXPEDITED) is registered and usable (the asymmetric fences of the direct window, the scheduler's parking and the
// deferred transposes' owner sections); TPP_HIP_NO_MEMBARRIER: never (the two-sided protocols everywhere)
inline bool membarrier_ok() {
  static const bool ok = !getenv("TPP_HIP_NO_MEMBARRIER") && syscall(__NR_membarrier, MEMBARRIER_CMD_REGISTER_PRIVATE_EXPEDITED, 0) == 0;
  return ok;
}

// ---- tracing: with TPP_HIP_TRACE >= 1 every invoke runs inside a roctx range named after its
// dispatch tuple and kernel, so `rocprofv3 --marker-trace --kernel-trace` timelines show which xsmm call a kernel
// belongs to. libroctx64 is looked up at run time (profiling tool, not a link dependency of the product).
struct Roctx {
  int (*push)(const char *) = nullptr;
  int (*pop)() = nullptr;
  Roctx() {
    if (cfg().trace < 1) return;
    // rocprofv3 (rocprofiler-sdk) traces the SDK's roctx library; the classic libroctx64 serves older tools
    void *h = nullptr;
    for (const char *name : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "/opt/rocm/lib/librocprofiler-sdk-roctx.so",
                             "libroctx64.so", "libroctx64.so.4", "/opt/rocm/lib/libroctx64.so"})
      if ((h = dlopen(name, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!h) return;
    push = (int (*)(const char *))dlsym(h, "roctxRangePushA");
    pop = (int (*)())dlsym(h, "roctxRangePop");
    if (!push || !pop) push = nullptr, pop = nullptr;
  }
};
Roctx &roctx() {
  static Roctx r;
  return r;
}
struct TraceRange {
  bool on = false;
  __attribute__((always_inline)) TraceRange(const char *who, const char *what) {
    if (__builtin_expect(cfg().trace < 1, 1)) return; // (inline: one load per invoke when tracing is off)
    begin(who, what);
  }
  __attribute__((noinline)) void begin(const char *who, const char *what) {
    if (cfg().trace >= 2) fprintf(stderr, "[tpp-xsmm-hip] %s %s\n", who, what);
    if (roctx().push) on = roctx().push(what) >= 0;
  }
  ~TraceRange() {
    if (on) roctx().pop();
  }
};
