/*
 * tpp_xsmm_abi.h - the dispatch/invoke C-ABI of tpp-mlir's runtime/Xsmm,
 * re-declared for the MI355X-native runtime (libtpp_xsmm_runner_utils.so).
 *
 * Every entry point below replaces the symbol of the same name exported by the
 * reference's libtpp_xsmm_runner_utils.so. Reference declarations:
 *   runtime/Xsmm/XsmmRunnerUtils.h:22-83   (13 xsmm_* symbols)
 *   runtime/PerfRunnerUtils.h:22-24        (perf_start_timer / perf_stop_timer)
 * The reference header types the enum arguments as libxsmm enums; the compiler
 * always materialises them as i64 constants (lib/TPP/Conversion/ConvertXsmmToFunc/
 * ConvertXsmmToFunc.cpp:63-65, 319-340), and libxsmm is not a dependency of this
 * runtime, so they are int64_t here. On x86-64 SysV the two declarations are
 * call-compatible for the value range the compiler emits (non-negative, < 2^31).
 *
 * All matrices are row-major. `off*` are element offsets (memref offsets), added
 * as typed pointer arithmetic (XsmmRunnerUtils.cpp:63-75).
 *
 * Data pointers may be device pointers (used in place, zero copy) or host
 * pointers (staged through a device mirror; results are copied back before the
 * invoke returns, preserving the reference's synchronous completion contract).
 */
#ifndef TPP_XSMM_ABI_H
#define TPP_XSMM_ABI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TPP_XSMM_EXPORT __attribute__((visibility("default")))

/* ---- wire values: include/TPP/Dialect/Xsmm/XsmmEnum.td:13-84 ---------------- */
enum { XSMM_DTYPE_F32 = 1, XSMM_DTYPE_BF16 = 2 };                          /* :13-20 */
enum {                                                                     /* :34-45 */
  XSMM_UNARY_NONE = 0, XSMM_UNARY_IDENTITY = 1, XSMM_UNARY_ZERO = 2,
  XSMM_UNARY_RELU = 5, XSMM_UNARY_VNNI2 = 28, XSMM_UNARY_TRANSPOSE = 29
};
enum {                                                                     /* :47-56 */
  XSMM_UNARY_FLAG_NONE = 0, XSMM_UNARY_FLAG_BCAST_ROW = 2,
  XSMM_UNARY_FLAG_BCAST_COL = 4, XSMM_UNARY_FLAG_BCAST_SCALAR = 8
};
enum {                                                                     /* :22-32 */
  XSMM_BINARY_NONE = 0, XSMM_BINARY_ADD = 1, XSMM_BINARY_MUL = 2,
  XSMM_BINARY_SUB = 3, XSMM_BINARY_DIV = 4
};
enum {                                                                     /* :58-70 */
  XSMM_BINARY_FLAG_NONE = 0,
  XSMM_BINARY_FLAG_BCAST_ROW_IN_0 = 1, XSMM_BINARY_FLAG_BCAST_ROW_IN_1 = 2,
  XSMM_BINARY_FLAG_BCAST_COL_IN_0 = 4, XSMM_BINARY_FLAG_BCAST_COL_IN_1 = 8,
  XSMM_BINARY_FLAG_BCAST_SCALAR_IN_0 = 16, XSMM_BINARY_FLAG_BCAST_SCALAR_IN_1 = 32
};
/* GEMM flags AS THEY ARRIVE ON THE WIRE. The dialect values are VNNI_A=2048,
 * VNNI_B=4096 (XsmmEnum.td:72-84) but ConvertXsmmToFunc.cpp:251-265 exchanges the
 * two because the runtime swaps A and B for libxsmm's column-major view: a
 * dialect `vnni_b` operand arrives as 2048, `vnni_a` as 4096. */
enum {
  XSMM_GEMM_FLAG_NONE = 0, XSMM_GEMM_FLAG_BETA_0 = 4,
  XSMM_GEMM_FLAG_NO_RESET_TILECONFIG = 64, XSMM_GEMM_FLAG_NO_SETUP_TILECONFIG = 128,
  XSMM_GEMM_WIRE_VNNI_B = 2048, /* row-major B operand is [K/2][N][2] */
  XSMM_GEMM_WIRE_VNNI_A = 4096, /* row-major A operand is [M][K/2][2] = plain row-major bytes (VNNIUtils.cpp:75-77) */
  XSMM_GEMM_FLAG_VNNI_C = 8192  /* C stored / read as VNNI-2 [M/2][N][2], ldc = pair-row stride / 2 (generic kernel) */
};

/* ---- dispatch: build (or look up) a kernel descriptor, return opaque handle ----
 * Handles are never freed (the reference has no destroy call); dispatching the
 * same arguments again returns the same handle. Unsupported arguments: message
 * on stderr + exit(-1), as XsmmRunnerUtils.cpp:132-137,170-176,202-208,352-358. */

/* replaces XsmmRunnerUtils.cpp:95-140 */
TPP_XSMM_EXPORT int64_t xsmm_gemm_dispatch(int64_t dtype, int64_t m, int64_t n, int64_t k,
                                           int64_t lda, int64_t ldb, int64_t ldc,
                                           int64_t flags);
/* replaces XsmmRunnerUtils.cpp:308-361 */
TPP_XSMM_EXPORT int64_t xsmm_brgemm_dispatch(int64_t dtype, int64_t m, int64_t n, int64_t k,
                                             int64_t lda, int64_t ldb, int64_t ldc,
                                             int64_t stride_a, int64_t stride_b,
                                             int64_t flags);
/* replaces XsmmRunnerUtils.cpp:385-457 */
TPP_XSMM_EXPORT int64_t xsmm_fused_brgemm_dispatch(int64_t dtype, int64_t m, int64_t n,
                                                   int64_t k, int64_t lda, int64_t ldb,
                                                   int64_t ldc, int64_t stride_a,
                                                   int64_t stride_b, int64_t gemm_flags,
                                                   int64_t unary_flags, int64_t unary_kind,
                                                   int64_t binary_flags, int64_t binary_kind);
/* replaces XsmmRunnerUtils.cpp:142-179 */
TPP_XSMM_EXPORT int64_t xsmm_unary_dispatch(int64_t unary_kind, int64_t dtype, int64_t m,
                                            int64_t n, int64_t ldi, int64_t ldo,
                                            int64_t flags);
/* replaces XsmmRunnerUtils.cpp:181-211 */
TPP_XSMM_EXPORT int64_t xsmm_binary_dispatch(int64_t binary_kind, int64_t dtype, int64_t m,
                                             int64_t n, int64_t ldi_lhs, int64_t ldi_rhs,
                                             int64_t ldo, int64_t flags);
/* replaces XsmmRunnerUtils.cpp:213-246 (Intel AMX only: a no-op here) */
TPP_XSMM_EXPORT int64_t xsmm_intel_amx_tile_config_dispatch(int64_t dtype, int64_t m,
                                                            int64_t n, int64_t k,
                                                            int64_t lda, int64_t ldb,
                                                            int64_t ldc, int64_t stride_a,
                                                            int64_t stride_b, int64_t flags);

/* ---- invoke: run a dispatched kernel; synchronous unless async mode is on ---- */

/* replaces XsmmRunnerUtils.cpp:79-93 */
TPP_XSMM_EXPORT void xsmm_gemm_invoke(int64_t dtype, int64_t handle, void *a, int64_t off_a,
                                      void *b, int64_t off_b, void *c, int64_t off_c);
/* replaces XsmmRunnerUtils.cpp:288-306 */
TPP_XSMM_EXPORT void xsmm_brgemm_invoke(int64_t dtype, int64_t handle, void *a,
                                        int64_t off_a, void *b, int64_t off_b, void *c,
                                        int64_t off_c, int64_t num_batches);
/* replaces XsmmRunnerUtils.cpp:363-383 */
TPP_XSMM_EXPORT void xsmm_fused_brgemm_invoke(int64_t dtype, int64_t handle, void *a,
                                              int64_t off_a, void *b, int64_t off_b, void *c,
                                              int64_t off_c, void *d, int64_t off_d,
                                              int64_t num_batches);
/* replaces XsmmRunnerUtils.cpp:248-259 */
TPP_XSMM_EXPORT void xsmm_unary_invoke(int64_t dtype, int64_t handle, void *in,
                                       int64_t off_in, void *out, int64_t off_out);
/* replaces XsmmRunnerUtils.cpp:276-286 (the scalar is ALWAYS an f32) */
TPP_XSMM_EXPORT void xsmm_unary_scalar_invoke(int64_t dtype, int64_t handle, float scalar,
                                              void *out, int64_t off_out);
/* replaces XsmmRunnerUtils.cpp:261-274 */
TPP_XSMM_EXPORT void xsmm_binary_invoke(int64_t dtype, int64_t handle, void *lhs,
                                        int64_t off_lhs, void *rhs, int64_t off_rhs,
                                        void *out, int64_t off_out);
/* replaces XsmmRunnerUtils.cpp:459-469 (no-op) */
TPP_XSMM_EXPORT void xsmm_intel_amx_tile_config_invoke(int64_t dtype, int64_t handle,
                                                       void *tile_state, int64_t off);

/* ---- timers: runtime/PerfRunnerUtils.cpp:23-35. perf_stop_timer drains the
 * device queue before reading the clock so that async-mode launches are counted. */
TPP_XSMM_EXPORT int64_t perf_start_timer(void);
TPP_XSMM_EXPORT double perf_stop_timer(int64_t start);

/* ---- extensions (NOT in the reference; the reference ABI has no config call) --
 * The JIT'd code never calls these; harnesses (bench.py, tests, tpp_replay) do. */

/* 0 (default): every invoke returns after its kernel completed (reference
 * semantics). 1: invokes only enqueue on the runtime's stream; call
 * xsmm_hip_synchronize() or perf_stop_timer() to drain. Returns previous mode.
 * Also settable with env TPP_HIP_ASYNC=1.
 * BUFFER LIFETIME in async mode: operands may be freed / re-allocated only after
 * xsmm_hip_synchronize(), perf_stop_timer() or xsmm_hip_set_async(0) returned -
 * those calls launch whatever the tile queue still holds, drain the stream and
 * forget the device allocation ranges the runtime has cached since the last such
 * call. Synchronising the device some other way (hipDeviceSynchronize,
 * torch.cuda.synchronize) leaves queued invokes unlaunched and the cache in place. */
TPP_XSMM_EXPORT int xsmm_hip_set_async(int enable);
/* Tile queue (async mode only, device pointers only): invokes of ONE small-tile handle - GEMM
 * family, unary or binary, m, n <= 64: the compiler's native 32x32x32 call pattern and its per-block
 * pack / unpack tiles - are collected and run as ONE grouped launch at the next flush point (other
 * handle / other op / data dependence on a queued output or overwrite of a queued input /
 * xsmm_hip_flush / xsmm_hip_synchronize / perf_stop_timer). Program order is preserved. Operands
 * of queued invokes must stay valid until the flush. Returns the previous setting. Also env
 * TPP_HIP_TILE_QUEUE=1. The queue serves ONE device per process (the device current on the first
 * queued invoke): a queued invoke from a thread whose current device differs is a fatal error.
 * Several calling threads (the reference's OpenMP team over a layer's tile grid): a group that was collected once is
 * REPLAYED when its invokes come again - each caller marks its own invokes in the recorded group without taking a lock, and
 * the complete group launches from a work list that already sits in device memory. Programs that do not repeat themselves
 * are handed to a scheduler thread after a few thousand locked arrivals; enable = 2 (TPP_HIP_TILE_QUEUE=2) does that as soon
 * as a second thread shows up (the round-2 behaviour, kept for comparison runs).
 * On a stream that is being captured into a graph a group is legal: it always gathers its members into a pinned work list of its
 * own, which the runtime never writes or frees again - every replay of the graph reads it - (160 KiB per captured flush, for the
 * life of the process), records no event, and a group planned on a split kernel runs and reports the unsplit one. The capture
 * must be in RELAXED mode (hipStreamCaptureModeRelaxed; torch: capture_error_mode="relaxed"): the ring allocates the pinned buffer
 * of a slot inside the capture - at a slot's first use, and after every captured flush - and under the global or thread-local
 * mode that allocation is an error, which ends the process like every other HIP error. */
TPP_XSMM_EXPORT int xsmm_hip_set_tile_queue(int enable);
TPP_XSMM_EXPORT void xsmm_hip_flush(void);
/* n fused_brgemm invokes in ONE call (arrays of length n, one entry per call): exactly the effect of
 *   for (i = 0; i < n; ++i) xsmm_fused_brgemm_invoke(dtype, handles[i], a[i], off_a[i], b[i], off_b[i], c[i], off_c[i],
 *                                                    d[i], off_d[i], num_batches[i]);
 * (XsmmRunnerUtils.cpp:363-457 per call). This is how a harness hands over a rank's MLP step (mlir-gen's layer chain,
 * MLIRGen.cpp:632-681: every layer one whole-layer fused_brgemm): when the calls form a CHAIN - call i+1 reads call i's
 * output as its A operand (same pointer, lda = ldc), bf16 with ONE kind of B operand (VNNI-2, flat or VNNI-4), beta 0, equal m and n, device pointers,
 * asynchronous mode, the outputs overlap no other operand, and one of the 32x64 .. 128x128 tiles covers m x n with at most
 * one workgroup per compute unit - the whole chain runs as ONE persistent kernel (rows of layer i+1 start as soon as the
 * same rows of layer i are stored: no kernel boundary, the next layer's weight panels are prefetched under the epilogue).
 * Same arithmetic as the separate launches (f32 accumulation in k order, one rounding per layer); bit-identical to them when
 * they run on the same tile, which is the case whenever dispatch planned the layers with a loader-wave tile (variants 20 .. 23)
 * that fits the chip. Returns 1 if the chain ran as one launch, 0 if it ran call by call.
 * f32 (round 4): chains of whole-layer f32 calls (no VNNI operand, beta 0, 16-byte aligned operands and bias) run as one launch when
 * EVERY call was planned on the same 64-row K-split loader-wave tile (64x64 + K2 or 64x32 + K4: 512 .. 1024 rows of a 1024-wide
 * layer) and that tile fits the chip - bit-identical to the calls, 1-2.5 % faster; 32-row tiles (256 rows) stay call by call, which
 * measured faster there (profiles/r04_f32_chain.txt).
 * Call i > 0 must keep every batch element inside its predecessor's rows ((br - 1) * stride_a + k <= lda): the hand-off is per row
 * block; a row-striding later call runs call by call.
 * RESIDENCY: the single launch needs every workgroup of its grid on a compute unit at the same time (one per CU). The grid is
 * checked against the CUs the stream may use (a CU mask is honoured); what cannot be checked is another process - or another
 * stream's LDS-heavy kernel - occupying CUs at that moment: the single-launch path needs the device to itself. Every wait inside
 * the kernel is bounded (50 ms): a starved launch never hangs, and since round 5 it does not end the process either - the library
 * DEGRADES (the reference never aborts on a valid invoke): the FIRST single launch of every (stream, tile grid, layer count) is
 * followed by a stream synchronisation and a look at its error word - a device that is shared from the start is found out before
 * anyone could consume the launch's outputs, the call runs call by call at once (return value 0; the inputs are intact: beta 0,
 * the outputs overlap no operand); later launches stay asynchronous and their calls are journaled - if the check at the next
 * xsmm_hip_synchronize / perf_stop_timer finds a starved launch, the journaled calls are re-run call by call, in launch order,
 * before that call returns. Either way one line goes to stderr and every later chain invoke of the process runs call by call.
 * (What the re-run cannot repair: work that OTHERS enqueued between a starved asynchronous launch and the synchronisation has read
 * invalid outputs.) A harness that knows it shares the GPU sets TPP_HIP_CHAIN=0 and spares itself the timeouts.
 * TPP_HIP_CHAIN=0 disables the single-launch path. */
TPP_XSMM_EXPORT int xsmm_hip_fused_brgemm_chain_invoke(int64_t dtype, int64_t n, const int64_t *handles, void *const *a,
                                                       const int64_t *off_a, void *const *b, const int64_t *off_b,
                                                       void *const *c, const int64_t *off_c, void *const *d,
                                                       const int64_t *off_d, const int64_t *num_batches);
/* STRICT mode (env TPP_HIP_STRICT=1): the kernel an invoke runs on - and with it the order of its floating-point additions - is a
 * function of its descriptor, its batch count and the alignment of its OWN pointers only (libxsmm's JIT'd kernel is a function of
 * the dispatch tuple: XsmmRunnerUtils.cpp:288-306). Off (default), the tile queue lets the GROUP choose: tile grids over flat operands
 * are merged into one launch, transposes are folded into the gemm they feed, the kernel family and the split follow the size of the
 * queued group - all within the 1e-5 bar, but the same invoke on the same data may return different last bits alone, in the first
 * pass of a loop and in its replays. On: no grid merge, no folded transposes, every size-dependent choice is taken as for a group of
 * one, a group holds invokes of one alignment class and one batch count only, single invokes of queue-sized tiles run on the kernel
 * their group runs on, and a chain call runs as one launch only on the tile its layers were planned on. Relayout grids
 * (xsmm_hip_set_relayout_grid) stay ON in strict mode: they copy raw words, and a copy's bits do not depend on the kernel. DETERMINISM: run to run
 * always (no floating-point atomics anywhere); call to call - alone / first queued pass / replay - under strict mode
 * (tests/test_strict_gpu.py). Choose the mode before the first queued invoke: returns the previous setting, -1 if the tile queue has
 * already recorded groups under the other one. */
TPP_XSMM_EXPORT int xsmm_hip_set_strict(int enable);
TPP_XSMM_EXPORT int xsmm_hip_get_strict(void);
/* The launch thread (round 6; TPP_HIP_LAUNCH_THREAD=0|1, default 1; tile queue + asynchronous mode only). A recorded group that is
 * replayed completely is launched by a helper thread of the runtime instead of the calling thread: the caller goes on queueing the
 * next group while hipLaunchKernel (2.3-2.6 us of host time) runs beside it. Stream order is unchanged - the hand-overs leave in
 * order, and everything else that launches / copies / synchronises first waits until they have left. The thread spins while
 * launches keep coming, sleeps after ~0.2 ms without one and ends after ~2 s. Kernel choice and results do not depend on the setting.
 * xsmm_hip_set_launch_thread returns the previous setting; stats: out[0] = launches handed over since process start, out[1] = 1 if
 * the thread exists right now. */
TPP_XSMM_EXPORT int xsmm_hip_set_launch_thread(int enable);
TPP_XSMM_EXPORT void xsmm_hip_launch_thread_stats(int64_t out[2]);
/* Sticky status of the chain launches: the number of journaled launches that were found starved at a synchronisation point and
 * re-run call by call since process start (0: never). Round 6: every journaled launch has its own error word, so only the starved
 * launch and the later ones of ITS stream are re-run (healthy earlier launches are left alone), the journal is kept per stream, and
 * a launching thread that finds the pool of error words nearly used up synchronises and checks instead of dropping an entry.
 * TPP_HIP_CHAIN_STRICT=1: a starved launch ends the process (stderr + exit(-1)) instead of being repaired. */
TPP_XSMM_EXPORT int64_t xsmm_hip_chain_status(void);
/* Peer-store all-gather (one process per GPU, no collective library call): every rank stores its row block straight into
 * every peer's output buffer through IPC-mapped pointers, completion by flags (csrc/peer_gather.hip; host-side protocol:
 * tpp-mlir_amd/peer.py). _peer_alloc returns a dedicated zeroed device allocation (IPC handles name whole allocations);
 * _ipc_export writes its 64-byte handle; _ipc_open maps a peer's handle (nullptr on failure); _peer_gather enqueues one step on
 * the runtime's stream: scatter of `bytes` from src to dst[w] + dst_offset for every w < world, then a wait until every peer's
 * block has landed in THIS rank's buffer. dst / flags / ready: `world` pointers each; epoch: 1, 2, 3, ... (the same on every rank). */
TPP_XSMM_EXPORT void *xsmm_hip_peer_alloc(int64_t bytes);
TPP_XSMM_EXPORT void xsmm_hip_peer_free(void *ptr);
TPP_XSMM_EXPORT int xsmm_hip_ipc_export(void *ptr, void *handle_out_64_bytes);
TPP_XSMM_EXPORT void *xsmm_hip_ipc_open(const void *handle_64_bytes);
TPP_XSMM_EXPORT int xsmm_hip_ipc_close(void *ptr);
TPP_XSMM_EXPORT void xsmm_hip_peer_gather(const void *src, int64_t bytes, int64_t dst_offset, int64_t world, int64_t rank,
                                          void *const *dst, void *const *flags, void *const *ready, void *my_flags, void *my_ready,
                                          void *ticket, void *err, int64_t epoch);
/* OVERLAP mode of the peer gather (0 / 1, returns the previous setting): the wait kernel goes to a side stream, so the transfer
 * time of a step's blocks no longer sits between this step's kernels and the next step's on the runtime's stream. The gathered
 * output of a step is then complete when the SIDE stream has passed that step's wait kernel: xsmm_hip_peer_drain() blocks the
 * host until it has; xsmm_hip_peer_wait_stream() returns the stream (hipStream_t) for an event-based dependence. A consumer of
 * the output of step e must run before this rank enqueues the gather of step e+1 on the runtime's stream (the peers take "rank r
 * has entered gather e+1" as the licence to overwrite the buffer of step e at step e+2, exactly as without the overlap). */
TPP_XSMM_EXPORT int xsmm_hip_peer_overlap(int enable);
TPP_XSMM_EXPORT void *xsmm_hip_peer_wait_stream(void);
TPP_XSMM_EXPORT void xsmm_hip_peer_drain(void);
/* counters of the tile queue since process start: out[0] grouped launches, out[1] invokes queued with the full
 * dependence bookkeeping, out[2] invokes queued by replay of a recorded group (trace cache), out[3] groups ended by
 * a remembered terminator, out[4] replays abandoned (the caller left the recorded group) */
TPP_XSMM_EXPORT void xsmm_hip_tile_queue_stats(int64_t out[5]);
/* Stream the kernels are launched on (a hipStream_t). NULL = default stream. */
TPP_XSMM_EXPORT void xsmm_hip_set_stream(void *hip_stream);
TPP_XSMM_EXPORT void *xsmm_hip_get_stream(void);
TPP_XSMM_EXPORT void xsmm_hip_synchronize(void);
/* Host residents: the ABI has no allocation hook, so the runtime never caches a mirror of a host buffer
 * behind the caller's back. A harness that knows a host buffer is long-lived (weights, the operands of a
 * timing loop: lib/TPP/Runner/MLIRBench.cpp:207-246 allocates them once) can declare it: the buffer is
 * uploaded once, and invokes whose operands lie inside it run on the device copy without any upload
 * (operands the kernel writes are still copied back, so the host view stays current). _update re-uploads
 * after the host changed the buffer; _release drops the copy. Return 0, or -1 (unknown / overlapping range). */
TPP_XSMM_EXPORT int xsmm_hip_host_resident(const void *ptr, int64_t bytes);
TPP_XSMM_EXPORT int xsmm_hip_host_update(const void *ptr);
TPP_XSMM_EXPORT int xsmm_hip_host_release(const void *ptr);
/* Host cache (round 6; csrc/host_cache.h): the AUTOMATIC form of the host residents - for an unmodified harness that hands host
 * pointers to every invoke (memref globals / malloc: lib/TPP/Runner/MLIRBench.cpp:207-246) and can be given environment variables only.
 * enable = 1 (env TPP_HIP_HOST_CACHE=1): a host operand gets a device mirror that OUTLIVES the invoke; before a kernel uses mirror
 * pages, the pages the host has written since the runtime last looked are uploaded again - and only those (the kernel's own write
 * tracking says which: userfaultfd asynchronous write-protect + PAGEMAP_SCAN, Linux >= 6.7; no fault handler, no signal, no helper
 * thread; system calls that write into tracked memory work as always). What kernels write goes back to exactly the host bytes they
 * wrote: in synchronous mode before the invoke returns - the reference's contract (SURVEY.md 8b "Completion"), unchanged -, in
 * asynchronous mode at the next synchronisation point (xsmm_hip_synchronize / perf_stop_timer / xsmm_hip_set_async(0) /
 * xsmm_hip_set_stream). ASYNCHRONOUS MODE CONTRACT with host operands: the lifetime rule above, and between two synchronisation
 * points the host neither reads outputs nor writes operands of the invokes in between (the runtime looks at an extent once per
 * synchronisation epoch; the tile queue then sees device pointers, so TPP_HIP_ASYNC=1 TPP_HIP_TILE_QUEUE=1 TPP_HIP_HOST_CACHE=1 runs
 * the compiler's tile invokes on host buffers as grouped launches). xsmm_hip_set_stream counts as a synchronisation point when it
 * changes the stream in asynchronous mode: the stream being left is drained, its outputs reach the host, a new epoch starts.
 * THREADS: with the host cache on, a synchronisation point (any of the four, and xsmm_hip_set_host_cache(0)) must not run while
 * ANOTHER thread is inside an invoke on host operands, or between that thread's invokes of one asynchronous region: the write-back
 * protects partly covered pages again and marks them for upload, and the other thread's next invoke would upload host bytes over
 * mirror bytes its own kernel wrote and that have not been written back yet. Join (or barrier) the calling threads first - the
 * reference's harness synchronises from its single main thread behind the OpenMP region.
 * A range that was unmapped and mapped again, or cannot be tracked (file-backed / shared mappings), falls back to the plain per-invoke mirror. Returns the previous setting, or -1 if the kernel
 * interface is missing (the cache stays off). Switching it off writes everything back and frees the mirrors.
 * _stats: out[0] extents, [1] mirror bytes, [2] bytes uploaded, [3] page-table scans, [4] bytes written back, [5] pages NOT written back
 * (their range changed hands or the host wrote them while a device write was pending), [6] extents created / grown / merged,
 * [7] invokes translated on the lock-free path, [8] on the locked path, [9] extents given up. */
TPP_XSMM_EXPORT int xsmm_hip_set_host_cache(int enable);
TPP_XSMM_EXPORT void xsmm_hip_host_cache_stats(int64_t out[10]);
/* Number of visible HIP devices (0 on a CPU-only host; never exits). */
TPP_XSMM_EXPORT int xsmm_hip_device_count(void);
/* Name of the HIP kernel variant a GEMM-like handle selected, for profiles. */
TPP_XSMM_EXPORT const char *xsmm_hip_kernel_name(int64_t handle);
/* Name of the kernel family the tile queue's most recent grouped GEMM launch ran on ("" before the first): a group of queued tile
 * invokes may run on a faster family than a single invoke of its handle would (xsmm_hip_kernel_name), e.g. 32-k f32 tiles with even
 * batch counts on the loader-wave kernels. A static string; diagnostics only. */
TPP_XSMM_EXPORT const char *xsmm_hip_last_grouped_kernel(void);
/* The kernel of the most recent NON-queued gemm / brgemm / fused_brgemm invoke when it was refined at invoke time - the batch count
 * arrives with the invoke, so two choices are made there: f32 outputs with fewer tiles than CUs and a long reduction run with the
 * batch-reduce range of a tile split over several workgroups (xsmm_hip_force_split), small bf16 outputs with K >= 1536 on the 32x64
 * loader-wave tile. "" = the kernel xsmm_hip_kernel_name(handle) names ran. For tests, tools and profiles. */
TPP_XSMM_EXPORT const char *xsmm_hip_last_refined_kernel(void);
/* The kernel instance the most recent NON-queued unary / binary invoke launched, and that launch's total number of workgroups: which of
 * the 16-byte and the element paths a shape / stride / alignment reached ("unary_kernel<f32,v4>", "unary_kernel<bf16,v1>",
 * "binary_kernel<bf16,v8>"; ", flat" appended when contiguous operands ran as one long row), which transpose ("transpose_vec<f32,128x128>",
 * "transpose_vec<bf16,64x64>", "transpose<f32>") and which VNNI-2 pack ("vnni2_rows4<wt>", "vnni2_rows4<plain>", "vnni2<v8>", "vnni2<v1>").
 * "" / 0 before the first. The grouped launches of the tile queue do not report here, and a transpose that xsmm_hip_set_fold_transpose
 * deferred has not launched yet. Static strings; for tests, tools and profiles. */
TPP_XSMM_EXPORT const char *xsmm_hip_last_eltwise_kernel(void);
TPP_XSMM_EXPORT int64_t xsmm_hip_last_eltwise_grid(void);
/* Force a GEMM tile variant for A/B benchmarking and tests (-1 = automatic): f32 0..4 (64x64,
 * 64x32+K2, 32x32+K4, 128x64, 64x64+K2), 5..7 the loader-wave kernels (64x64, 64x64+K2, 64x32+K4), 8 generic, 9 / 10 loader-wave 32x32+K4 / 128x64, bf16 16 / 17 / 18 / 19 (64x64, 128x128, 256x256, 32x32 + K split),
 * 20 .. 23 the bf16 loader-wave tiles for mid-size outputs (32x64 + K split, 64x64, 64x128, 128x128).
 * Honoured at dispatch when the shape divides the tile;
 * 24 .. 27 the same tiles for a flat bf16 B operand, 28 .. 31 for a VNNI-4 B operand. */
TPP_XSMM_EXPORT void xsmm_hip_force_variant(int variant);
/* Skinny f32 outputs (fewer output tiles than compute units, a long batch-reduce: the reference's M = 128 / 256 benchmark shapes,
 * benchmarks/config/matmul/128x1024x4096.json ...) run with the batch-reduce range of ONE output tile split over several workgroups:
 * each adds its chunks, the workgroup that finishes last sums the partial tiles in split order (a fixed order of additions: the same
 * call pattern gives the same bits every run; no float atomics). How many workgroups share a tile is chosen per launch from the
 * descriptor, the batch count and the number of tiles in the launch; this call overrides it for the launches that FOLLOW (a test /
 * measurement switch): -1 = the model (default), 0 or 1 = never split, n > 1 = n workgroups per tile (at most 16 and at most the
 * number of 64-k chunks). Also TPP_HIP_SPLIT. Returns the previous setting. */
TPP_XSMM_EXPORT int xsmm_hip_force_split(int workgroups_per_tile);
/* Tail split (opt-in; also TPP_HIP_TAIL_SPLIT). The f32 loader-wave tiles run one workgroup per compute unit, so a whole-layer f32
 * call of q * CUs + r output tiles runs q full rounds of workgroups and a last one that occupies r CUs for a whole K loop. With the
 * tail split on, a call planned on one of the K-split tiles (64x64 + K2, 64x32 + K4, 32x32 + K4) with q >= 1 and 0 < r <= CUs / 2 runs
 * as ONE launch in which the q * CUs tiles of the full rounds run unsplit and each of the r tail tiles is shared by S workgroups on the
 * otherwise idle CUs, under the protocol of xsmm_hip_force_split (partials summed in split order by the workgroup that finishes last;
 * nobody waits for anybody). mode 0 = off (default); 1 = the model: S = min(CUs / r, 16, chunks / 4) where chunks is the number of 64-k
 * chunks of a tile, used if S >= 2 and the K-loop time it saves exceeds the hand-off; 2 .. 16 = that many workgroups per tail tile (at most
 * the chunks) wherever r * S <= CUs (a test / measurement switch). Read per invoke; returns the previous setting, -1 (and changes
 * nothing) for any other value. xsmm_hip_force_split >= 0 switches the tail split off. The choice depends on the descriptor, the batch
 * count and the CU count only, so it is made in strict mode too. Results are run-to-run reproducible and within the f32 bars; body
 * tiles have the bits of the unsplit launch, tail tiles those of a split launch with S workgroups - they differ from the unsplit launch
 * in last bits on the tail tiles only. Without a scratch block, or on a stream that is being captured, the call runs unsplit
 * (xsmm_hip_last_refined_kernel then reads ""; otherwise "..., tail split"). A chain launch is unaffected: chains already refuse grids
 * larger than the chip.
 * _stats: out[0] launches that ran with a split tail since process start; of the most recent one: [1] tail tiles, [2] workgroups per
 * tail tile, [3] body tiles. */
TPP_XSMM_EXPORT int xsmm_hip_set_tail_split(int mode);
TPP_XSMM_EXPORT void xsmm_hip_tail_split_stats(int64_t out[4]);
/* Edge tiles (opt-in; also TPP_HIP_EDGE_TILES, read as a number). A whole-layer f32 call whose m or n is not a multiple of 32 is planned
 * on the generic kernel. With edge tiles on, such a call runs on a loader-wave tile (64x64 + K2, 64x32 + K4, 32x32 + K4 or 128x64) all the
 * same, as ONE launch of ceil(m / BM) x ceil(n / BN) workgroups: the last tile of a row or column of tiles is shifted back so that it
 * ends at the matrix edge, computes a whole BM x BN block there and stores (and, with beta = 1, joins C for) only the rows and columns no
 * other tile owns. Every element is computed from its own row of A and column of B in the order of the plain tile, so the result has
 * the bits the same tile gives on the shape padded up to whole tiles; no load leaves rows [0, m) of A or columns [0, n) of B, no byte of
 * C outside the m x n window is written. No scratch block, no counters: legal on a captured stream.
 * A call takes edge tiles when all of this holds: f32, no VNNI operand, no transposed operand, not on the bf16x6 kernel, the generic
 * kernel not forced, no tile divides m x n (the descriptor's kernel is the generic one), k a positive multiple of 64, batch count >= 1,
 * lda / ldb / ldc / strides multiples of 4 and ld < 2^22, n a multiple of 4, A, B, C (and the bias row) 16-byte aligned, and m >= BM,
 * n >= BN for the tile. Everything else runs as with the mode off - also every tile-queue group, chain and folded call.
 * mode 0 = off (default); 1 = the tile rule of the divisible shapes (rounds of workgroups, a 128x64 round = 1.85 rounds of 64x64, a
 * tile per CU before a larger tile) on ceil-divided tile counts; 6 / 7 / 9 / 10 = the tile of that kernel variant (64x64 + K2, 64x32 +
 * K4, 32x32 + K4, 128x64) wherever it fits (a test / measurement switch). Read per invoke; returns the previous mode, -1 (and changes
 * nothing) for any other value. A forced split count and the tail split do not apply to an edge launch. The choice depends on the
 * descriptor, the batch count, the pointers' alignment and the CU count only, so it is made in strict mode too.
 * xsmm_hip_last_refined_kernel reads "brgemm_f32_lw<64x64,k2>, edge tiles" (<64x32,k4>, <32x32,k4>, <128x64,k1>).
 * _stats: out[0] edge launches since process start; of the most recent one: [1] tile rows, [2] tile columns, [3] the variant number
 * of its tile (6, 7, 9, 10).
 * bf16 (modes 2 and 20 .. 23; modes 1, 6, 7, 9, 10 leave every bf16 call alone). A whole-layer bf16 call no loader-wave tile divides - m not a
 * multiple of 32 or n not of 64 - is planned on the generic kernel or, with m and n multiples of 32, on the latency-bound 32x32 K-split
 * kernel. Under these modes it runs on a bf16 loader-wave tile (32x64 + K2, 64x64, 64x128, 128x128; VNNI-2, flat or VNNI-4 B image) the
 * same way: one launch of ceil(m / BM) x ceil(n / BN) workgroups, the last tile of a row or column of tiles shifted back to end at the
 * matrix edge; it stores only the rows and 16-byte pieces no other tile owns (with beta = 1 it reads C for its whole block and drops what
 * it does not own). The bits are those of the same tile on the shape padded up to whole tiles; no scratch, no counters, no waits.
 * A call takes bf16 edge tiles when all of this holds: bf16, no VNNI C, no transposed operand, neither a variant nor the generic kernel
 * forced, planned on the generic or the 32x32 K-split kernel, m % 32 != 0 or n % 64 != 0, a VNNI-2, flat or VNNI-4 B, the leading
 * dimensions, strides and lane offsets that image's loader-wave tiles ask for (lda / ldc / strides multiples of 8, ldb of 4 / 8 / 2,
 * lda, ldc < 2^22, ldb < 2^21 / 2^21 / 2^20), k a positive multiple of 64, batch count >= 1, n a multiple of 8, A, B and C 16-byte and
 * a bias row 8-byte aligned, and m >= BM, n >= BN for the tile. Everything else - every tile-queue group, quad and chain too - runs as
 * with the mode off.
 * mode 2 = mode 1's rule for f32 calls AND, for bf16 calls, the cheapest tile that fits by the fitted model of the divisible shapes
 * (rounds of workgroups over ceil-divided tile counts x (a + b x the call's 64-k chunks); ties to the larger tile); 20 / 21 / 22 / 23 =
 * the bf16 tile 32x64 + K2 / 64x64 / 64x128 / 128x128 wherever it fits, whatever the B image (a test / measurement switch; f32 calls
 * run as with the mode off).
 * xsmm_hip_last_refined_kernel reads "brgemm_bf16_lw<64x64>, edge tiles" (<32x64,k2>, <64x128>, <128x128>; brgemm_bf16_lw_flatb<...> and
 * brgemm_bf16_lw_vnni4<...> for the other images). _stats [3] is then the variant number of the tile WITH its image: 20 + t VNNI-2,
 * 24 + t flat, 28 + t VNNI-4. */
TPP_XSMM_EXPORT int xsmm_hip_set_edge_tiles(int mode);
TPP_XSMM_EXPORT void xsmm_hip_edge_tiles_stats(int64_t out[4]);
/* Ragged k (opt-in; also TPP_HIP_EDGE_K, read as a number). A whole-layer f32 call whose k is not a multiple of 64 - a 784-wide input
 * layer, a 1000-wide hidden dimension - is planned on the generic kernel, whatever the edge-tile mode. With this switch on, a call with
 * k >= 64 and k a multiple of 8 runs on a loader-wave tile (64x64 + K2, 64x32 + K4, 32x32 + K4 or 128x64) as ONE launch: every batch
 * element is read as ceil(k / 64) chunks of 64, the LAST chunk shifted back to start at k - 64 so that it ends at k, and the MFMA waves
 * skip the o = 64 - k % 64 k-values at its head that the chunk before it has multiplied (whole 8-k blocks; skipped, not multiplied by
 * zero: an Inf or NaN there counts once, as data). No load leaves [0, k) of a row of A or rows [0, k) of a B element, nothing outside
 * the m x n window of C is written. No scratch block, no counters: legal on a captured stream.
 * A call is taken when all of this holds: f32, no VNNI operand, no transposed operand, not on the bf16x6 kernel, the generic kernel
 * not forced, the descriptor's kernel is the generic one, k >= 64, k % 8 == 0, k % 64 != 0, batch count >= 1, lda / ldb / ldc / strides
 * multiples of 4 and ld < 2^22, n a multiple of 4, A, B, C (and the bias row) 16-byte aligned, m >= BM and n >= BN for the tile - and,
 * if that tile does not divide m and n, an f32 edge-tile mode (xsmm_hip_set_edge_tiles 1, 2, 6, 7, 9, 10) is on as well: the kernel
 * then also shifts back its last tile row and column. Everything else runs as with the switch off - every tile-queue group, chain and
 * folded call too.
 * mode 0 = off (default); 1 = the tile rule of the edge tiles (the divisible shapes' rule on ceil-divided tile counts; a forcing
 * edge-tile mode forces the tile); 6 / 7 / 9 / 10 = the tile of that kernel variant wherever it fits (a test / measurement switch).
 * Read per invoke; returns the previous mode, -1 (and changes nothing) for any other value. A forced split count and the tail split
 * do not apply. The choice depends on the descriptor, the batch count, the pointers' alignment and the CU count only: made in strict
 * mode too. xsmm_hip_last_refined_kernel reads "brgemm_f32_lw<64x64,k2>, ragged k", or "..., edge tiles, ragged k" when m or n is
 * ragged as well.
 * _stats: out[0] ragged-k launches since process start; of the most recent one: [1] chunks per batch element, [2] o, [3] the variant
 * number of its tile (6, 7, 9, 10). The edge-tile counters do not move on these launches. */
TPP_XSMM_EXPORT int xsmm_hip_set_edge_k(int mode);
TPP_XSMM_EXPORT void xsmm_hip_edge_k_stats(int64_t out[4]);
/* Ragged k, bf16 (opt-in; also TPP_HIP_EDGE_K_BF16, read as a number; a switch of its own: xsmm_hip_set_edge_k leaves every bf16 call
 * where it is). A whole-layer bf16 call whose k is not a multiple of 64 - a 784-wide input layer, k = 400, 1200, 2000 - is planned on
 * the generic or the 32x32 K-split kernel, whatever its m and n. With this switch on, a call with k >= 64 and k a multiple of 16 runs on
 * a bf16 loader-wave tile (32x64 + K2, 64x64, 64x128 or 128x128) as ONE launch: every batch element is read as ceil(k / 64) chunks of
 * 64, the LAST chunk shifted back to start at k - 64 so that it ends at k, and the MFMA waves skip the o = 64 - k % 64 k-values (16, 32
 * or 48) at its head that the chunk before it has multiplied (whole 16-k MFMA steps; skipped, not multiplied by zero: an Inf or NaN
 * there counts once, as data). No load leaves [0, k) of a row of A or k-rows [0, k) of a B element, nothing outside the m x n window
 * of C is written. No scratch block, no counters: legal on a captured stream.
 * A call is taken when all of this holds: bf16, no VNNI C, no transposed operand, neither a kernel variant nor the generic kernel
 * forced, the descriptor's kernel is the generic or the 32x32 K-split one, k >= 64, k % 16 == 0, k % 64 != 0, batch count >= 1, n a
 * multiple of 8, lda / ldc / strides multiples of 8 and lda, ldc < 2^22, ldb as its image asks (VNNI-2: a multiple of 4 below 2^21; flat:
 * of 8 below 2^21; VNNI-4: of 2 below 2^20), A, B, C 16-byte and the bias row 8-byte aligned, m >= BM and n >= BN for the tile - and, if
 * that tile does not divide m and n, a bf16 edge-tile mode (xsmm_hip_set_edge_tiles 2, 20 .. 23) is on as well: the kernel then also
 * shifts back its last tile row and column. Everything else runs as with the switch off - every tile-queue group, quad, chain and
 * folded call too; k % 16 != 0 (1000, 200, 72) and k < 64 stay where they are (k % 16 == 8: xsmm_hip_set_edge_k8_bf16 below).
 * mode 0 = off (default); 1 = the tile rule: the cheapest tile by the loader-wave cost model on ceil-divided tile counts among the
 * tiles that fit and - with the bf16 edge tiles off - divide m and n (a forcing edge-tile mode forces the tile); 20 .. 23 = the tile
 * 32x64 + K2 / 64x64 / 64x128 / 128x128 wherever it is such a candidate (a test / measurement switch).
 * Read per invoke; returns the previous mode, -1 (and changes nothing) for any other value. The choice depends on the descriptor, the
 * batch count, the pointers' alignment and the CU count only: made in strict mode too. xsmm_hip_last_refined_kernel reads
 * "brgemm_bf16_lw<64x64>, ragged k", or "..., edge tiles, ragged k" when m or n is ragged as well (brgemm_bf16_lw_flatb / _vnni4 for
 * a flat / VNNI-4 B).
 * _stats: out[0] bf16 ragged-k launches since process start; of the most recent one: [1] chunks per batch element, [2] o, [3] the
 * variant number of its tile with its B image (20 + t VNNI-2, 24 + t flat, 28 + t VNNI-4). The edge-tile and the f32 ragged-k counters
 * do not move on these launches. */
TPP_XSMM_EXPORT int xsmm_hip_set_edge_k_bf16(int mode);
TPP_XSMM_EXPORT void xsmm_hip_edge_k_bf16_stats(int64_t out[4]);
/* Ragged k in half steps, bf16 (opt-in; also TPP_HIP_EDGE_K8_BF16, read as a number; a switch of its own: it and xsmm_hip_set_edge_k_bf16
 * partition the lengths - k % 16 == 0 is that switch's only, k % 16 == 8 this one's only - and neither looks at the other's mode). A
 * whole-layer bf16 call with k >= 64, k a multiple of 8 but not of 16 - a 1000-wide layer, k = 200, 72 - runs on a bf16 loader-wave tile
 * (32x64 + K2, 64x64, 64x128 or 128x128) as ONE launch, read as ceil(k / 64) chunks per batch element with the LAST chunk shifted back to
 * start at k - 64, exactly as under xsmm_hip_set_edge_k_bf16. The o = 64 - k % 64 k-values at its head that the chunk before it has
 * multiplied are now 8, 24, 40 or 56: o / 16 whole 16-k MFMA steps, which are skipped, plus the LOWER half of one more step. In that one
 * step the MFMA's operands are zero in the lanes that hold the lower eight k-values, on BOTH sides, so the half adds +0.0 products only:
 * the result has the bits of a skip, and an Inf or NaN in the re-read region counts once, as data. No load leaves [0, k) of a row of A
 * or k-rows [0, k) of a B element, nothing outside the m x n window of C is written. No scratch block, no counters: legal on a captured
 * stream.
 * A call is taken when all of this holds: bf16, no VNNI C, no transposed operand, neither a kernel variant nor the generic kernel
 * forced, the descriptor's kernel is the generic or the 32x32 K-split one, k >= 64, k % 8 == 0, k % 16 != 0, batch count >= 1, n a
 * multiple of 8, lda / ldc / strides multiples of 8 and lda, ldc < 2^22, ldb as its image asks (VNNI-2: a multiple of 4 below 2^21; flat:
 * of 8 below 2^21; VNNI-4: of 2 below 2^20), A, B, C 16-byte and the bias row 8-byte aligned, m >= BM and n >= BN for the tile - and, if
 * that tile does not divide m and n, a bf16 edge-tile mode (xsmm_hip_set_edge_tiles 2, 20 .. 23) is on as well. Everything else runs as
 * with the switch off - every tile-queue group, quad, chain and folded call too; k % 8 != 0 and k < 64 stay where they are.
 * mode 0 = off (default); 1 = the tile rule of xsmm_hip_set_edge_k_bf16 (a forcing edge-tile mode forces the tile), with its gate: a call
 * on the 32x32 K-split kernel whose 32x32 tiles fit one round of the compute units and whose batch count x k is below 1024 stays;
 * 20 .. 23 = the tile 32x64 + K2 / 64x64 / 64x128 / 128x128 wherever it is a candidate (a test / measurement switch).
 * Read per invoke; returns the previous mode, -1 (and changes nothing) for any other value. The choice depends on the descriptor, the
 * batch count, the pointers' alignment and the CU count only: made in strict mode too. xsmm_hip_last_refined_kernel reads
 * "brgemm_bf16_lw<64x64>, ragged k, half step", or "..., edge tiles, ragged k, half step" when m or n is ragged as well
 * (brgemm_bf16_lw_flatb / _vnni4 for a flat / VNNI-4 B).
 * _stats: out[0] half-step launches since process start; of the most recent one: [1] chunks per batch element, [2] o, [3] the variant
 * number of its tile with its B image (20 + t VNNI-2, 24 + t flat, 28 + t VNNI-4). The counters of xsmm_hip_edge_k_bf16_stats,
 * xsmm_hip_edge_k_stats and xsmm_hip_edge_tiles_stats do not move on these launches. */
TPP_XSMM_EXPORT int xsmm_hip_set_edge_k8_bf16(int mode);
TPP_XSMM_EXPORT void xsmm_hip_edge_k8_bf16_stats(int64_t out[4]);
/* Flat and VNNI-4 B on the 256x256 bf16 tile (opt-in; also TPP_HIP_DMA256_IMAGES, read as a number). brgemm_bf16_dma256, the 256x256
 * LDS-DMA tile of large bf16 GEMMs, takes a VNNI-2 B; a large call with a flat [k][ldb] or a VNNI-4 [k/4][ldb][4] B runs on the 128x128
 * loader-wave tile, which needs twice the LDS fill per flop. With this switch on, such a call runs on the 256x256 tile with the B image of
 * its operand (kernel entry points brgemm_bf16_dma256_flatb / _vnni4: the same ring, A image, schedule and epilogue; flat rows are
 * read by ds_read_b64_tr_b16, VNNI-4 k-group rows by 8-byte reads). Every output is one chain over k, in k order, on the same MFMA as on
 * the loader-wave tile: bit for bit the result of the switch off. No scratch block, no counters: legal on a captured stream.
 * A call is taken when all of this holds: bf16, flat or VNNI-4 B, no VNNI C, neither a kernel variant nor the generic kernel forced, the
 * descriptor's kernel is a flat or VNNI-4 loader-wave tile, m and n multiples of 256, batch count >= 1, A, B, C 16-byte and the bias row
 * 8-byte aligned. Everything else runs as with the switch off - every tile-queue group, quad and chain too.
 * mode 0 = off (default); 1 = the rule that sends a VNNI-2 descriptor to the 256x256 tile (at least 240 tiles of 256x256 and the fill
 * term of the tile choice) - every such row of both images measured faster (profiles/dma256_images_ab.txt); 2 = every eligible call (a
 * test / measurement switch).
 * Read per invoke; returns the previous mode, -1 (and changes nothing) for any other value. The choice depends on the descriptor, the
 * batch count, the pointers' alignment and the CU count only: made in strict mode too. xsmm_hip_last_refined_kernel reads
 * "brgemm_bf16_dma_flatb<256x256>" or "brgemm_bf16_dma_vnni4<256x256>".
 * _stats: out[0] such launches since process start; of the most recent one: [1] tile rows, [2] tile columns, [3] the B image (2 flat,
 * 4 VNNI-4). */
TPP_XSMM_EXPORT int xsmm_hip_set_dma256_images(int mode);
TPP_XSMM_EXPORT void xsmm_hip_dma256_images_stats(int64_t out[4]);
/* Edge tiles on the 256x256 bf16 tile (opt-in; also TPP_HIP_DMA256_EDGE, read as a number). The 256x256 tile takes a call only when 256
 * divides m and n; a large call that misses this by a few rows or columns (4000 x 4096, 4096 x 4000, 8000 x 8000) runs on a much smaller
 * tile or on the generic kernel. With this switch on, such a call runs on ceil(m / 256) x ceil(n / 256) workgroups of the 256x256 tile
 * (kernel entry points brgemm_bf16_dma256_edge / _edge_flatb / _edge_vnni4: the same ring, images, schedule and K loop). The last tile row
 * starts at row m - 256 and the last tile column at column n - 256; a shifted tile computes all its elements and stores only the rows
 * and columns no other tile owns. Every output is one chain over k, in k order, on the same MFMA with one rounding: bit for bit what the
 * divisible kernel gives on the problem padded to whole tiles. No scratch block, no counters: legal on a captured stream.
 * A call is taken when all of this holds: bf16, no VNNI C, neither a kernel variant nor the generic kernel forced, m >= 256, n >= 256, m
 * or n not a multiple of 256, n % 8 == 0, k % 32 == 0, batch count >= 1, A, B, C 16-byte and the bias row 8-byte aligned, B VNNI-2, flat or
 * VNNI-4 with leading dimensions and strides on the grid of the LDS-DMA tiles. Everything else runs as with the switch off - every
 * tile-queue group, quad and chain too. The switch reads no other switch and covers flat and VNNI-4 B by itself.
 * mode 0 = off (default); 1 = the rule: at least 240 ceil-divided tiles of 256x256, and 1.4 x their occupancy of the compute units over
 * the rounds at least that of the ceil-divided 128x128 tiles - measured (profiles/dma256_edge_ab.txt, K = 1024, every switch off /
 * xsmm_hip_set_edge_tiles(2) -> on): 4000x4096 154.3 / 152.9 -> 35.0 us, 4096x4000 214.1 / 45.3 -> 36.0, 5000x5000 412.6 / 85.1 -> 64.8,
 * 8000x8000 350.7 / 346.4 -> 135.0, 16000x1024 49.0 / 49.2 -> 38.7, flat and VNNI-4 B alike; the occupancy term refuses 4100x4096 (272
 * tiles, a partial second round: 52.0 us on the 128x128 edge tile, 58.3 here); 2 = every eligible call (a test / measurement switch).
 * Read per invoke; returns the previous mode, -1 (and changes nothing) for any other value. The choice depends on the descriptor, the
 * batch count, the pointers' alignment and the CU count only: made in strict mode too. xsmm_hip_last_refined_kernel reads
 * "brgemm_bf16_dma<256x256>, edge tiles", "brgemm_bf16_dma_flatb<256x256>, edge tiles" or "brgemm_bf16_dma_vnni4<256x256>, edge tiles".
 * _stats: out[0] such launches since process start; of the most recent one: [1] tile rows, [2] tile columns (ceil-divided), [3] the B
 * image (0 VNNI-2, 2 flat, 4 VNNI-4). The counters of the other switches do not move on these launches. */
TPP_XSMM_EXPORT int xsmm_hip_set_dma256_edge(int mode);
TPP_XSMM_EXPORT void xsmm_hip_dma256_edge_stats(int64_t out[4]);
/* Skinny-batch bf16 layers (opt-in; also TPP_HIP_SKINNY_BF16, read as a number). A bf16 call with fewer than 32 rows - batch 1, 4, 8 or 16
 * of online inference - runs on the generic kernel: one workgroup per 32x32 output tile (n / 32 workgroups), a 32-row MFMA of which m rows
 * are used, B read in 64-byte row pieces and staged through LDS. Such a layer is a weight stream: its time is the bytes of B. With this
 * switch on, the call runs on ceil(n / BN) workgroups of brgemm_bf16_skinny<IMG, BN, MB> (brgemm_bf16_skinny.hip; maps in
 * brgemm_bf16_skinny.h), BN = 16, 32 or 64: one workgroup computes ALL m rows of one block of BN columns on v_mfma_f32_16x16x32_bf16 - one
 * accumulator set for m <= 16 (MB = 16), two that share every B fragment for m = 17 .. 31 (MB = 32). B goes from global memory straight
 * into the MFMA operand registers, without LDS: per 32-k step a lane loads its 8 k values of BN / 16 consecutive columns - 4 pair-rows of a
 * VNNI-2 B, 2 k-group rows of a VNNI-4 B, 8 k-rows of a flat B, 4 .. 16 bytes each - and the operand of MFMA j is a selection of their
 * halves; a lane ends up with BN / 16 consecutive columns of four rows and stores them as one piece per row. A flat B has no BN = 16
 * instance (it would need 2-byte loads): eight B instances x two MB. The stream of 32-k steps over (batch element, k) is dealt over
 * W = min(8, br * ceil(k / 32)) waves of the workgroup in contiguous runs, four steps of loads in flight per wave; the partial accumulators
 * are added through LDS in wave order, then beta 1's C, the bias, relu and ONE rounding to bf16. W depends on br and k alone, so an
 * element's chain of additions depends neither on m, nor on n, nor on where its column block sits, and the bits are the same on every run.
 * A row at or beyond m is read from row m - 1 and never stored; for k % 32 != 0 the lane groups of a batch element's last step whose k
 * values do not exist issue no load and feed zeros on both sides; the last column block is shifted back to end at n and stores only the
 * columns no other block owns. No load leaves rows [0, m) x [0, k) of A, [0, k) x [0, n) of a B element or the bias row, nothing outside
 * the m x n window of C is written. No cross-workgroup synchronisation, no scratch block, no counters: legal on a captured stream.
 * A call is taken, at invoke time, when all of this holds: bf16, B VNNI-2, flat or VNNI-4, no VNNI C, no transposed operand, neither a
 * kernel variant nor the generic kernel forced, the descriptor's kernel is the generic one, 1 <= m <= 31, n >= BN, n % 8 == 0, k >= 8,
 * k % 8 == 0 per batch element, batch count >= 1, lda >= k, ldb >= n, ldc >= n, lda, ldb, ldc, stride_a and stride_b multiples of 8
 * elements, A, B and C 16-byte and the bias row 8-byte aligned. The launcher checks the same again; a call it refuses runs the launch of
 * mode 0. Everything else runs exactly as with the switch off - f32 calls, m >= 32, every tile-queue group, quad, chain launch and folded
 * call. No other switch takes a bf16 call with m < 32, and this one reads no other mode: there is no precedence question.
 * mode 0 = off (default); 1 = the rule, measured (profiles/skinny_bf16_ab.txt: one MI355X, 256 CUs, beta 0 + bias + relu, five alternating
 * rounds, us per call, generic kernel -> skinny; a BN is taken only where it was faster in every round). THE GATE: a call with m >= 17
 * that the generic kernel runs on its 16-byte path (a VNNI B, k % 32 == 0) stays there - it lost on every BN in every round (1024 x 1024
 * (n x K) 5.00 -> 5.72 on BN 16, 4096 x 4096 12.41 -> 14.31, 4096 x 1024 5.07 -> 5.96, 1024 x 4096 10.78 -> 11.36). Every other eligible call is
 * taken: where B (2 br k n bytes) has at least 16 MiB on the BN whose row piece is one 128-byte line - 32 for VNNI-2, 16 for VNNI-4, 64 for
 * flat (4096 x 4096, m 1 / 8 / 16: 11.34 / 12.02 / 12.15 -> 9.19 / 10.55 / 10.88; VNNI-4 m 8 11.78 -> 8.35; flat m 8 136.39 -> 14.87) -, a
 * smaller B on the smallest BN with an instance, 16 or flat 32 (1024 x 1024 m 8 5.02 -> 4.49, 4096 x 1024 4.97 -> 4.31, 1024 x 4096 10.67 ->
 * 6.75; k = 1000, the generic kernel's element path, 1000 x 1000 m 1 / 8 / 16 / 31: 34.82 / 35.04 / 37.31 / 41.49 -> 4.63 / 4.17 / 4.20 / 5.05),
 * halved while n < BN. The rule reads no CU count: other counts, several ranks, beta 1 and a B between 8 and 32 MiB were not measured.
 * 16, 32, 64 = every eligible call on that BN (test / measurement switches; a flat B under 16 and n < BN stay where they are).
 * Read per invoke; returns the previous mode, -1 (and changes nothing) for any other value. The choice depends on the descriptor, the
 * batch count, the pointers' alignment and the CU count only: made in strict mode too. xsmm_hip_last_refined_kernel reads
 * "brgemm_bf16_skinny<MBxBN>", "brgemm_bf16_skinny_flatb<MBxBN>" or "brgemm_bf16_skinny_vnni4<MBxBN>" (MB 16 / 32, BN 16 / 32 / 64).
 * _stats: out[0] such launches since process start; of the most recent one: [1] workgroups, [2] waves per workgroup, [3] BN, [4] the B
 * image (0 VNNI-2, 2 flat, 4 VNNI-4). The counters of the other switches do not move on these launches. */
TPP_XSMM_EXPORT int xsmm_hip_set_skinny_bf16(int mode);
TPP_XSMM_EXPORT void xsmm_hip_skinny_bf16_stats(int64_t out[5]);
/* A K split across workgroups for the skinny-batch kernel (opt-in; also TPP_HIP_SKINNY_SPLIT, read as a number). The skinny launch above
 * has ceil(n / BN) workgroups - 64 for a 1024-wide layer on BN 16 -, too few to keep enough bytes of B in flight: it is bound by bytes in
 * flight, not by HBM. With this switch on, a call that xsmm_hip_set_skinny_bf16 has put on the skinny kernel runs on
 * brgemm_bf16_skinny_split<IMG, BN, MB> (brgemm_bf16_skinny_split.hip; maps in brgemm_bf16_skinny_split.h): the S = br * ceil(k / 32)
 * steps of the call go to P_eff = min(P, S) parts in contiguous runs, ceil(n / BN) * P_eff workgroups in all, part-major. A part runs its
 * steps as the unsplit kernel does, parks its f32 partial accumulators with write-through stores in the stream's scratch block and adds
 * one to the column block's arrival counter; the LAST workgroup to arrive, whichever it is, resets the counter, sums ALL partials in part
 * order and runs the unsplit epilogue (beta 1's C, bias, relu, one rounding). No workgroup waits for another and none need be resident
 * together; a result's bits depend on br, k and P_eff alone, not on m, n, the block or the arrival order. They are NOT the bits of the
 * unsplit kernel (another order of f32 additions); on exact inputs both are the oracle's.
 * It refines the skinny launch and nothing else: with xsmm_hip_set_skinny_bf16 at 0 it changes nothing, BN and the m >= 17 gate stay that
 * switch's, no other switch reads it and no other counter moves. P_eff < 2 is the plain skinny launch. The launcher refuses a launch
 * with more than 4096 column blocks, more than 16 parts, more than 32 MiB of partials, or without a scratch block (no memory, a 17th
 * stream, a stream being captured into a graph): the call then runs the UNSPLIT skinny launch of the same BN.
 * mode 0 = off (default); 1 = the rule (gemm_plan.cpp skinny_split_parts, fitted to profiles/skinny_split_ab.txt); 2 .. 16 = that many
 * parts P wherever eligible (test / measurement switches). Read per invoke; returns the previous mode, -1 (and changes nothing) for any
 * other value. The choice depends on the descriptor, the batch count and the CU count only: made in strict mode too.
 * xsmm_hip_last_refined_kernel reads "brgemm_bf16_skinny_split<MBxBN>", "..._split_flatb<MBxBN>" or "..._split_vnni4<MBxBN>".
 * _stats: out[0] skinny launches that ran split since process start; of the most recent one: [1] P_eff, [2] workgroups (column blocks *
 * P_eff). A split launch is still a skinny launch: xsmm_hip_skinny_bf16_stats counts it, with [1] = column blocks * P_eff and [2] = the
 * waves of part 0. */
TPP_XSMM_EXPORT int xsmm_hip_set_skinny_split(int mode);
TPP_XSMM_EXPORT void xsmm_hip_skinny_split_stats(int64_t out[3]);
/* Layer chains on the 256x256 bf16 tile (opt-in; also TPP_HIP_CHAIN_DMA256, read as a number). Every chain form above is a form of the
 * loader-wave tiles (32x64 .. 128x128); a chain whose calls run on the 256x256 LDS-DMA tile - 16384 rows x 1024 columns are exactly 256
 * such tiles - ran call by call. With this switch on, xsmm_hip_fused_brgemm_chain_invoke runs such a chain as ONE launch of that tile's
 * chain kernel (entry points brgemm_bf16_dma256_chain / _chain_flatb / _chain_vnni4: the same ring, images, schedule, K loop and epilogue):
 * G x n / 256 resident workgroups, workgroup (g, tn) computes tile (tm, tn) of every layer for the row blocks tm = g, g + G, .. of its
 * group, layer by layer; G = m / 256 when the grid fits the compute units (one round), fewer otherwise. The hand-off between layers is
 * the chain's: write-through stores, a counter per row block that only grows, a bounded wait that ends in the error word, never in a
 * hang; probation, the journal and the re-run of a starved launch are the ones described at xsmm_hip_fused_brgemm_chain_invoke. Every
 * output is computed as the same call on the 256x256 tile computes it: bit for bit the separate calls on that tile.
 * A chain is eligible when all of this holds: 2 .. 8 calls, all bf16 and beta 0 with the same m and n, 256 dividing both, no VNNI C, not
 * the forced generic kernel, one B image (VNNI-2, flat or VNNI-4) with leading dimensions and strides on the tile's grid, every k a
 * multiple of 32, every batch count >= 1, n / 256 at most the stream's compute units - and what every chain launch asks: asynchronous
 * mode, no stream capture, A, B, C 16-byte and bias rows 8-byte aligned, each call reading its predecessor's output, batch elements
 * inside their rows, device operands, no overlaps. Everything else - and every chain with the mode 0 - is decided exactly as without
 * this switch: it is asked first, no other switch reads it, and it reads no other mode but xsmm_hip_set_dma256_images' in mode 1.
 * mode 0 = off (default); 1 = the rule: an eligible chain EVERY call of which runs on the 256x256 tile as a single call today - VNNI-2:
 * dispatched on that tile; flat / VNNI-4: xsmm_hip_set_dma256_images is non-zero and takes the call - subject to the measured gate of
 * gemm_plan.h plan_chain_dma256 (profiles/chain_dma256_ab.txt); 2 = every eligible chain (a test / measurement switch); 1000 + G = every
 * eligible chain on G row groups, 1 <= G <= m / 256 and G * n / 256 at most the compute units (likewise). Read per invoke; returns the
 * previous mode, -1 (and changes nothing) for any other value. Strict mode takes a chain only where every call was dispatched on the
 * tile: the launch then has the separate calls' bits.
 * _stats: out[0] such launches since process start; of the most recent one: [1] resident row groups G (m / 256 in one round), [2]
 * rounds ceil(m / 256 / G), [3] the B image (0 VNNI-2, 2 flat, 4 VNNI-4). The counters of the other switches do not move on these launches. */
TPP_XSMM_EXPORT int xsmm_hip_set_chain_dma256(int mode);
TPP_XSMM_EXPORT void xsmm_hip_chain_dma256_stats(int64_t out[4]);
/* Skinny-batch layer chains (opt-in; also TPP_HIP_CHAIN_SKINNY, read as a number; a refused value leaves 0). Every chain form above asks for
 * m >= 32, so a chain with 1 .. 31 rows - decode, small-batch inference - ran call by call. With this switch on,
 * xsmm_hip_fused_brgemm_chain_invoke runs such a chain as ONE launch of the skinny-batch kernel's chain form (brgemm_bf16_skinny_chain): G
 * resident workgroups, workgroup w computing the column blocks w, w + G, .. of BN columns of every layer, layer by layer, each block as
 * the single skinny call computes it. The hand-off between layers is the chain's: write-through stores, ONE counter per seam that only
 * grows (a launch adds G), a bounded wait that ends in the error word, never in a hang; the next layer's weights are requested ahead of
 * the wait. Probation, the journal and the re-run of a starved launch are the ones described at xsmm_hip_fused_brgemm_chain_invoke.
 * Every output is bit for bit the same calls made one by one under xsmm_hip_set_skinny_bf16(BN) with xsmm_hip_set_skinny_split(0).
 * A chain is eligible when all of this holds: 2 .. 8 calls, all bf16 and beta 0 with the same m in 1 .. 31, no VNNI C, no forced kernel,
 * one B image (VNNI-2, flat or VNNI-4), per call n >= BN, n % 8 == 0, k >= 8, k % 8 == 0, a batch count >= 1, leading dimensions that
 * cover their operands and, like the strides, are multiples of 8 elements, lda and ldc below 2^24 - the widths may differ from call to
 * call - and what every chain launch asks: asynchronous mode, no stream capture, A, B, C 16-byte and bias rows 8-byte aligned, each
 * call reading its predecessor's output, batch elements inside their rows, device operands, no overlaps. Strict mode
 * (xsmm_hip_set_strict) stays call by call: the launch has the bits of the skinny kernel, not of the calls as dispatched. Everything
 * else - every chain with m >= 32, and every chain with the mode 0 - is decided exactly as without this switch. It reads neither
 * xsmm_hip_set_skinny_bf16 nor xsmm_hip_set_skinny_split, which decide single calls only, and neither reads it.
 * mode 0 = off (default); 1 = the rule: the smallest BN with an instance, G = min(column blocks of the widest layer, compute units),
 * subject to the measured gate of gemm_plan.cpp plan_chain_skinny (profiles/chain_skinny_ab.txt): a chain with a layer of more than 2 MiB
 * of B, and a chain with a flat or a VNNI-4 B, stays call by call - 1024-wide VNNI-2 MLPs gain 22 .. 31 % at m <= 16, 4096-wide ones lose
 * 14 % and more to the split single calls; 16 / 32 / 64 = that BN wherever eligible, never gated; 1000 * G + BN,
 * 1 <= G <= 512 = that BN on G resident workgroups, refused where G exceeds the compute units (tests, measurements). Read per invoke;
 * returns the previous mode, -1 (and changes nothing) for any other value.
 * _stats: out[0] such launches since process start; of the most recent one: [1] resident workgroups G, [2] BN, [3] the B image (0
 * VNNI-2, 2 flat, 4 VNNI-4). The counters of the other switches, xsmm_hip_skinny_bf16_stats among them, do not move on these launches. */
TPP_XSMM_EXPORT int xsmm_hip_set_chain_skinny(int mode);
TPP_XSMM_EXPORT void xsmm_hip_chain_skinny_stats(int64_t out[4]);
/* Halves (on by default; also TPP_HIP_F32_HALVES, read as a number). A whole-layer f32 call on the 64x64 + K2 loader-wave tile runs one
 * workgroup of 8 MFMA waves per tile and CU; every SIMD then holds two MFMA waves that meet the same barrier. With this switch on, every 64x64
 * tile of such a call runs as TWO independent workgroups of 4 MFMA waves, one per 32-column half (64x32, the chunk still split over two
 * K groups), two workgroups to a CU. Every output element is computed exactly as before - the same two k-ordered chains, summed in the
 * same order: bit for bit the result of the switch off. xsmm_hip_kernel_name and xsmm_hip_last_refined_kernel do not change. No scratch
 * block, no counters, no waiting between workgroups: legal on a captured stream and in strict mode.
 * A call is taken when all of this holds: it would run on launch_f32_lw's 64x64 + K2 tile as ONE plain launch (no split, forced or
 * modelled; no tail split; not an edge-tile or ragged-k launch), m and n multiples of 64. Tile-queue groups and chain launches run as
 * with the switch off.
 * mode 0 = off; 1 = the rule (default): eligible calls with at least one 64x64 tile per compute unit, where the form measured faster
 * (profiles/f32_halves_ab.txt); 2 = wherever eligible (a test / measurement switch). Read per invoke; returns the previous mode, -1
 * (and changes nothing) for any other value.
 * _stats: out[0] launches carried out as halves since process start; of the most recent one: [1] rows and [2] columns of 64x64 tiles;
 * [3] 0. */
TPP_XSMM_EXPORT int xsmm_hip_set_f32_halves(int mode);
TPP_XSMM_EXPORT void xsmm_hip_f32_halves_stats(int64_t out[4]);
/* Ragged-m layer chains, opt-in (environment: TPP_HIP_CHAIN_EDGE; default 0 = off): a switch of its own - the four ragged-layer switches
 * above decide single calls and leave every decision of xsmm_hip_fused_brgemm_chain_invoke where it is. mode 1: a bf16 chain of 2 .. 8
 * calls whose m is not a multiple of the tile's rows BM runs as ONE launch on ceil(m / BM) x n / BN workgroups - the last row block is
 * shifted back to end at row m, stores only the rows no other block owns, and waits at every seam for both row blocks whose rows it
 * reads - when everything else the chain launch asks holds as before (one kind of B operand, beta 0, equal m and n, device pointers,
 * asynchronous mode, no stream capture, no output overlapping an operand, batch elements inside the predecessor's rows) and m >= BM,
 * n % BN == 0, every k % 64 == 0 and ceil(m / BM) * (n / BN) <= the stream's compute units. The tile: the one
 * xsmm_hip_set_edge_tiles(20 .. 23) names if it fits, else the smallest of the four that fits. Bit for bit the same calls made one by
 * one on that tile. Call by call as before: strict mode (xsmm_hip_set_strict: the chain tile is no function of the descriptor alone),
 * f32 chains, a ragged n or k, a forced kernel, m below every tile's rows - and every chain a tile's rows divide runs as with the switch
 * off. The launch still needs the device to itself: a starved launch degrades exactly as a divisible one, through probation, the
 * journal and the re-run (xsmm_hip_chain_status counts). Returns the previous value, -1 (nothing changed) for any other value.
 * _stats: out[0] ragged chain launches since process start; of the most recent one: [1] tile rows ceil(m / BM), [2] tile columns
 * n / BN, [3] the variant number of its tile with its B image (20 + t VNNI-2, 24 + t flat, 28 + t VNNI-4), as
 * xsmm_hip_edge_tiles_stats reports it. The edge-tile counters do not move on these launches. */
TPP_XSMM_EXPORT int xsmm_hip_set_chain_edge(int mode);
TPP_XSMM_EXPORT void xsmm_hip_chain_edge_stats(int64_t out[4]);
/* Multi-round layer chains, opt-in (environment: TPP_HIP_CHAIN_ROUNDS; default 0 = off): a switch of its own - every other switch keeps its
 * meaning. A chain launch needs every workgroup resident, so without this switch a bf16 chain runs as one launch only while its output
 * tiles are no more than the stream's compute units (three 1024-wide layers: up to 4096 rows on 256 CUs) and call by call beyond. mode 1: a
 * bf16 chain of 2 .. 8 calls that meets everything else the chain launch asks (one kind of B operand, beta 0, equal m and n, device
 * pointers, asynchronous mode, no stream capture, no output overlapping an operand, batch elements inside the predecessor's rows) but has
 * MORE tiles than compute units runs as ONE launch on G x n / BN resident workgroups: G row groups, workgroup (g, tn) computing the row
 * blocks g, g + G, g + 2G, .. of every layer, layer by layer, and waiting at every seam for the counter of the row block it is about to
 * read - a block its own row of workgroups stored R - 1 blocks earlier, R = ceil(tiles_m / G) rounds. The tile: the loader-wave tile all
 * calls were planned on; if they share none, call by call in strict mode, else the largest tile whose rows divide m and whose columns
 * divide n. The groups: Gmax = CUs / (n / BN) rounded down, R = ceil(tiles_m / Gmax), G = ceil(tiles_m / R) (8192 x 1024 on 256 CUs:
 * 128x128 tiles, G = 32, R = 2; 4224 rows: G = 17, R = 2). Bit for bit the same calls made one by one on that tile, so strict mode takes
 * the rule on the planned tile. Mode 1 takes at most TWO rounds: deeper chains measured slower than call by call (16384 rows +4.6 %, 32768
 * rows +12.8 %, profiles/chain_rounds_ab.txt) and stay call by call. mode 1000 + G: force G row groups (1 <= G < tiles_m, G * (n / BN) <= CUs) - for tests and measurements; it
 * is asked in front of the one-round rules and so also applies to a chain that would fit; a G that does not fit leaves every decision as
 * with the switch off. Call by call (or as with the switch off) as before: f32 chains, a ragged m, n or k (xsmm_hip_set_chain_edge and
 * this switch never combine: where a one-round ragged launch applies it is taken, and a ragged shape is never run in several rounds),
 * a row of tiles wider than the compute units, a chain that fits in one round under mode 1 (today's chain kernel). The launch still
 * needs the device to itself: a starved launch degrades exactly as every chain launch, through probation, the journal and the re-run
 * (xsmm_hip_chain_status counts). Returns the previous value, -1 (nothing changed) for any other value.
 * _stats: out[0] multi-round chain launches since process start; of the most recent one: [1] row groups G, [2] rounds R =
 * ceil(tiles_m / G), [3] the variant number of its tile with its B image (20 + t VNNI-2, 24 + t flat, 28 + t VNNI-4). The chain-edge
 * and edge-tile counters do not move on these launches. */
TPP_XSMM_EXPORT int xsmm_hip_set_chain_rounds(int mode);
TPP_XSMM_EXPORT void xsmm_hip_chain_rounds_stats(int64_t out[4]);
/* Ragged-width layer chains, opt-in (environment: TPP_HIP_CHAIN_RAGGED; default 0 = off): a switch of its own - no other switch changes
 * meaning: xsmm_hip_set_chain_edge still takes 0 and 1 and still leaves a ragged n or k call by call. mode 1: a bf16 chain of 2 .. 8 calls
 * runs as ONE launch on ceil(m / BM) x ceil(n / BN) workgroups when every call is beta 0, stores no VNNI C and is not forced to a kernel
 * (the generic kernel included); all calls have the same m, n and B image (VNNI-2, flat or VNNI-4); every call's leading dimensions, strides
 * and alignment are those the edge tiles ask (xsmm_hip_set_edge_tiles) with the k term replaced by "k >= 64 and k % 8 == 0" - per layer k
 * may be whole (k % 64 == 0), a multiple of 16, or a multiple of 8; n % 8 == 0, m >= BM, n >= BN, every batch count >= 1; at least one of
 * n % BN != 0 or some k % 64 != 0 holds (m may be ragged or not); ceil(m / BM) * ceil(n / BN) <= the stream's compute units; the runtime
 * is not in strict mode - and everything else the chain launch asks holds as before (each call reads its predecessor's output, batch
 * elements inside the predecessor's rows, device pointers, no overlaps, asynchronous mode, no stream capture). The rule is asked only
 * where the other rules refuse because of n or k: a chain ragged in m alone stays xsmm_hip_set_chain_edge's, a divisible chain the plain
 * chain's, and the multi-round switch never combines with this one (more tiles than compute units: call by call). The tile: the one
 * xsmm_hip_set_edge_tiles(20 .. 23) names if it fits, else the smallest of the four that fits; the 64x128 tile has no VNNI-2 instance in
 * this mode (it would need scratch) and is passed over for such chains. Rows as under xsmm_hip_set_chain_edge; the last column tile is
 * shifted back to end at column n and stores only its own columns; every batch element of a layer is ceil(k / 64) chunks, the last one
 * shifted back to end at k, the k-values it holds again skipped in half steps of 8. Bit for bit the same calls made one by one on that
 * tile under xsmm_hip_set_edge_tiles / _edge_k_bf16 / _edge_k8_bf16 (the same k-values in the same order, one rounding). Two regions
 * measured slower as one launch and stay call by call unless an edge-tile mode forces a tile (profiles/chain_ragged_ab.txt): a VNNI-2
 * chain whose tile by the rule would be 64x128 and that would land on 128x128 (2000 rows x 1000: +13 %), and a chain with a whole-k layer
 * of an even chunk count on the 32x64 or 64x64 tile (1024 rows x [1024, 1000, 1000]: +3.5 %). A starved launch
 * degrades as every chain launch. Returns the previous value, -1 (nothing changed) for any other value.
 * _stats: out[0] ragged-width chain launches since process start; of the most recent one: [1] tile rows ceil(m / BM), [2] tile columns
 * ceil(n / BN), [3] the variant number of its tile with its B image (20 + t VNNI-2, 24 + t flat, 28 + t VNNI-4). The chain-edge,
 * chain-rounds and single-call edge counters do not move on these launches. */
TPP_XSMM_EXPORT int xsmm_hip_set_chain_ragged(int mode);
TPP_XSMM_EXPORT void xsmm_hip_chain_ragged_stats(int64_t out[4]);
/* Mixed-width layer chains, opt-in (environment: TPP_HIP_CHAIN_WIDTHS; default 0 = off): a switch of its own - no other switch changes
 * meaning. The chain contract asks for the same m AND n in every call; mode 1 widens it: a bf16 chain of 2 .. 8 calls whose n differ in at
 * least two calls runs as ONE launch on m / BM x max_l(n_l / BN) workgroups when all calls have the same m; every call is beta 0, stores
 * no VNNI C, was not dispatched to the generic kernel and has the same B image (VNNI-2, flat or VNNI-4) of the loader-wave tiles; every
 * k >= 64 and a multiple of 64, every batch count >= 1; BM divides m and BN divides every n_l; m / BM * max_l(n_l / BN) <= the stream's
 * compute units - and everything else the chain launch asks holds as before (each call reads its predecessor's output, batch elements
 * inside the predecessor's rows, device pointers, no overlaps, asynchronous mode, no stream capture). The tile: the loader-wave tile ALL
 * calls were dispatched on if it fits - the launch then has the bits of the calls made one by one, so strict mode takes it -, otherwise
 * (never in strict mode) the smallest tile that fits. Workgroup (tm, tn) computes tile (tm, tn) of every layer with a column tile tn and
 * sits out the others; the counter of layer l and row block tm receives n_l / BN arrivals per launch. The rule is asked only where the
 * calls differ in n: equal widths stay the plain chain's; a ragged m, n or k together with different widths, more tiles than compute
 * units, and f32 stay call by call whatever the other chain switches say. A starved launch degrades as every chain launch. Returns the
 * previous value, -1 (nothing changed) for any other value.
 * _stats: out[0] mixed-width chain launches since process start; of the most recent one: [1] row blocks m / BM, [2] column tiles of the
 * widest layer max_l(n_l / BN), [3] the variant number of its tile with its B image (20 + t VNNI-2, 24 + t flat, 28 + t VNNI-4). The
 * counters of the other chain modes and of the single-call edge switches do not move on these launches. */
TPP_XSMM_EXPORT int xsmm_hip_set_chain_widths(int mode);
TPP_XSMM_EXPORT void xsmm_hip_chain_widths_stats(int64_t out[4]);
/* Column rounds of mixed-width layer chains, opt-in (environment: TPP_HIP_CHAIN_WIDTH_ROUNDS, read as a number; default 0 = off): a switch
 * of its own - xsmm_hip_set_chain_widths and every other switch keep their meaning. Mode 1: a chain that passes what
 * xsmm_hip_set_chain_widths(1) asks of the calls (bf16, 2 .. 8 calls, the same m, at least two different n, beta 0, no VNNI C, not the
 * generic kernel, one B image of the loader-wave tiles, every k >= 64 and a multiple of 64, every batch count >= 1, BM divides m and BN
 * every n_l) runs as ONE launch on m / BM x W resident workgroups, 1 <= W < max_l T_l with T_l = n_l / BN and m / BM * W <= the stream's
 * compute units: workgroup (tm, c) walks the column tiles c, c + W, .. of every layer that has them, layer by layer, and sits out a
 * layer with T_l <= c. So a chain whose widest layer has more tiles than compute units (4096 rows x [1024, 4096, 1024]), which the
 * one-round launch refuses, runs as one launch. W for a tile: Wfit = min(max T - 1, compute units / (m / BM)), R = ceil(max T / Wfit),
 * W = ceil(max T / R). The tile: the loader-wave tile ALL calls were dispatched on if it fits with its W - the launch then has the bits of
 * the calls made one by one, so strict mode takes it -, otherwise (never in strict mode) the tile with the smallest K-loop time
 * sum_l ceil(T_l / W) * (the tile's fitted time per 64-k chunk) * batch_l * k_l / 64, ties to the larger tile. Where
 * xsmm_hip_set_chain_widths(1) is on as well and takes the chain, its one-round launch runs as before; this rule is asked where that one
 * refuses or gates, or is off. THE GATE: what measured slower than call by call stays call by call in mode 1
 * (profiles/chain_width_rounds_ab.txt; gemm_plan.h chain_width_rounds_gated names the regions and quotes the rows).
 * Mode 1000 + W (W >= 1; a test and measurement switch): that W on the tile all calls were dispatched on, without one on the smallest tile
 * that fits with it; asked in front of xsmm_hip_set_chain_widths' rule, never gated; a W that does not fit (W >= max T included) leaves
 * every decision as with the switch off. A ragged m, n or k, f32 and synchronous mode stay call by call whatever the other switches say.
 * A starved launch degrades as every chain launch. Returns the previous value, -1 (nothing changed) for any value other than 0, 1 and
 * 1000 + W.
 * _stats: out[0] column-round launches since process start; of the most recent one: [1] row blocks m / BM, [2] workgroup columns W,
 * [3] the variant number of its tile with its B image (20 + t VNNI-2, 24 + t flat, 28 + t VNNI-4). The counters of the other chain modes
 * and of the single-call edge switches do not move on these launches, nor this one on theirs. */
TPP_XSMM_EXPORT int xsmm_hip_set_chain_width_rounds(int mode);
TPP_XSMM_EXPORT void xsmm_hip_chain_width_rounds_stats(int64_t out[4]);
/* Ragged mixed-width layer chains, opt-in (environment: TPP_HIP_CHAIN_WIDTHS_RAGGED; default 0 = off): a switch of its own - no other switch
 * changes meaning, and none of their counters moves on these launches. Mode 1: a bf16 chain of 2 .. 8 calls with the same m and at least
 * two different n that NO tile divides entirely - a ragged m, a ragged n_l or a k_l that is no multiple of 64: 784-512-256-128, a funnel on
 * 1000 rows - runs as ONE launch on ceil(m / BM) x max_l ceil(n_l / BN) workgroups (launch mode 11 of the loader-wave tile) when every call
 * is beta 0, stores no VNNI C, was not dispatched to a forced kernel (the generic kernel included) and has the same B image (VNNI-2, flat
 * or VNNI-4) with the leading dimensions, strides and alignment the edge tiles ask of it; every k >= 64 and k % 8 == 0, every batch count
 * >= 1, every n_l % 8 == 0; m >= BM and every n_l >= BN; ceil(m / BM) * max_l ceil(n_l / BN) <= the stream's compute units; not in strict
 * mode - and everything else the chain launch asks holds as before (each call reads its predecessor's output with lda = ldc, batch elements
 * inside the predecessor's rows, device pointers, no overlaps, asynchronous mode, no stream capture). Refused, so call by call: f32, an n
 * or k that is no multiple of 8, k < 64, m or an n_l below every tile, more tiles than compute units, a forced kernel, synchronous mode,
 * calls that differ in m.
 * Bits: those of the same calls made one by one on the launch's tile under xsmm_hip_set_edge_tiles / _edge_k_bf16 / _edge_k8_bf16(20 + t):
 * the same k-values in the same order, one rounding per layer; no load outside rows [0, m) of A or k-rows [0, k) / columns [0, n_l) of B,
 * no byte outside any layer's m x n_l window written.
 * The partition (the descriptors alone decide): a chain SOME tile divides entirely (BM | m, BN | every n_l, every k_l % 64 == 0) is
 * xsmm_hip_set_chain_widths' / _width_rounds', or call by call with those off - never this switch's; equal widths are the other three chain
 * switches' as before. The tile: the one xsmm_hip_set_edge_tiles(20 .. 23) names if it fits and has an instance (64x128 with the VNNI-2
 * image has none: it would need scratch), else the smallest tile that fits and has one.
 * The gate (structural, xsmm_hip_set_chain_widths'): a chain in which some layer alone fits a smaller tile than the launch's stays call by
 * call unless an edge-tile mode forces the tile (profiles/chain_widths_ragged_ab.txt holds the measurement). A starved launch degrades as
 * every chain launch. Returns the previous value, -1 (nothing changed) for any other value.
 * _stats: out[0] ragged mixed-width launches since process start; of the most recent one: [1] row blocks ceil(m / BM), [2] column tiles of
 * the widest layer max_l ceil(n_l / BN), [3] the variant number of its tile with its B image (20 + t VNNI-2, 24 + t flat, 28 + t VNNI-4). */
TPP_XSMM_EXPORT int xsmm_hip_set_chain_widths_ragged(int mode);
TPP_XSMM_EXPORT void xsmm_hip_chain_widths_ragged_stats(int64_t out[4]);
/* Transposes folded into the gemm they feed (tile queue on, asynchronous mode, device operands, f32). A contraction with a
 * transposed B operand reaches the runtime as xsmm.unary transpose into a small temporary + xsmm.gemm reading it, per tile and with
 * ONE temporary per caller (test/Conversion/LinalgToXsmm/linalg-to-gemm.mlir:46-62, the lowering of
 * benchmarks/mlir/fp32-query-times-key.mlir): a dependence chain through the temporary that no queue can batch. So a transpose of a
 * tile of at most 64x64 into a dense destination (ldo = m) is remembered instead of launched; a gemm of the same thread whose B
 * operand is exactly that destination (k, n, ldb matching, one batch element) reads B transposed from the transpose's SOURCE (all
 * such gemms of a loop are one queue group = one launch); a later transpose of the same handle into the same destination replaces
 * the remembered one (it is dead: fully overwritten, its readers were served); any other invoke of the thread, xsmm_hip_flush and
 * every synchronisation point launch the remembered transpose first - whenever anything can look at the destination it holds what
 * the program wrote. Results of a folded gemm are those of the generic kernel on the same values. One remembered transpose per
 * calling thread (the reference's OpenMP callers own a temporary each); an invoke of another thread launches it first only if it
 * touches the destination or writes the source.
 * mode (also TPP_HIP_FOLD_TRANSPOSE=0|1|2, read as a number): 0 = off; 1 = the above (default); 2 (opt-in) = the above, and
 *  - a gemm of the same thread whose A operand is exactly the destination folds too: pa == destination and pb != destination, one
 *    batch element, f32 without VNNI operands or bf16x6, m = the transpose's n, k = its m, lda = its ldo, m and k at most 64, B, C
 *    and the bias off the destination, C off the transpose's source, not in strict mode. It reads A transposed from the SOURCE;
 *    the remembered transpose stays and is replaced or launched exactly as for B. Such a gemm pays the full (not the inlined) host path;
 *  - a folded gemm reads its operands with 16-byte loads when every A and B pointer of its group is 16-byte aligned, k, lda, ldb,
 *    stride_a and stride_b are multiples of 4, lda and ldb are below 2^24 and, for a transposed A, m and n are multiples of 4;
 *    otherwise element by element. The same bits either way, and for B the bits of mode 1.
 *  xsmm_hip_last_grouped_kernel names the path: "brgemm_grouped<f32,v4>, B read transposed", "brgemm_grouped<f32,v4>, A read
 *  transposed", "brgemm_grouped<f32>, A read transposed"; "brgemm_grouped<f32>, B read transposed" is the element path of B and the
 *  only name mode 1 reports.
 * Returns the previous mode (0, 1 or 2); any other value is refused with -1 and changes nothing.
 * stats: [0] gemm invokes served from a transpose's source (through B or A), [1] remembered transposes dropped as dead, [2] launched after all.
 *  Between a transpose invoke and the gemm invoke that consumes its temporary, no OTHER thread may write the transpose's
 * source: the folded gemm reads the source when it is enqueued, not when the transpose was invoked. */
TPP_XSMM_EXPORT int xsmm_hip_set_fold_transpose(int mode);
/* Epilogue fold (TPP_HIP_FOLD_EPILOGUE=0|1, default 1; tile queue + asynchronous mode, device operands only). The compiler fuses a
 * gemm tile with its element-wise epilogue only as brgemm + binary add bcast_col + unary relu (CombineXsmmOp); every other epilogue -
 * a bias alone, a relu alone, a residual add, a scale, other broadcasts - reaches the runtime as a gemm invoke followed by one or two
 * element-wise invokes on that tile's output. A binary add / mul / sub / div (any broadcast of its OTHER operand, the tile in either
 * position) or a unary identity / relu / zero without flags, on the same stream and dtype, whose input is exactly the latest value of
 * one queued GEMM item (same address, leading dimension and m x n, no broadcast) joins that item's group as the next stage of its
 * chain instead of flushing the group: at most two stages per item, stage s of every item the same handle in the same position, the
 * other operand written by nothing queued, the output either the tile itself (in place) or touching nothing the group reads or writes.
 * The group then runs as its GEMM launch plus ONE epilogue-program launch for all of its post-ops, and a recorded group replays that
 * way. Every stage rounds at its own store with the element-wise op's own arithmetic: the same bits as the unfolded invokes (on in
 * strict mode too). Anything else flushes as before. set returns the previous setting (with 0, recorded folded groups are no longer replayed);
 * stats: [0] post-op invokes folded, [1] epilogue-program launches, [2] element-wise invokes on a queued GEMM group that flushed it
 * because they were not eligible.
 * Between a post-op invoke and the next synchronisation point (xsmm_hip_flush, a synchronize, leaving asynchronous mode) no OTHER
 * thread may write the post-op's second operand (bias, residual, scale): the epilogue reads it when the group is launched, not when
 * the post-op was invoked. */
TPP_XSMM_EXPORT int xsmm_hip_set_fold_epilogue(int enable);
TPP_XSMM_EXPORT void xsmm_hip_fold_epilogue_stats(int64_t out[3]);
/* Relayout grids (TPP_HIP_RELAYOUT_GRID=0|1, default 1; tile queue + asynchronous mode only). A recorded queue group of ONE unary
 * identity (f32 / bf16) or VNNI-2 (bf16) handle without broadcast flags - the per-block invokes a tensor.pack / unpack lowers to -
 * whose items form at most 16 affine block grids, each writing one dense range, with pairwise disjoint input extents, is launched on every
 * complete replay as ONE relayout-grid launch (16-byte accesses where bases and strides allow) instead of one workgroup per invoke;
 * xsmm_hip_last_grouped_kernel then reads "relayout grid: ...". The result is the same bits (a copy of raw words: on in strict mode
 * too). Any other group runs as before. set returns the previous setting; stats: [0] relayout grid launches, [1] the invokes they
 * covered. */
TPP_XSMM_EXPORT int xsmm_hip_set_relayout_grid(int enable);
TPP_XSMM_EXPORT void xsmm_hip_relayout_grid_stats(int64_t out[2]);
TPP_XSMM_EXPORT void xsmm_hip_fold_transpose_stats(int64_t out[3]);
/* The VNNI blocking factor v of bf16 B operands ([k/v][ldb][v]) of gemm / brgemm / fused_brgemm handles dispatched FROM NOW ON with
 * the VNNI_B wire flag: 2 (default) or 4; also TPP_HIP_VNNI_FACTOR. The factor is not on the wire - the reference's compiler and its
 * runtime library both ask libxsmm_cpuid_dot_pack_factor(LIBXSMM_DATATYPE_BF16) (lib/TPP/Transforms/Utils/VNNIUtils.cpp:25-45; the
 * `--vnni=4` rows of benchmarks/config/omp/mlir-bf16.json:68-100): a harness that lowers with vnni = 4 sets 4 here before it
 * dispatches. k must then be a multiple of 4 (dispatch dies otherwise); ldb is the k-group row stride / v as the compiler passes it
 * (ConvertLinalgToXsmm.cpp:1144). xsmm.unary VNNI2 (kind 28) always packs pairs - there is no VNNI-4 pack kind at this revision
 * (XsmmEnum.td:34-45). set returns the previous factor, -1 for an invalid one. The setting is process-wide and read once per
 * dispatch: set it BEFORE dispatching (a handle keeps the factor it was dispatched with); a VNNI A operand (wire flag 4096) is
 * checked against the same factor (k a multiple of it; [m][k/v][v] is byte-identical to the flat row). */
TPP_XSMM_EXPORT int xsmm_hip_set_vnni_factor(int factor);
TPP_XSMM_EXPORT int xsmm_hip_get_vnni_factor(void);
/* f32 GEMM arithmetic of descriptors dispatched from now on: 0 = exact f32 MFMA (default), 6 = bf16x6 split. Read once per
 * dispatch and kept by the handle (part of the descriptor key). Returns the previous setting; other values are refused (-1).
 * Also TPP_HIP_F32_PRECISION=bf16x6 (or 6). bf16x6 writes every f32 operand as hi + mid + lo, three bf16 parts rounded to nearest
 * even one after another (about 2^-27 relative left over), and sums the six part products down to 2^-18 relative (hi.hi, hi.mid,
 * mid.hi, hi.lo, lo.hi, mid.mid) on the bf16 MFMA in its f32 accumulator: the dropped terms are about 2^-26 relative, below the f32
 * rounding of the sum. The first split kernel measured SLOWER than the exact one on every shape (profiles/x6_first_ab.txt), so it runs
 * only where a split tile is also forced (xsmm_hip_force_variant 12 = 64x64, 13 = 64x32, 14 = 32x32, 15 = 128x64) and the shape fits
 * (k a multiple of 64, m / n multiples of the tile, leading dimensions and strides multiples of 4); every other bf16x6 descriptor runs
 * on the exact kernel it gets under 0. The kernel name (xsmm_hip_kernel_name) contains "bf16x6" only where the split kernel runs. bf16
 * descriptors ignore the setting. A bf16x6 handle is never grouped by the tile queue or chained (xsmm_hip_fused_brgemm_chain_invoke
 * runs a chain holding one call by call). */
TPP_XSMM_EXPORT int xsmm_hip_set_f32_precision(int mode);
TPP_XSMM_EXPORT int xsmm_hip_get_f32_precision(void);
/* Library version string. */
TPP_XSMM_EXPORT const char *xsmm_hip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* TPP_XSMM_ABI_H */
