// rt_rewrites.h - run-time rewrites of call sequences: GRID MERGE (a recorded tile grid over flat operands -> one launch) and DEFERRED TRANSPOSES (a transpose folded into the gemm it feeds)
// One of the subsystem units of runtime.cpp (round 6, VERDICT r5 next 7: the 3 000-line file split by subsystem, no behaviour
// change). The units are INCLUDED into the one translation unit runtime.cpp, in dependence order, inside its anonymous namespace:
// the per-invoke host path (14-18 ns: enqueue_item -> join_window -> Segment::mark) crosses four of them and is inlined across
// their borders - as separate objects without LTO it would pay a call per border. Not a stand-alone header: include runtime.cpp's way only.

// GRID MERGE (round 5). The compiler tiles a contraction over FLAT operands into one gemm invoke per output tile (the mha projection,
// benchmarks/mlir/fp32-projection.mlir: 64 x 8 invokes of [32,64,512,512,512,512] = one 2048 x 512 x 512 problem with lda = ldb = ldc =
// 512). When a recorded group is exactly such a grid - every item the same f32 descriptor and batch count, A a function of the tile row
// only (A0 + r m lda), B of the tile column only (B0 + c n, all columns inside one row of B: cols n <= ldb), C = C0 + r m ldc + c n, the
// bias D0 + c n, every (r, c) once - a complete replay of it is launched as ONE invoke of the merged problem (rows m, cols n) on the
// kernel plan_gemm picks for THAT shape (64x64 tiles instead of 1024 workgroups of 32x32 with 8 chunks each: 13.0 -> ~10.5 us). Same
// reads, same writes, the same sums per element in a different (fixed) order: like every kernel choice that depends on the group.
// Packed block layouts (mlir-gen's tiles) are never grids: their B tiles are not columns of one row.
static bool grid_merge_on() {
  return !cfg().strict.load(std::memory_order_relaxed); // (a merged grid sums in the merged problem's order: not in strict mode)
}
std::atomic<const char *> g_last_merged{nullptr}; // trace text of the merged descriptor if the most recent group launch was a merged one
inline void detect_grid(Segment &S) {
  S.grid_state = -1;
  const size_t n = S.items.size();
  if (!grid_merge_on() || n < 4) return;
  const void *desc = S.items[0].desc;
  if (*(const int *)desc != KIND_GEMM) return;
  const GemmDesc *d = (const GemmDesc *)desc;
  if (d->dtype != DT_F32 || d->vnni_b || d->vnni_c || d->b_trans || d->a_trans || d->generic_forced || d->variant_forced || d->m <= 0 || d->n <= 0 || d->k <= 0) return;
  const int64_t br = S.items[0].w.br;
  std::vector<uintptr_t> ua, ub;
  ua.reserve(n);
  ub.reserve(n);
  for (const TraceItem &t : S.items) {
    if (t.desc != desc || t.w.br != br || t.stream != S.items[0].stream) return;
    ua.push_back((uintptr_t)t.w.A);
    ub.push_back((uintptr_t)t.w.B);
  }
  std::sort(ua.begin(), ua.end());
  ua.erase(std::unique(ua.begin(), ua.end()), ua.end());
  std::sort(ub.begin(), ub.end());
  ub.erase(std::unique(ub.begin(), ub.end()), ub.end());
  const size_t R = ua.size(), Cn = ub.size();
  if (R * Cn != n || br < 1) return;
  const uintptr_t sa = (uintptr_t)d->m * (uintptr_t)d->lda * 4, sb = (uintptr_t)d->n * 4;
  for (size_t r = 0; r < R; ++r)
    if (ua[r] != ua[0] + r * sa) return;
  for (size_t c = 0; c < Cn; ++c)
    if (ub[c] != ub[0] + c * sb) return;
  if ((int64_t)Cn * d->n > d->ldb || (int64_t)Cn * d->n > d->ldc) return;
  uintptr_t c0 = 0, d0 = 0;
  for (const TraceItem &t : S.items)
    if ((uintptr_t)t.w.A == ua[0] && (uintptr_t)t.w.B == ub[0]) c0 = (uintptr_t)t.w.C, d0 = (uintptr_t)t.w.D;
  if (!c0) return;
  std::vector<char> seen(n, 0);
  for (const TraceItem &t : S.items) {
    const size_t r = ((uintptr_t)t.w.A - ua[0]) / sa, c = ((uintptr_t)t.w.B - ub[0]) / sb;
    if ((uintptr_t)t.w.C != c0 + ((uintptr_t)r * d->m * d->ldc + (uintptr_t)c * d->n) * 4) return;
    if (d->bias && (uintptr_t)t.w.D != d0 + (uintptr_t)c * d->n * 4) return;
    if (seen[r * Cn + c]++) return;
  }
  const int64_t M = (int64_t)R * d->m, N = (int64_t)Cn * d->n;
  std::vector<int64_t> key = {KIND_GEMM, -31, (int64_t)(uintptr_t)d, M, N};
  bool ok = true;
  const GemmDesc *e = (const GemmDesc *)intern(key, [&]() {
    GemmDesc *g = new GemmDesc(*d);
    g->m = M;
    g->n = N;
    g->f32_prec = 0; // the tiles ran on exact kernels (a split-kernel handle is never queued): so does the merged grid
    ok = plan_gemm(*g, -1);
    snprintf(g->trace, sizeof(g->trace), "tile grid %zu x %zu of gemm[%ld,%ld,%ld] merged -> [%ld,%ld,%ld,%ld,%ld,%ld] %s", R, Cn, (long)d->m, (long)d->n,
             (long)d->k, (long)M, (long)N, (long)d->k, (long)d->lda, (long)d->ldb, (long)d->ldc, g->name);
    return (void *)g;
  });
  if (!ok || e->variant == V_GENERIC) return; // (no fast tile for the merged shape: the grouped launch stays)
  S.grid_desc = e;
  S.grid_w = WorkItem{(const void *)ua[0], (const void *)ub[0], (void *)c0, d->bias ? (const void *)d0 : nullptr, br};
  S.grid_state = 1;
}

// QUADS (round 6). mlir-gen tiles a bf16 layer into 64x64x64 invokes over PACKED blocks (A [MB][KB][64][64], B VNNI [NB][KB][..]): never
// a tile grid over flat operands (no grid merge), and as items the group runs on 64x64 tiles - three rounds of workgroups for
// benchmarks/config/fc/1024x2560x1024.json (15.3 us) where the same layer as one call runs on 128x128 tiles in one round (10.2 us).
// When a recorded group is such a grid - one bf16 descriptor and batch count, every item = (item row r, item column c) with A a
// function of r only, B and the bias of c only, every (r, c) once, R and C even - and the tile model prefers it (gemm_quads_pay), a
// complete replay is launched as R C / 4 blocks of 2 x 2 items on the 128x128 loader-wave tile: rows 64 .. 127 of a block's A panel
// come from the lower item row's block, columns 64 .. 127 of its B panel from the right item column's block (two byte distances per
// block: same allocation, ascending, below 2 GiB), each of its four 64x64 outputs goes to its own item's C. Same reads, same
// writes, the same k order per element. Not in strict mode (the kernel would depend on the group), not while the stream is captured.
inline void detect_quads(Segment &S, hipStream_t stream) {
  S.quad_state = -1;
  const size_t n = S.items.size();
  if (n < 4 || (n & 3) || cfg().strict.load(std::memory_order_relaxed)) return;
  const void *desc = S.items[0].desc;
  if (*(const int *)desc != KIND_GEMM) return;
  const GemmDesc *d = (const GemmDesc *)desc;
  const int64_t br = S.items[0].w.br;
  if (!S.vec_ok || !S.out_ok || !gemm_quads_pay(*d, (int)n, br)) return;
  std::vector<uintptr_t> ua, ub;
  ua.reserve(n);
  ub.reserve(n);
  for (const TraceItem &t : S.items) {
    if (t.desc != desc || t.w.br != br || t.stream != S.items[0].stream) return;
    if ((((uintptr_t)t.w.A | (uintptr_t)t.w.B | (uintptr_t)t.w.C) & 15) || ((uintptr_t)t.w.D & 7)) return;
    ua.push_back((uintptr_t)t.w.A);
    ub.push_back((uintptr_t)t.w.B);
  }
  std::sort(ua.begin(), ua.end());
  ua.erase(std::unique(ua.begin(), ua.end()), ua.end());
  std::sort(ub.begin(), ub.end());
  ub.erase(std::unique(ub.begin(), ub.end()), ub.end());
  const size_t R = ua.size(), Cn = ub.size();
  if (R * Cn != n || (R & 1) || (Cn & 1)) return;
  // (r, c) -> item; the bias is the column's
  std::vector<int> at(n, -1);
  std::vector<uintptr_t> dcol(Cn, 0);
  for (size_t i = 0; i < n; ++i) {
    const TraceItem &t = S.items[i];
    const size_t r = (size_t)(std::lower_bound(ua.begin(), ua.end(), (uintptr_t)t.w.A) - ua.begin());
    const size_t c = (size_t)(std::lower_bound(ub.begin(), ub.end(), (uintptr_t)t.w.B) - ub.begin());
    if (at[r * Cn + c] >= 0) return;
    at[r * Cn + c] = (int)i;
    if (r == 0) dcol[c] = (uintptr_t)t.w.D;
  }
  for (size_t r = 0; r < R; ++r)
    for (size_t c = 0; c < Cn; ++c)
      if (d->bias && (uintptr_t)S.items[at[r * Cn + c]].w.D != dcol[c]) return;
  const uint64_t a_rows = (uint64_t)64 * (uint64_t)d->lda * 2; // bytes the instruction offsets of rows 64 .. 127 already cover
  const uint64_t lim = (uint64_t)1 << 30;                      // (buffer offsets are 32 bits against a 2 GiB range: distance + panel below that)
  for (size_t r = 0; r < R; r += 2)
    if (ua[r + 1] - ua[r] < a_rows || ua[r + 1] - ua[r] >= lim) return;
  for (size_t c = 0; c < Cn; c += 2)
    if (ub[c + 1] - ub[c] >= lim) return;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &cs) != hipSuccess) (void)hipGetLastError();
  else if (cs != hipStreamCaptureStatusNone) {
    S.quad_state = 0; // (not now: look again at the next complete replay)
    return;
  }
  const size_t nq = n / 4;
  if (S.quad_used) { // the buffers carried another recording's blocks: its last launch must be done (and, first, issued)
    launcher_drain();
    HIP_OK(hipStreamSynchronize(S.quad_stream));
    S.quad_used = false;
  }
  if (S.quad_cap < nq) {
    if (S.quad_host) HIP_OK(hipHostFree(S.quad_host));
    if (S.quad_dev) HIP_OK(hipFree(S.quad_dev));
    S.quad_cap = nq < 256 ? 256 : nq;
    HIP_OK(hipHostMalloc((void **)&S.quad_host, sizeof(QuadItem) * S.quad_cap, hipHostMallocDefault));
    HIP_OK(hipMalloc((void **)&S.quad_dev, sizeof(QuadItem) * S.quad_cap));
  }
  size_t k = 0;
  for (size_t r = 0; r < R; r += 2)
    for (size_t c = 0; c < Cn; c += 2) {
      QuadItem &q = S.quad_host[k++];
      const WorkItem &w00 = S.items[at[r * Cn + c]].w, &w01 = S.items[at[r * Cn + c + 1]].w, &w10 = S.items[at[(r + 1) * Cn + c]].w,
                     &w11 = S.items[at[(r + 1) * Cn + c + 1]].w;
      q.A = w00.A;
      q.B = w00.B;
      q.C[0] = w00.C, q.C[1] = w01.C, q.C[2] = w10.C, q.C[3] = w11.C;
      q.D[0] = w00.D, q.D[1] = w01.D;
      q.br = br;
      q.da = (uint32_t)(ua[r + 1] - ua[r] - a_rows);
      q.db = (uint32_t)(ub[c + 1] - ub[c]);
    }
  HIP_OK(hipMemcpyAsync(S.quad_dev, S.quad_host, sizeof(QuadItem) * nq, hipMemcpyHostToDevice, stream));
  S.quad_used = true; // (the copy reads quad_host)
  S.quad_stream = stream;
  S.n_quads = (int)nq;
  S.quad_state = 1;
}

// RELAYOUT GRIDS (rt_relayout.h says what qualifies and why). Called once per recording at its first complete replay, like
// detect_quads: the run table is uploaded then (not while the stream is captured - look again at the next replay) and every later
// complete replay launches from it. Stays on in strict mode (a copy's bits do not depend on the kernel).
static bool relayout_grid_on() { return cfg().relayout_grid.load(std::memory_order_relaxed) != 0; }
// the launch's text for xsmm_hip_last_grouped_kernel: interned, so that a reader never sees a segment's buffer being rewritten
static const char *intern_text(const char *s) {
  static std::mutex mu;
  static std::unordered_map<std::string, int> texts; // (node-based: a key's characters never move)
  std::lock_guard<std::mutex> lk(mu);
  return texts.emplace(s, 0).first->first.c_str();
}
inline void detect_relayout(Segment &S, hipStream_t stream) {
  S.rl_state = -1;
  const size_t n = S.items.size();
  const void *desc = S.items[0].desc;
  if (n < 2 || *(const int *)desc != KIND_UNARY || !launch_relayout_grid) return; // (null: a host-only test build)
  const UnaryDesc *d = (const UnaryDesc *)desc;
  const bool f32 = d->dtype == DT_F32;
  if (d->flags != 0 || d->m > 64 || d->n > 64 || !(d->op == XSMM_UNARY_IDENTITY || (d->op == XSMM_UNARY_VNNI2 && !f32))) return;
  std::vector<RelayoutItem> io;
  io.reserve(n);
  for (const TraceItem &t : S.items) {
    if (t.desc != desc || t.stream != S.items[0].stream || !t.w.A || !t.w.C) return;
    io.push_back(RelayoutItem{(uintptr_t)t.w.A, (uintptr_t)t.w.C});
  }
  RelayoutRun runs[RELAYOUT_MAX_RUNS];
  const int nr = relayout_decompose(d->op, f32 ? 4 : 2, d->m, d->n, d->ldi, d->ldo, std::move(io), runs, RELAYOUT_MAX_RUNS);
  if (nr <= 0) return;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &cs) != hipSuccess) (void)hipGetLastError();
  else if (cs != hipStreamCaptureStatusNone) {
    S.rl_state = 0; // (not now: look again at the next complete replay)
    return;
  }
  int wg = 0; // one workgroup per block
  for (int k = 0; k < nr; ++k) {
    runs[k].wg0 = wg;
    wg += runs[k].R * runs[k].C;
  }
  if (S.rl_used) { // the table carried another recording's runs: its last launch must be done (and, first, issued)
    launcher_drain();
    HIP_OK(hipStreamSynchronize(S.rl_stream));
    S.rl_used = false;
  }
  if (!S.rl_host) {
    HIP_OK(hipHostMalloc((void **)&S.rl_host, sizeof(RelayoutRun) * RELAYOUT_MAX_RUNS, hipHostMallocDefault));
    HIP_OK(hipMalloc((void **)&S.rl_dev, sizeof(RelayoutRun) * RELAYOUT_MAX_RUNS));
  }
  std::copy(runs, runs + nr, S.rl_host);
  HIP_OK(hipMemcpyAsync(S.rl_dev, S.rl_host, sizeof(RelayoutRun) * nr, hipMemcpyHostToDevice, stream));
  S.rl_used = true; // (the copy reads rl_host)
  S.rl_stream = stream;
  int vec = 0;
  for (int k = 0; k < nr; ++k) vec += runs[k].vec;
  char text[160];
  snprintf(text, sizeof(text), "relayout grid: %d run%s, %zu blocks of %ldx%ld, %s %s, %d of them 16-byte", nr, nr == 1 ? "" : "s", n, (long)d->m, (long)d->n,
           d->op == XSMM_UNARY_VNNI2 ? "vnni2" : "identity", f32 ? "f32" : "bf16", vec);
  S.rl_trace = intern_text(text);
  S.rl_runs = nr;
  S.rl_wg = wg;
  S.rl_state = 1;
}

// ---- deferred transposes (round 5) ------------------------------------------------------------------------------------
// A contraction whose B operand is transposed in memory reaches the runtime as TWO invokes per tile: xsmm.unary transpose into a
// small temporary, then xsmm.gemm reading it (ConvertLinalgToXsmm; test/Conversion/LinalgToXsmm/linalg-to-gemm.mlir:46-62 has the
// query-times-key benchmark lowered exactly so: transpose [32,64,512,32] + gemm [32,32,64,512,32,32] per (batch, head), ONE
// temporary for every tile of a caller). Through the tile queue that is a chain of true and anti dependences on the temporary:
// every invoke its own launch (1024 launches for benchmarks/mlir/fp32-query-times-key.mlir, 3.6 ms; the queue cannot help).
// So a transpose of a small tile into a DENSE destination (ldo = m) is not launched when it is invoked but REMEMBERED - one record
// per calling thread (the reference's OpenMP callers own a temporary each) - and
//   * a gemm of the same thread whose B operand is exactly that destination (k = the transpose's n, n = its m, ldb = ldo, one batch
//     element, f32, no operand of it overlapping the destination, C not overlapping the transpose's source) runs on a SIBLING
//     descriptor that reads B transposed straight from the transpose's source (GemmDesc::b_trans - the generic kernel). All such
//     gemms of a loop, of every thread, share that sibling: the queue groups them into one launch;
//   * a second transpose of the same thread, the same descriptor and the same destination REPLACES the record: the remembered one is
//     dead - fully overwritten, and its only readers were served from its source;
//   * any other invoke of the owning thread launches the remembered transpose first, the ordinary way (dt_launch); an invoke of
//     ANOTHER thread does so if one of its operands overlaps the record's destination, or if it writes into the record's source (a
//     race-free program orders such an invoke behind the transpose's invoke: it then sees the record); a flush and every
//     synchronisation point launch every record - the destination holds what the program wrote whenever anything can look at it.
// Between a transpose's invoke and its launch only folded gemms of its own thread and invokes that touch neither its destination
// nor (writing) its source run: the deferred launch reads what the immediate one would have read.
// Summation order of a folded gemm = the generic kernel's (what a single invoke of the same gemm on the generic kernel adds).
// MODE 2 (xsmm_hip_set_fold_transpose(2) / TPP_HIP_FOLD_TRANSPOSE=2, opt-in): the siblings are made under mode 2 - the planner may run
// them on the 16-byte instances of the generic kernel (gemm_plan.cpp trans_launch), the same bits - and a gemm of the owning thread whose
// A operand is exactly the destination (ConvertLinalgToXsmm.cpp:797-805 "emit transpose for A": m = the transpose's n, k = its m,
// lda = ldo, B not the destination, one batch element, f32, m and k at most 64, B / C / bias off the destination, C off the source)
// folds the same way, on a sibling that reads A transposed (GemmDesc::a_trans, lda = the source's). The record stays, and everything
// said above about replacement, launches and the other threads holds for it unchanged. A gemm whose A is the temporary never takes
// the inlined fast path (dt_gemm_fast knows B folds only): its host cost per invoke is dt_gemm's.
struct DeferredTranspose {
  const UnaryDesc *d = nullptr;
  void *src = nullptr, *dst = nullptr;
  hipStream_t stream = nullptr;
  const GemmDesc *sib_of = nullptr, *sib = nullptr; // the last gemm descriptor folded and its sibling
  size_t a_bytes = 0, c_bytes = 0, d_bytes = 0;     // ... and the footprints of that descriptor's A / C / bias operands (sib_of != nullptr)
  // the owner's fast path (dt_defer_fast): the device allocation the record's sources have been seen in, validated in this
  // synchronisation epoch by the full path (0: not); a source inside it needs no further look at the allocation table
  uintptr_t src_alloc_b = 0, src_alloc_e = 0;
  uint64_t valid_epoch = 0;
  // mode 2, the last gemm descriptor folded through its A operand, apart from sib_of (dt_gemm_fast serves B folds only and must never
  // meet an A sibling): its sibling and the footprints of its B / C / bias operands
  const GemmDesc *asib_of = nullptr, *asib = nullptr;
  size_t ab_bytes = 0, ac_bytes = 0, ad_bytes = 0;
};
struct alignas(64) DtSlot {
  // line 0 - what EVERY thread reads per invoke while records exist; written when a record appears or goes, not per tile:
  std::atomic<uintptr_t> owner{0};   // thread_token() of the thread that owns the slot (0: free)
  std::atomic<int> live{0};          // a record is remembered
  // the record's destination, and the hull of the sources it has had (the source changes with every tile of a loop - the next
  // transpose replaces the record -, the hull stops growing after one pass: eight callers that each rewrote a line the seven others
  // read per invoke took 2.5 us per tile). For the other threads' overlap test: written under mu before live = 1 (release), read after live
  // (acquire). A reader that races with a replacement may see either record's source range - both belong to invokes it is not ordered with.
  std::atomic<uintptr_t> d_lo{0}, d_hi{0}, s_lo{0}, s_hi{0};
  // line 1 - the owner's (and, rarely, of a thread that launches the record):
  alignas(64) SpinLock mu;           // the record and its hand-over: every thread but the owner, and the owner when `contended`
  DeferredTranspose r;               // under mu / inside an owner section
  std::atomic<int64_t> folded{0}, dropped{0}; // statistics (the owner's relaxed adds)
  // OWNER SECTIONS (round 6): the owner touches its record twice per tile (the transpose replaces it, the gemm folds into it) and an
  // uncontended spin lock was two locked exchanges of the ~35 ns that pair costs. The owner now brackets its section with oseq (odd
  // inside; plain stores) and looks at `contended`; any OTHER thread that wants the record takes mu, sets contended, issues
  // membarrier(PRIVATE_EXPEDITED) - a full barrier at a precise point of the owner's instruction stream - and waits for an even oseq:
  // either the owner's oseq store had retired when the barrier landed (the other thread waits for the section to end) or the owner's
  // load of `contended` had not retired either and sees 1 (the owner takes mu like everybody else). The same pair as the direct
  // window's SOLO sections (rt_tile_queue.h), per slot and reversible. Other threads want a record at flush points and on a real
  // overlap only. No membarrier: the owner locks as before.
  std::atomic<uint64_t> oseq{0};
  std::atomic<int> contended{0};
};
struct DtOwnerSection { // the calling thread OWNS the slot
  DtSlot &sl;
  bool locked = true;
  __attribute__((always_inline)) explicit DtOwnerSection(DtSlot &s) : sl(s) {
    if (membarrier_ok()) {
      const uint64_t q = sl.oseq.load(std::memory_order_relaxed);
      sl.oseq.store(q + 1, std::memory_order_relaxed);
      std::atomic_signal_fence(std::memory_order_seq_cst); // (the compiler keeps the order; the other side's membarrier makes it hold)
      if (!sl.contended.load(std::memory_order_acquire)) {
        locked = false;
        return;
      }
      sl.oseq.store(q + 2, std::memory_order_release);
    }
    sl.mu.lock();
  }
  __attribute__((always_inline)) ~DtOwnerSection() {
    if (locked) {
      sl.mu.unlock();
      return;
    }
    std::atomic_signal_fence(std::memory_order_seq_cst);
    sl.oseq.store(sl.oseq.load(std::memory_order_relaxed) + 1, std::memory_order_release);
  }
};
struct DtForeignSection { // any other thread (or nobody's slot)
  DtSlot &sl;
  explicit DtForeignSection(DtSlot &s) : sl(s) {
    sl.mu.lock();
    if (membarrier_ok()) {
      sl.contended.store(1, std::memory_order_seq_cst);
      if (syscall(__NR_membarrier, MEMBARRIER_CMD_PRIVATE_EXPEDITED, 0) != 0) die("tpp-xsmm-hip: membarrier failed");
      while (sl.oseq.load(std::memory_order_acquire) & 1) cpu_relax();
    }
  }
  ~DtForeignSection() {
    sl.contended.store(0, std::memory_order_release);
    sl.mu.unlock();
  }
};
constexpr int DT_SLOTS = 64;
DtSlot g_dt_slots[DT_SLOTS];
std::atomic<int> g_dt_top{0}; // slots [0, top) have been claimed at some time
std::atomic<int64_t> g_dt_launched{0}; // statistics (xsmm_hip_fold_transpose_stats; folded / dropped: per slot)
static __thread bool tl_dt_busy = false; // this thread is inside dt_launch's hand-over (its own flush_tile_queue calls must not re-enter)
void unary_invoke_core(const UnaryDesc *d, void *pi, float scalar, bool use_scalar, void *po, bool may_defer);
// Launches the slot's remembered transpose, if there is one (any thread). The record stays live until the transpose HAS BEEN handed to
// the queue / launched, and the lock is held across that: a thread that then sees live = 0 (and goes on to queue an invoke that reads
// the destination) is ordered behind the transpose.
void dt_launch_locked(DtSlot &sl) { // inside a section of the slot
  if (!sl.live.load(std::memory_order_relaxed)) return;
  const DeferredTranspose r = sl.r;
  g_dt_launched.fetch_add(1, std::memory_order_relaxed);
  if (cfg().stream.load(std::memory_order_relaxed) != r.stream) die("tpp-xsmm-hip: a deferred transpose outlived its stream"); // (xsmm_hip_set_stream flushes first)
  tl_dt_busy = true;
  unary_invoke_core(r.d, r.src, 0.0f, false, r.dst, false);
  tl_dt_busy = false;
  sl.live.store(0, std::memory_order_release);
  g_dt_pending.fetch_sub(1, std::memory_order_release);
}
void dt_launch(DtSlot &sl) {
  if (tl_dt_busy) return;
  if (sl.owner.load(std::memory_order_relaxed) == thread_token()) {
    DtOwnerSection sec(sl);
    dt_launch_locked(sl);
  } else {
    DtForeignSection sec(sl);
    dt_launch_locked(sl);
  }
}
void dt_materialize() { // every record (flush, synchronisation points)
  if (tl_dt_busy) return;
  const int top = g_dt_top.load(std::memory_order_acquire);
  for (int i = 0; i < top; ++i)
    if (g_dt_slots[i].live.load(std::memory_order_acquire)) dt_launch(g_dt_slots[i]);
}
struct DtRange {
  uintptr_t lo, hi;
};
inline DtRange dt_range(const void *p, size_t bytes) { return DtRange{(uintptr_t)p, p ? (uintptr_t)p + bytes : 0}; }
inline bool dt_overlap(const void *a, size_t na, const void *b, size_t nb) {
  return a && b && na && nb && (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
}
// the records of OTHER threads that this invoke (reads rd[0..nr), writes wr[0..nw)) must see launched
void dt_scan_foreign(const DtSlot *mine, const DtRange *rd, int nr, const DtRange *wr, int nw) {
  const int top = g_dt_top.load(std::memory_order_acquire);
  for (int i = 0; i < top; ++i) {
    DtSlot &sl = g_dt_slots[i];
    if (&sl == mine || !sl.live.load(std::memory_order_acquire)) continue;
    const uintptr_t dl = sl.d_lo.load(std::memory_order_relaxed), dh = sl.d_hi.load(std::memory_order_relaxed);
    const uintptr_t slo = sl.s_lo.load(std::memory_order_relaxed), shi = sl.s_hi.load(std::memory_order_relaxed);
    bool hit = false;
    for (int k = 0; k < nr && !hit; ++k) hit = rd[k].lo < dh && dl < rd[k].hi;
    for (int k = 0; k < nw && !hit; ++k) hit = (wr[k].lo < dh && dl < wr[k].hi) || (wr[k].lo < shi && slo < wr[k].hi);
    if (hit) dt_launch(sl);
  }
}
// the owning thread ends: the slot is free for another thread once its record (if any) has been launched by a flush
void dt_release_slot(int slot) { g_dt_slots[slot].owner.store(0, std::memory_order_release); }
DtSlot *dt_my_slot(bool claim) {
  CallerState &tl = caller_state();
  if (tl.dt_slot >= 0) return &g_dt_slots[tl.dt_slot];
  if (!claim) return nullptr;
  const uintptr_t me = thread_token();
  for (int i = 0; i < DT_SLOTS; ++i) {
    DtSlot &sl = g_dt_slots[i];
    uintptr_t none = 0;
    if (sl.owner.load(std::memory_order_relaxed) == 0 && !sl.live.load(std::memory_order_acquire) && sl.owner.compare_exchange_strong(none, me)) {
      int top = g_dt_top.load(std::memory_order_relaxed);
      while (top < i + 1 && !g_dt_top.compare_exchange_weak(top, i + 1, std::memory_order_release)) {
      }
      tl.dt_slot = i;
      return &sl;
    }
  }
  return nullptr; // more transposing threads than slots: this one's transposes are launched as they come
}
// keyed by (descriptor, source ld, operand, mode); the mode-1 siblings (B only) keep the key they have always had
const GemmDesc *dt_sibling(const GemmDesc *d, int64_t ld_src, bool a_operand = false, int mode = 1) {
  std::vector<int64_t> key = {KIND_GEMM, -29, (int64_t)(uintptr_t)d, ld_src};
  if (a_operand || mode != 1) key.push_back(a_operand), key.push_back(mode);
  return (const GemmDesc *)intern(key, [&]() {
    GemmDesc *e = new GemmDesc(*d);
    e->b_trans = !a_operand;
    e->a_trans = a_operand;
    e->trans_mode = mode;
    (a_operand ? e->lda : e->ldb) = ld_src;
    e->variant = V_GENERIC;
    e->generic_forced = 1;
    snprintf(e->name, sizeof(e->name), "brgemm_grouped(generic), %c read transposed", a_operand ? 'A' : 'B');
    if (a_operand)
      snprintf(e->trace, sizeof(e->trace), "gemm[%ld,%ld,%ld,(%ld)^T,%ld,%ld] dt%ld flags%ld %s (transpose folded)", (long)d->m, (long)d->n, (long)d->k,
               (long)ld_src, (long)d->ldb, (long)d->ldc, (long)d->dtype, (long)d->wire_flags, e->name);
    else
      snprintf(e->trace, sizeof(e->trace), "gemm[%ld,%ld,%ld,%ld,(%ld)^T,%ld] dt%ld flags%ld %s (transpose folded)", (long)d->m, (long)d->n, (long)d->k,
               (long)d->lda, (long)ld_src, (long)d->ldc, (long)d->dtype, (long)d->wire_flags, e->name);
    return (void *)e;
  });
}
// a gemm invoke while transposes are remembered: the sibling descriptor + the transpose's source if it folds into this thread's record
// (which stays), else nullptr - this thread's record, and every other thread's record the gemm's operands touch, launched first.
// *a_operand: the source replaces the gemm's A (mode 2), not its B
const GemmDesc *dt_gemm(const GemmDesc *d, void *pa, void *pb, void *pc, void *pd, int64_t br, hipStream_t s, void **src, bool *a_operand) {
  *a_operand = false;
  const int mode = cfg().fold_transpose.load(std::memory_order_relaxed);
  const size_t es = esize(d->dtype);
  DtSlot *mine = dt_my_slot(false);
  const GemmDesc *sib = nullptr;
  if (mine && mine->live.load(std::memory_order_acquire)) {
    {
      DtOwnerSection sec(*mine);
      if (mine->live.load(std::memory_order_relaxed)) {
        DeferredTranspose &r = mine->r;
        const UnaryDesc *t = r.d;
        const size_t dst_bytes = (size_t)t->n * t->m * 4, src_bytes = span(t->m, t->ldi, t->n) * 4;
        // (the descriptor-level conditions and footprints were established when this descriptor was folded into this record last: the
        // record keeps its transpose descriptor for as long as it lives)
        const bool known = r.sib_of == d;
        if (pb == r.dst && br == 1 && s == r.stream && queue_active() &&
            (known || (d->dtype == DT_F32 && !gemm_on_x6(*d) && !d->vnni_b && !d->vnni_c && !d->b_trans && d->k == t->n && d->n == t->m && d->ldb == t->ldo && d->m <= 64 && d->n <= 64))) {
          const size_t a_bytes = known ? r.a_bytes : span(d->m, d->lda, d->k) * 4, c_bytes = known ? r.c_bytes : span(d->m, d->ldc, d->n) * 4,
                       d_bytes = known ? r.d_bytes : (d->bias ? (size_t)d->n * 4 : 0);
          if (!dt_overlap(pa, a_bytes, r.dst, dst_bytes) && !dt_overlap(pc, c_bytes, r.dst, dst_bytes) && !dt_overlap(pd, d_bytes, r.dst, dst_bytes) &&
              !dt_overlap(pc, c_bytes, r.src, src_bytes)) {
            if (!known) {
              r.sib = dt_sibling(d, t->ldi, false, mode == 2 ? 2 : 1);
              r.sib_of = d;
              r.a_bytes = a_bytes, r.c_bytes = c_bytes, r.d_bytes = d_bytes;
            }
            *src = r.src;
            sib = r.sib;
            mine->folded.store(mine->folded.load(std::memory_order_relaxed) + 1, std::memory_order_relaxed);
          }
        }
        // mode 2: the destination is the gemm's A operand (and not its B: both on the temporary is a gemm that reads the transpose twice,
        // launched like any other). Strict mode needs no test here, as for B: dt_defer makes no record under it.
        const bool aknown = r.asib_of == d;
        if (!sib && mode == 2 && pa == r.dst && pb != r.dst && br == 1 && s == r.stream && queue_active() &&
            (aknown || (d->dtype == DT_F32 && !gemm_on_x6(*d) && !d->vnni_b && !d->vnni_c && !d->b_trans && !d->a_trans && d->m == t->n && d->k == t->m &&
                        d->lda == t->ldo && d->m <= 64 && d->k <= 64))) {
          const size_t b_bytes = aknown ? r.ab_bytes : span(d->k, d->ldb, d->n) * 4, c_bytes = aknown ? r.ac_bytes : span(d->m, d->ldc, d->n) * 4,
                       d_bytes = aknown ? r.ad_bytes : (d->bias ? (size_t)d->n * 4 : 0);
          if (!dt_overlap(pb, b_bytes, r.dst, dst_bytes) && !dt_overlap(pc, c_bytes, r.dst, dst_bytes) && !dt_overlap(pd, d_bytes, r.dst, dst_bytes) &&
              !dt_overlap(pc, c_bytes, r.src, src_bytes)) {
            if (!aknown) {
              r.asib = dt_sibling(d, t->ldi, true, 2);
              r.asib_of = d;
              r.ab_bytes = b_bytes, r.ac_bytes = c_bytes, r.ad_bytes = d_bytes;
            }
            *src = r.src;
            sib = r.asib;
            *a_operand = true;
            mine->folded.store(mine->folded.load(std::memory_order_relaxed) + 1, std::memory_order_relaxed);
          }
        }
      }
    }
    if (!sib) dt_launch(*mine);
  }
  if (g_dt_pending.load(std::memory_order_relaxed) > (sib ? 1 : 0)) { // other threads' records
    const GemmDesc *e = sib ? sib : d;
    const void *a = *a_operand ? *src : pa, *b = sib && !*a_operand ? *src : pb;
    const int64_t vf = e->vnni_factor ? e->vnni_factor : 2;
    const size_t bspan = e->vnni_b ? span((e->k + vf - 1) / vf, vf * e->ldb, vf * e->n) : e->b_trans ? span(e->n, e->ldb, e->k) : span(e->k, e->ldb, e->n);
    const size_t nb = br > 0 ? (size_t)(br - 1) : 0;
    const size_t aspan = e->a_trans ? span(e->k, e->lda, e->m) : span(e->m, e->lda, e->k);
    const DtRange rd[4] = {dt_range(a, (nb * e->stride_a + aspan) * es), dt_range(b, (nb * e->stride_b + bspan) * es),
                           dt_range(pd, e->bias ? (size_t)e->n * es : 0), dt_range(pc, span(e->m, e->ldc, e->n) * es * (e->vnni_c ? 2 : 1))};
    dt_scan_foreign(mine, rd, 4, rd + 3, 1);
  }
  return sib;
}
// any other invoke while transposes are remembered: this thread's record first, then the other threads' records it touches
void dt_other(const void *const *reads, const size_t *read_bytes, int nr, const void *out, size_t out_bytes) {
  if (DtSlot *mine = dt_my_slot(false)) {
    if (mine->live.load(std::memory_order_acquire)) dt_launch(*mine);
  }
  if (g_dt_pending.load(std::memory_order_relaxed) == 0) return;
  DtRange rd[3], wr[1] = {dt_range(out, out_bytes)};
  for (int i = 0; i < nr && i < 3; ++i) rd[i] = dt_range(reads[i], read_bytes[i]);
  dt_scan_foreign(nullptr, rd, nr < 3 ? nr : 3, wr, 1);
}
// The steady state of the query-times-key loop, inlined into xsmm_unary_invoke (round 6): this thread's live record is this very
// transpose (descriptor, destination, stream), nobody else holds the slot, no other record exists, and the new source lies inside the
// device allocation the full path validated in this epoch and inside the hull already published to the other threads: the record's
// source is replaced - the remembered transpose is dead - and nothing else happens. Everything else: dt_defer.
__attribute__((always_inline)) inline bool dt_defer_fast(const UnaryDesc *d, void *pi, void *po, hipStream_t s) {
  CallerState *tl = tl_fast;
  if (!tl || tl->dt_slot < 0 || !membarrier_ok()) return false;
  DtSlot &sl = g_dt_slots[tl->dt_slot];
  if (!sl.live.load(std::memory_order_acquire) || g_dt_pending.load(std::memory_order_relaxed) != 1) return false;
  bool done = false;
  const uint64_t q = sl.oseq.load(std::memory_order_relaxed);
  sl.oseq.store(q + 1, std::memory_order_relaxed); // an owner section (DtOwnerSection), lock-free or not at all
  std::atomic_signal_fence(std::memory_order_seq_cst);
  if (!sl.contended.load(std::memory_order_acquire) && sl.live.load(std::memory_order_relaxed)) {
    DeferredTranspose &r = sl.r;
    const uintptr_t a = (uintptr_t)pi;
    if (r.d == d && r.dst == po && r.stream == s && r.valid_epoch == g_devmem_epoch.load(std::memory_order_relaxed) && a >= r.src_alloc_b) {
      const size_t src_bytes = span(d->m, d->ldi, d->n) * 4, dst_bytes = (size_t)d->n * d->m * 4;
      if (a + src_bytes <= r.src_alloc_e && a >= sl.s_lo.load(std::memory_order_relaxed) && a + src_bytes <= sl.s_hi.load(std::memory_order_relaxed) &&
          !dt_overlap(pi, src_bytes, po, dst_bytes) && cfg().fold_transpose.load(std::memory_order_relaxed) && queue_active()) {
        r.src = pi;
        sl.dropped.store(sl.dropped.load(std::memory_order_relaxed) + 1, std::memory_order_relaxed);
        done = true;
      }
    }
  }
  std::atomic_signal_fence(std::memory_order_seq_cst);
  sl.oseq.store(q + 2, std::memory_order_release);
  return done;
}
// ... and of the gemm that follows it, inlined into the gemm entry points: the descriptor this record folded last, B = the record's
// destination, one batch element, the record's stream, no operand on the destination, C off the source - the sibling and the source.
// B folds only (r.sib_of / r.sib never hold an A sibling): a gemm whose A is the temporary (mode 2) goes through dt_gemm every time.
__attribute__((always_inline)) inline const GemmDesc *dt_gemm_fast(const GemmDesc *d, void *pa, void *pb, void *pc, void *pd, int64_t br, hipStream_t s, void **src) {
  CallerState *tl = tl_fast;
  if (!tl || tl->dt_slot < 0 || !membarrier_ok()) return nullptr;
  DtSlot &sl = g_dt_slots[tl->dt_slot];
  if (!sl.live.load(std::memory_order_acquire) || g_dt_pending.load(std::memory_order_relaxed) != 1) return nullptr;
  const GemmDesc *sib = nullptr;
  const uint64_t q = sl.oseq.load(std::memory_order_relaxed);
  sl.oseq.store(q + 1, std::memory_order_relaxed);
  std::atomic_signal_fence(std::memory_order_seq_cst);
  if (!sl.contended.load(std::memory_order_acquire) && sl.live.load(std::memory_order_relaxed)) {
    DeferredTranspose &r = sl.r;
    if (r.sib_of == d && pb == r.dst && br == 1 && s == r.stream && queue_active()) {
      const UnaryDesc *t = r.d;
      const size_t dst_bytes = (size_t)t->n * t->m * 4, src_bytes = span(t->m, t->ldi, t->n) * 4;
      if (!dt_overlap(pa, r.a_bytes, r.dst, dst_bytes) && !dt_overlap(pc, r.c_bytes, r.dst, dst_bytes) && !dt_overlap(pd, r.d_bytes, r.dst, dst_bytes) &&
          !dt_overlap(pc, r.c_bytes, r.src, src_bytes)) {
        *src = r.src;
        sib = r.sib;
        sl.folded.store(sl.folded.load(std::memory_order_relaxed) + 1, std::memory_order_relaxed);
      }
    }
  }
  std::atomic_signal_fence(std::memory_order_seq_cst);
  sl.oseq.store(q + 2, std::memory_order_release);
  return sib;
}
// a transpose invoke: true = remembered (nothing launched)
bool dt_defer(const UnaryDesc *d, void *pi, void *po, hipStream_t s) {
  if (d->dtype != DT_F32 || d->m > 64 || d->n > 64 || d->ldo != d->m || !cfg().fold_transpose.load(std::memory_order_relaxed) || cfg().strict.load(std::memory_order_relaxed) || !queue_active()) return false;
  DeviceRanges &devmem = caller_state().devmem;
  if (devmem.refresh()) check_queue_device();
  if (!devmem.is_device(pi, 0) || !devmem.is_device(po, 1)) return false;
  const size_t dst_bytes = (size_t)d->n * d->m * 4, src_bytes = span(d->m, d->ldi, d->n) * 4;
  if (dt_overlap(pi, src_bytes, po, dst_bytes)) return false;
  DtSlot *mine = dt_my_slot(true);
  if (!mine) return false;
  const uintptr_t s_lo = (uintptr_t)pi, s_hi = (uintptr_t)pi + src_bytes;
  bool replaced = false, launch_old = false;
  if (mine->live.load(std::memory_order_acquire)) {
    DtOwnerSection sec(*mine);
    if (mine->live.load(std::memory_order_relaxed)) {
      DeferredTranspose &r = mine->r;
      if (r.d == d && r.dst == po && r.stream == s) {
        r.src = pi; // the remembered transpose is dead: fully overwritten, its readers were served from its source
        {           // (for dt_defer_fast: pi and po were just seen to be device memory in devmem's epoch)
          const Range al = devmem.range_of(pi);
          r.src_alloc_b = al.b, r.src_alloc_e = al.e;
          r.valid_epoch = al.e ? devmem.epoch : 0;
        }
        // (the published source range only GROWS while the record lives: the hull of the sources of the loop's transposes - after one
        // pass over the source tensor the line the other threads read is not written any more)
        if (s_lo < mine->s_lo.load(std::memory_order_relaxed)) mine->s_lo.store(s_lo, std::memory_order_relaxed);
        if (s_hi > mine->s_hi.load(std::memory_order_relaxed)) mine->s_hi.store(s_hi, std::memory_order_relaxed);
        mine->dropped.store(mine->dropped.load(std::memory_order_relaxed) + 1, std::memory_order_relaxed);
        replaced = true;
      } else {
        launch_old = true;
      }
    }
  }
  if (launch_old) dt_launch(*mine);
  // the other threads' records this transpose touches (it will read its source and write its destination when it is launched)
  if (g_dt_pending.load(std::memory_order_relaxed) > (replaced ? 1 : 0)) {
    const DtRange rd[1] = {dt_range(pi, src_bytes)}, wr[1] = {dt_range(po, dst_bytes)};
    dt_scan_foreign(mine, rd, 1, wr, 1);
  }
  if (replaced) return true;
  DtOwnerSection sec(*mine);
  if (mine->live.load(std::memory_order_relaxed)) return false; // (cannot happen: only the owner makes a record live)
  mine->r = DeferredTranspose{d, pi, po, s, nullptr, nullptr, 0, 0, 0, 0, 0, 0};
  {
    const Range al = devmem.range_of(pi);
    mine->r.src_alloc_b = al.b, mine->r.src_alloc_e = al.e;
    mine->r.valid_epoch = al.e ? devmem.epoch : 0;
  }
  mine->d_lo.store((uintptr_t)po, std::memory_order_relaxed);
  mine->d_hi.store((uintptr_t)po + dst_bytes, std::memory_order_relaxed);
  mine->s_lo.store(s_lo, std::memory_order_relaxed);
  mine->s_hi.store(s_hi, std::memory_order_relaxed);
  g_dt_pending.fetch_add(1, std::memory_order_relaxed);
  mine->live.store(1, std::memory_order_release);
  return true;
}
