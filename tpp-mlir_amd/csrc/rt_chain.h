// rt_chain.h - chains of whole-layer fused BRGEMMs in one launch: blocks, probation, journal with one error word per launch, re-run
// One of the subsystem units of runtime.cpp (round 6, VERDICT r5 next 7: the 3 000-line file split by subsystem, no behaviour
// change). The units are INCLUDED into the one translation unit runtime.cpp, in dependence order, inside its anonymous namespace:
// the per-invoke host path (14-18 ns: enqueue_item -> join_window -> Segment::mark) crosses four of them and is inlined across
// their borders - as separate objects without LTO it would pay a call per border. Not a stand-alone header: include runtime.cpp's way only.

// ---- chains of whole-layer fused BRGEMMs in one launch (xsmm_hip_fused_brgemm_chain_invoke) -----------------------------
// Hand-off state of the chain kernel (brgemm_bf16_lw.hip, chain mode): arrival counters that only grow - a launch adds
// tiles_n to each, its target is epoch * tiles_n - so a block of counters is tied to ONE (stream, tile grid, layer count):
// launches of one block are ordered by their stream and issued under the mutex (epoch order = stream order). The err word
// lives in pinned host memory: a workgroup whose wait timed out writes it over PCIe, the host reads it at its sync points.
struct ChainBlock {
  hipStream_t stream;
  int tiles_m, tiles_n, nlayers;
  unsigned *cnt; // device: (CH_MAXL - 1) * tiles_m counters, CHAIN_CNT_STRIDE words apart
  unsigned *err; // pinned host
  unsigned epoch;
  int verified;  // launches of this block that were checked synchronously and had every hand-off succeed (probation, see below)
  // a mixed-width chain (xsmm_hip_set_chain_widths): column tiles PER LAYER - part of the key, since a launch adds tiles_l[l] to the counters
  // of layer l (tiles_n is the widest layer's: the grid). All zero in every other block: there every layer has tiles_n.
  int tiles_l[CH_MAXL];
};
// A STARVED chain launch (another process, or another stream's LDS-heavy kernel, held compute units while it ran: not every
// workgroup became resident, a consumer's bounded wait ran out, the error word is set) used to end the process. Round 5 (VERDICT r4
// item 5): the library degrades instead - the reference never aborts on a valid invoke (XsmmRunnerUtils.cpp:363-383).
//  * PROBATION: the first launch of every block (stream, tile grid, layer count) is followed by a stream synchronisation and a look
//    at the error word. A device that is shared when the harness starts is found out here, before anything could consume the
//    launch's outputs: the chain call then runs call by call at once (its inputs are intact: beta 0, outputs overlap no operand),
//    and the process remembers that the device is shared - every later chain invoke runs call by call (TPP_HIP_CHAIN=0 behaviour).
//  * LATER launches stay asynchronous; the calls of every launch since the last check are kept in a journal (the last launch per
//    set of output pointers). If the check at a synchronisation point finds the error word set, the journal is re-run call by call
//    in launch order before the synchronisation returns: what the caller then reads is what the calls compute from the operands as
//    they are now. (Work that OTHERS enqueued between a starved launch and the synchronisation has read invalid outputs - the
//    stderr line says so; the chain contract of include/tpp_xsmm_abi.h asks for the device to oneself for this reason.)
// Round 6: every journaled launch has its OWN error word (a pool of pinned words), so the check knows WHICH launch
// starved: only that launch and the later ones of the same stream are re-run (a healthy earlier launch whose inputs have since
// been overwritten is left alone); the journal is looked at per stream - the one that has just been drained - and the entries of
// other streams stay; when the pool runs dry the launching thread synchronises and checks instead of dropping entries; the re-run
// goes to the launch's stream through a thread-local override (the process-wide stream setting is not touched);
// xsmm_hip_chain_status() counts the repairs, TPP_HIP_CHAIN_STRICT=1 keeps fail-stop.
struct ChainCall {
  int n;
  int64_t dtype;
  int64_t handle[CH_MAXL];
  void *a[CH_MAXL], *b[CH_MAXL], *c[CH_MAXL], *d[CH_MAXL];
  int64_t br[CH_MAXL];
  hipStream_t stream;
  unsigned *err; // this launch's own error word (pinned host memory, from g_chain_err_free)
};
std::vector<ChainCall> g_chain_journal; // under g_chain_mu, in launch order
std::vector<unsigned *> g_chain_err_free; // under g_chain_mu
constexpr int CHAIN_ERR_POOL = 512;
std::atomic<int> g_chain_journaled{0};  // entries in the journal (read without the lock: "is the pool about to run dry")
std::atomic<int64_t> g_chain_repairs{0}; // starved launches found and re-run since process start (xsmm_hip_chain_status)
std::atomic<bool> g_chain_shared{false}; // a chain launch was starved once: no more chain launches in this process
std::mutex g_chain_mu;

std::vector<ChainBlock> g_chain_blocks;
std::atomic<int> g_chain_launched{0}; // chain launches since the last check of the err words

ChainBlock &chain_block(hipStream_t s, int tiles_m, int tiles_n, int nlayers, const int *tiles_l = nullptr) { // under g_chain_mu
  int key_l[CH_MAXL] = {};
  for (int l = 0; tiles_l && l < nlayers && l < CH_MAXL; ++l) key_l[l] = tiles_l[l];
  for (ChainBlock &b : g_chain_blocks)
    if (b.stream == s && b.tiles_m == tiles_m && b.tiles_n == tiles_n && b.nlayers == nlayers && !memcmp(b.tiles_l, key_l, sizeof(key_l))) return b;
  ChainBlock b{s, tiles_m, tiles_n, nlayers, nullptr, nullptr, 0, 0, {}};
  memcpy(b.tiles_l, key_l, sizeof(key_l));
  const size_t bytes = sizeof(unsigned) * (size_t)(CH_MAXL - 1) * (size_t)tiles_m * CHAIN_CNT_STRIDE;
  HIP_OK(hipMalloc((void **)&b.cnt, bytes));
  HIP_OK(hipMemset(b.cnt, 0, bytes));
  HIP_OK(hipHostMalloc((void **)&b.err, sizeof(unsigned), hipHostMallocDefault));
  *b.err = 0;
  g_chain_blocks.push_back(b);
  return g_chain_blocks.back();
}
// after stream `s` has been drained: did a hand-off of a chain launch on it time out?
void chain_rerun_call_by_call(const ChainCall &c);
void check_chain_errors(hipStream_t s) {
  if (!g_chain_launched.load(std::memory_order_acquire)) return;
  std::vector<ChainCall> redo;
  unsigned layer = 0;
  {
    std::lock_guard<std::mutex> lk(g_chain_mu);
    std::vector<ChainCall> keep;
    for (const ChainCall &c : g_chain_journal) {
      if (c.stream != s) { // another stream's launch: not drained by this synchronisation, stays
        keep.push_back(c);
        continue;
      }
      const unsigned e = *(volatile unsigned *)c.err;
      if (e && !layer) layer = e;
      if (layer) redo.push_back(c); // the first starved launch of this stream and every later one (they may have consumed its outputs)
      *(volatile unsigned *)c.err = 0;
      g_chain_err_free.push_back(c.err);
    }
    g_chain_journal.swap(keep);
    g_chain_journaled.store((int)g_chain_journal.size(), std::memory_order_relaxed);
    if (g_chain_journal.empty()) g_chain_launched.store(0, std::memory_order_release);
  }
  if (!layer) return;
  static const bool strict = [] { const char *e = getenv("TPP_HIP_CHAIN_STRICT"); return e && atoi(e) != 0; }();
  if (strict)
    die("tpp-xsmm-hip: a fused-brgemm chain launch was starved (a hand-off for layer %u's input timed out: not every workgroup was resident - "
        "the device is shared) and TPP_HIP_CHAIN_STRICT=1 asks for fail-stop", layer - 1);
  // starved: the device is shared. The starved launch and the later ones of its stream run again, call by call, in launch order;
  // chains are off from now on.
  g_chain_shared.store(true, std::memory_order_release);
  g_chain_repairs.fetch_add((int64_t)redo.size(), std::memory_order_relaxed);
  fprintf(stderr, "[tpp-xsmm-hip] a fused-brgemm chain launch was starved (a hand-off for layer %u's input timed out: not every workgroup "
                  "was resident - the device is shared); that launch and the %zu later one(s) of its stream are re-run call by call now "
                  "(earlier launches completed and are left alone), and chain invokes run call by call from here on "
                  "(xsmm_hip_chain_status() counts; TPP_HIP_CHAIN_STRICT=1 ends the process instead). Work that others enqueued behind a "
                  "starved launch has read invalid data.\n",
          layer - 1, redo.size() - 1);
  for (const ChainCall &c : redo) chain_rerun_call_by_call(c);
  HIP_OK(hipStreamSynchronize(s));
}
void check_chain_errors() { check_chain_errors(cfg().stream.load()); }

int chip_cus() { // compute units of the current device (0: unknown)
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
}
// Compute units a launch on `s` can actually use: the device's, restricted by the stream's CU mask (hipExtStreamCreateWithCUMask,
// or the process-wide ROC_GLOBAL_CU_MASK / HSA_CU_MASK the runtime folds into every stream's mask). The persistent chain kernel
// needs all of its workgroups resident at once - one per CU - so its grid is checked against THIS number. What no query
// can see is another PROCESS (or another stream's LDS-heavy kernel) holding CUs at launch time: the chain launch needs the device
// to itself (include/tpp_xsmm_abi.h says so); every spin in the kernel is bounded and a starved launch is reported, not hung.
int stream_cus(hipStream_t s) {
  const int all = chip_cus();
  uint32_t mask[16] = {};
  if (all <= 0 || hipExtStreamGetCUMask(s, 16, mask) != hipSuccess) {
    (void)hipGetLastError();
    return all;
  }
  int bits = 0;
  for (uint32_t w : mask) bits += __builtin_popcount(w);
  return bits > 0 && bits < all ? bits : all;
}

bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
  return (const char *)a < (const char *)b + nb && (const char *)b < (const char *)a + na;
}

// true: the chain was launched as ONE kernel. false: the caller runs the invokes one by one (same result).
// Three steps: the chain contract (of the process and of the operands' pointers), the decision - ONE call of plan_chain (gemm_plan.h:
// host-only, every switch and the order of the rules are there) -, and the mechanism that carries the plan out: counter block, epoch and
// target, error word, launch, probation, journal. Nothing here looks at a chain switch or derives the launch form again.
static_assert(CHAIN_PLAN_MAXL == CH_MAXL, "plan_chain's layer arrays are the launch's");
bool try_chain_launch(int n, const GemmDesc *const *d, void *const *pa, void *const *pb, void *const *pc, void *const *pd, const int64_t *br,
                      hipStream_t s) {
  // with TPP_HIP_TRACE >= 1 the reason for running call by call goes to stderr
#define NOCHAIN(why)                                                                             \
  do {                                                                                           \
    if (cfg().trace) fprintf(stderr, "[tpp-xsmm-hip] fused_brgemm_chain: call by call (%s)\n", why); \
    return false;                                                                                \
  } while (0)
  if (n < 2 || n > CH_MAXL) NOCHAIN("fewer than 2 or more than 8 calls");
  if (!cfg().async.load(std::memory_order_relaxed)) NOCHAIN("synchronous mode");
  {
    // a launch's hand-off target (epoch x tiles per row block) is baked into its arguments: replayed from a graph it would be
    // stale - the consumers would not wait. Captured streams get the separate launches.
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(cfg().stream.load(std::memory_order_relaxed), &cs) != hipSuccess) (void)hipGetLastError();
    else if (cs != hipStreamCaptureStatusNone) NOCHAIN("the stream is being captured into a graph");
  }
  static const int enabled = [] {
    const char *e = getenv("TPP_HIP_CHAIN");
    return e ? atoi(e) : 1;
  }();
  if (!enabled) NOCHAIN("TPP_HIP_CHAIN=0");
  if (g_chain_shared.load(std::memory_order_acquire)) NOCHAIN("an earlier chain launch was starved: the device is shared");
  thread_local DeviceRanges devmem;
  devmem.refresh();
  for (int i = 0; i < n; ++i) {
    const GemmDesc &g = *d[i];
    if (((uintptr_t)pa[i] | (uintptr_t)pb[i] | (uintptr_t)pc[i]) & 15) NOCHAIN("an operand is not 16-byte aligned");
    if (g.dtype == DT_F32 && g.bias && ((uintptr_t)pd[i] & 15)) NOCHAIN("an f32 bias operand is not 16-byte aligned");
    if (g.bias && (!pd[i] || ((uintptr_t)pd[i] & 7))) NOCHAIN("a bias operand is not 8-byte aligned");
    if (i > 0 && (pa[i] != pc[i - 1] || g.lda != d[i - 1]->ldc)) NOCHAIN("not a chain: a call does not read its predecessor's output");
    // The kernel hands layer i-1's output over row block by row block (a consumer waits for the producers of ITS rows only): every
    // batch element of layer i must stay inside its own rows, i.e. the batch strides walk along k within one leading dimension.
    // (A row-striding stride_a would read rows that other workgroups may not have stored yet.)
    if (i > 0 && (br[i] - 1) * g.stride_a + g.k > g.lda) NOCHAIN("a later call's batch elements leave the rows of its predecessor's output");
    if (!devmem.is_device(pa[i], 0) || !devmem.is_device(pb[i], 1) || !devmem.is_device(pc[i], 2) || (g.bias && !devmem.is_device(pd[i], 3)))
      NOCHAIN("a host operand");
  }
  // The persistent chain kernels need all of their workgroups resident at once: the rules check their grids against the compute units of
  // the stream the launch goes to - asked for through the plan's callback, at most once, and only by a rule that reads them.
  ChainCus cus{[](void *stream) { return (int64_t)stream_cus((hipStream_t)stream); }, (void *)s};
  const ChainLaunchPlan plan = plan_chain(n, d, br, chain_plan_env(), cus);
  if (cfg().trace)
    for (int i = 0; i < plan.n_notes; ++i) fprintf(stderr, "[tpp-xsmm-hip] fused_brgemm_chain: no %s (%s)\n", plan.notes[i].rule, plan.notes[i].why);
  if (plan.form == CF_CALLS) NOCHAIN(plan.why);
  // no operand of the launch may overlap an output (a layer's input rows are read by other workgroups while later layers store)
  Operand A, B, C, D;
  struct Span { const void *p; size_t n; };
  Span outs[CH_MAXL], ins[2 * CH_MAXL + 1], a_in[CH_MAXL];
  int n_ins = 0;
  for (int i = 0; i < n; ++i) {
    gemm_operands(d[i], pa[i], pb[i], pc[i], pd[i], br[i], A, B, C, D);
    outs[i] = Span{C.ptr, C.bytes};
    a_in[i] = Span{A.ptr, A.bytes};
    ins[n_ins++] = Span{B.ptr, B.bytes};
    if (d[i]->bias) ins[n_ins++] = Span{D.ptr, D.bytes};
    if (i == 0) ins[n_ins++] = Span{A.ptr, A.bytes};
  }
  for (int i = 0; i < n; ++i) {
    for (int j = i + 1; j < n; ++j)
      if (ranges_overlap(outs[i].p, outs[i].n, outs[j].p, outs[j].n)) NOCHAIN("two outputs overlap");
    for (int j = 0; j < n_ins; ++j)
      if (ranges_overlap(outs[i].p, outs[i].n, ins[j].p, ins[j].n)) NOCHAIN("an output overlaps an input");
    // the A operand of a later layer is its predecessor's output by construction; what it reads (k may be wider than the
    // predecessor's n: the gap columns of the rows) may overlap no OTHER output of the launch
    for (int j = 1; j < n; ++j)
      if (j != i + 1 && ranges_overlap(outs[i].p, outs[i].n, a_in[j].p, a_in[j].n)) NOCHAIN("an output overlaps a later call's input");
  }
#undef NOCHAIN
  ChainArgs c;
  memset(&c, 0, sizeof(c));
  c.A = pa[0];
  c.lda = d[0]->lda;
  c.m = (int)d[0]->m;
  c.n = plan.args_n;
  c.nlayers = n;
  c.groups = plan.groups;
  for (int i = 0; i < n; ++i)
    c.L[i] = ChainLayer{pb[i], pd[i], pc[i], d[i]->ldb, d[i]->ldc, d[i]->stride_a, d[i]->stride_b, (int)d[i]->k, (int)br[i],
                        EP_BETA0 | (d[i]->bias ? EP_BIAS : 0) | (d[i]->relu ? EP_RELU : 0), plan.mixed || plan.form == CF_SKINNY ? (int)d[i]->n : 0};
  // the pool of error words is about to run dry (hundreds of launches without a synchronisation): synchronise and check here
  // instead of ever dropping a journal entry
  if (g_chain_journaled.load(std::memory_order_relaxed) >= CHAIN_ERR_POOL - 8) {
    std::vector<hipStream_t> streams;
    {
      std::lock_guard<std::mutex> lk0(g_chain_mu);
      for (const ChainCall &j : g_chain_journal)
        if (std::find(streams.begin(), streams.end(), j.stream) == streams.end()) streams.push_back(j.stream);
    }
    for (hipStream_t st : streams) {
      HIP_OK(hipStreamSynchronize(st));
      check_chain_errors(st);
    }
    if (g_chain_shared.load(std::memory_order_acquire)) return false; // (found a starved launch: call by call from here on)
  }
  std::lock_guard<std::mutex> lk(g_chain_mu);
  // The block's key is the plan's grid: row blocks (ceil-divided in a form with edge row tiles: the counters it uses) and column tiles
  // (the arrivals per counter). A width form is keyed on the widest layer's column tiles AND every layer's own - two chains with one grid
  // but different inner widths add different numbers to a layer's counters and may not share them.
  ChainBlock &blk = chain_block(s, plan.tiles_m, plan.tiles_n, n, plan.mixed ? plan.tiles_l : nullptr);
  c.cnt = blk.cnt;
  c.err = blk.err; // probation launches: the block's word (checked right behind the launch)
  if (blk.verified >= 1) {
    if (g_chain_err_free.empty() && g_chain_journal.empty()) { // first use: the pool
      unsigned *pool = nullptr;
      HIP_OK(hipHostMalloc((void **)&pool, sizeof(unsigned) * CHAIN_ERR_POOL, hipHostMallocDefault));
      for (int i = 0; i < CHAIN_ERR_POOL; ++i) {
        pool[i] = 0;
        g_chain_err_free.push_back(pool + i);
      }
    }
    if (g_chain_err_free.empty()) return false; // (cannot happen: the check above keeps 8 words spare; call by call is always right)
    c.err = g_chain_err_free.back();
    g_chain_err_free.pop_back();
  }
  // (a width form: the kernel multiplies by the producing layer's column tiles - chain_widths_target / chain_wragged_target)
  c.target = plan.mixed ? ++blk.epoch : ++blk.epoch * (unsigned)blk.tiles_n;
  // the launch and the form's *_stats words (xsmm_hip_chain_*_stats): launches; then row blocks, column tiles and the GemmVariant of the tile
  // with its B image, unless the case says otherwise
  const int tile = plan.tile, b_kind = plan.b_kind;
  tpp::ModeSwitch counted = tpp::MS_COUNT; // the switch whose counters the launch moves (mode_switches.h); MS_COUNT: none
  int64_t word[3] = {plan.tiles_m, plan.tiles_n, blw_variant(tile, b_kind)};
  switch (plan.form) {
  case CF_F32: HIP_OK(launch_f32_chain(tile, c, s)); break;
  case CF_PLAIN: HIP_OK(launch_bf16_chain(BLW_LAYER, tile, b_kind, c, s)); break;
  case CF_EDGE: HIP_OK(launch_bf16_chain(BLW_CHAIN_EDGE, tile, b_kind, c, s)); counted = tpp::MS_CHAIN_EDGE; break;
  case CF_ROUNDS: // row groups G, rounds R
    HIP_OK(launch_bf16_chain(BLW_CHAIN_ROUNDS, tile, b_kind, c, s)); counted = tpp::MS_CHAIN_ROUNDS;
    word[0] = plan.groups, word[1] = (plan.tiles_m + plan.groups - 1) / plan.groups;
    break;
  case CF_RAGGED: HIP_OK(launch_bf16_chain_ragged(tile, b_kind, c, s)); counted = tpp::MS_CHAIN_RAGGED; break;
  case CF_WIDTHS: HIP_OK(launch_bf16_chain_widths(tile, b_kind, c, s)); counted = tpp::MS_CHAIN_WIDTHS; break;
  case CF_WROUNDS: // row blocks, resident workgroup columns W
    HIP_OK(launch_bf16_chain_wrounds(tile, b_kind, c, s)); counted = tpp::MS_CHAIN_WIDTH_ROUNDS;
    word[1] = plan.groups;
    break;
  case CF_WRAGGED: HIP_OK(launch_bf16_chain_wragged(tile, b_kind, c, s)); counted = tpp::MS_CHAIN_WIDTHS_RAGGED; break;
  case CF_DMA256: // row groups G, rounds R, the B image
    HIP_OK(launch_bf16_dma256_chain(b_kind, c, s)); counted = tpp::MS_CHAIN_DMA256;
    word[0] = plan.groups, word[1] = chain_rounds_rounds(plan.tiles_m, plan.groups), word[2] = b_kind;
    break;
  case CF_SKINNY: // resident workgroups G, the column-block width BN (the plan's tile), the B image; the block's key is (1, G): target = epoch * G
    HIP_OK(launch_bf16_skinny_chain(b_kind, tile, c, s)); counted = tpp::MS_CHAIN_SKINNY;
    word[0] = plan.groups, word[1] = tile, word[2] = b_kind;
    break;
  default: return false; // (CF_CALLS has returned above)
  }
  if (counted != tpp::MS_COUNT) tpp::count_mode_launch(counted, {word[0], word[1], word[2]});
  if (blk.verified < 1) {
    // probation (comment at ChainBlock): wait for this launch and look at its error word before anyone can consume its outputs
    HIP_OK(hipStreamSynchronize(s));
    const unsigned e = *(volatile unsigned *)blk.err;
    if (e) {
      *(volatile unsigned *)blk.err = 0;
      g_chain_shared.store(true, std::memory_order_release);
      fprintf(stderr, "[tpp-xsmm-hip] the first fused-brgemm chain launch on this stream was starved (a hand-off for layer %u's input timed "
                      "out: not every workgroup was resident - the device is shared): this call and every later chain invoke run call "
                      "by call.\n", e - 1);
      return false; // the caller runs the calls one by one (inputs intact: beta 0, outputs overlap no operand)
    }
    ++blk.verified;
    return true;
  }
  // journal: the calls of this launch with its own error word, for a re-run should the check at the next synchronisation of this
  // stream find it starved
  {
    ChainCall j;
    j.n = n;
    j.dtype = d[0]->dtype;
    j.stream = s;
    j.err = c.err;
    for (int i = 0; i < n; ++i) {
      j.handle[i] = reinterpret_cast<int64_t>(d[i]);
      j.a[i] = pa[i]; j.b[i] = pb[i]; j.c[i] = pc[i]; j.d[i] = pd[i]; j.br[i] = br[i];
    }
    g_chain_journal.push_back(j);
    g_chain_journaled.store((int)g_chain_journal.size(), std::memory_order_relaxed);
  }
  g_chain_launched.store(1, std::memory_order_release);
  return true;
}

// the calls of one journaled chain launch, one by one (operands are pointers with offsets applied: offsets 0)
void chain_rerun_call_by_call(const ChainCall &c) {
  // on the stream the launch went to - through this thread's override: the process-wide setting is not touched (another thread may
  // invoke, or call xsmm_hip_set_stream, meanwhile: ADVICE r5)
  tl_hot.stream_override = c.stream;
  tl_hot.has_stream_override = true;
  for (int i = 0; i < c.n; ++i)
    xsmm_fused_brgemm_invoke(c.dtype, c.handle[i], c.a[i], 0, c.b[i], 0, c.c[i], 0, c.d[i], 0, c.br[i]);
  flush_tile_queue();
  tl_hot.has_stream_override = false;
}
