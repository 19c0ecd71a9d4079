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
  const int64_t m = d[0]->m, nn = d[0]->n;
  thread_local DeviceRanges devmem;
  devmem.refresh();
  // f32 chains (round 4): every call planned on the SAME K-split loader-wave tile (the launch is then bit-identical to the calls)
  const bool f32 = d[0]->dtype == DT_F32;
  const int f32_tile = f32 ? f32_chain_tile(*d[0]) : -1;
  // RAGGED m (xsmm_hip_set_chain_edge, opt-in; gemm_plan.cpp plan_chain_edge): where the rules of the divisible chain below say no
  // because of the SHAPE - a call no loader-wave tile divides (no B image by bf16_lw_b_kind, planned on the generic kernel), no tile
  // whose rows divide m fits the compute units - a bf16 chain may still run as one launch on edge row tiles. `divisible` = the
  // rules as they are with the switch off still hold; edge_kind = the B image of the ragged launch, edge_why = why there is none.
  // With the switch off edge_on is false and every NOCHAIN below is taken exactly as before.
  // ON THE 256x256 TILE (xsmm_hip_set_chain_dma256, opt-in; gemm_plan.cpp plan_chain_dma256, brgemm_bf16_dma256_chain.hip): asked FIRST, and
  // only with the switch non-zero. The rule sees the calls' shapes, their shared B image (chain_dma256_b_kind) and whether every call runs
  // on that tile as a single call (chain_dma256_on_tile; mode 1 reads xsmm_hip_set_dma256_images for it, nothing else reads another mode).
  // d256 = the launch is that tile's chain kernel on d256_groups row groups: the shape terms of the loader-wave chain below are the
  // rule's then and no other chain switch is looked at; everything the chain contract asks of the operands is checked as for every
  // launch, and blocks, targets, probation and the journal are the same. Where the rule refuses or gates, or the mode is 0, d256 is false
  // and every decision below is exactly what it is without this switch.
  const int dma256_mode = g_chain_dma256.load(std::memory_order_relaxed);
  int d256_groups = 0, d256_kind = -1;
  if (dma256_mode) {
    const char *w = "the calls differ in m or n, or a batch is empty";
    const int images = dma256_mode == 1 ? g_dma256_images.load(std::memory_order_relaxed) : 0;
    bool same = true, on_tile = true;
    d256_kind = chain_dma256_b_kind(*d[0]);
    int64_t ks[CH_MAXL], brs[CH_MAXL];
    for (int i = 0; i < n; ++i) {
      if (d[i]->m != m || d[i]->n != nn || br[i] < 1) same = false;
      if (d256_kind != -2 && chain_dma256_b_kind(*d[i]) != d256_kind) d256_kind = chain_dma256_b_kind(*d[i]) == -2 ? -2 : -1;
      on_tile = on_tile && chain_dma256_on_tile(*d[i], images);
      ks[i] = d[i]->k, brs[i] = br[i];
    }
    if (same) {
      const ChainDma256Plan dp = plan_chain_dma256(m, nn, n, ks, brs, stream_cus(s), on_tile, d256_kind, dma256_mode, cfg().strict.load(std::memory_order_relaxed));
      w = dp.why;
      if (dp.take && !dp.gated) d256_groups = dp.groups; // (gated: the rule's answer is on record in why, nothing is launched)
    }
    if (!d256_groups && cfg().trace) fprintf(stderr, "[tpp-xsmm-hip] fused_brgemm_chain: no launch on the 256x256 tile (%s)\n", w);
  }
  const bool d256 = d256_groups > 0;
  const int chain_edge = d256 ? 0 : g_chain_edge.load(std::memory_order_relaxed);
  const bool edge_on = !f32 && chain_edge != 0;
  bool divisible = true;
  const char *edge_why = nullptr;
  const int edge_kind = edge_on ? chain_edge_b_kind(*d[0], chain_edge, &edge_why) : -1;
  // SEVERAL ROUNDS (xsmm_hip_set_chain_rounds, opt-in; gemm_plan.cpp plan_chain_rounds): a bf16 chain that passes every rule of the
  // divisible chain but the last one - more tiles than compute units - may run as one launch on G resident row groups. The rule is asked
  // only where the rules below say "more tiles than compute units" - of the tile all calls were planned on, or of every tile -, a
  // forced G (mode 1000 + G) in front of them. With the switch off rounds_mode is 0 and every NOCHAIN below is taken exactly as before.
  const int rounds_mode = f32 || d256 ? 0 : g_chain_rounds.load(std::memory_order_relaxed);
  int groups = 0; // > 0: the multi-round launch on that many row groups
  const char *rounds_why = nullptr;
  // A forced G is asked in front of the one-round rules, so also in front of their m and n terms (bf16_lw_b_kind: 64 rows for VNNI-2):
  // rounds_kind = the B image every call has by chain_rounds_b_kind, -1 = none or not the same.
  int rounds_kind = -1;
  if (chain_rounds_mode_forced(rounds_mode)) {
    rounds_kind = chain_rounds_b_kind(*d[0]);
    for (int i = 1; i < n; ++i)
      if (chain_rounds_b_kind(*d[i]) != rounds_kind) rounds_kind = -1;
  }
  // RAGGED WIDTH (xsmm_hip_set_chain_ragged, opt-in; gemm_plan.cpp plan_chain_ragged): asked only where the rules below end in NOCHAIN
  // because of n or k - a call no loader-wave tile takes (k % 64, n % 64, planned on the generic kernel), no ragged-m launch (edge_why: a
  // k % 64), plan_chain_edge's refusal (n not in whole column tiles). ragged_w() is the rule's answer, asked at most once: every call
  // passes chain_ragged_b_kind with the same B image and plan_chain_ragged names a tile. ragw = the launch is the ragged-width one. With
  // the switch off ragged_w() is false without a look at the calls and every NOCHAIN below is taken exactly as before.
  const int chain_ragged = f32 || d256 ? 0 : g_chain_ragged.load(std::memory_order_relaxed);
  int ragw_state = chain_ragged ? -1 : 0, ragw_tile = -1, ragw_kind = -1; // -1 not asked yet, 0 no, 1 yes
  bool ragw = false;
  auto ragged_w = [&]() {
    if (ragw_state >= 0) return ragw_state == 1;
    ragw_state = 0;
    const char *w = nullptr;
    ragw_kind = chain_ragged_b_kind(*d[0], chain_ragged, &w);
    for (int i = 1; i < n && ragw_kind >= 0; ++i)
      if (chain_ragged_b_kind(*d[i], chain_ragged, &w) != ragw_kind || d[i]->m != m || d[i]->n != nn) ragw_kind = -1; // (calls that differ in m or n: the loop below says so)
    if (ragw_kind >= 0) {
      int64_t ks[CH_MAXL], brs[CH_MAXL];
      for (int i = 0; i < n; ++i) ks[i] = d[i]->k, brs[i] = br[i];
      const int et = g_edge_tiles.load(std::memory_order_relaxed);
      const ChainRaggedPlan rp = plan_chain_ragged(m, nn, n, ks, brs, stream_cus(s), et >= V_BF16_LW_32x64 && et <= V_BF16_LW_128x128 ? et - V_BF16_LW_32x64 : -1,
                                                   ragw_kind, chain_ragged, cfg().strict.load(std::memory_order_relaxed));
      w = rp.why;
      ragw_tile = rp.tile;
      if (rp.tile >= 0) ragw_state = 1;
    }
    if (!ragw_state && cfg().trace) fprintf(stderr, "[tpp-xsmm-hip] fused_brgemm_chain: no ragged-width launch (%s)\n", w ? w : "the calls' B operands differ in kind");
    return ragw_state == 1;
  };
  // MIXED WIDTHS (xsmm_hip_set_chain_widths, opt-in; gemm_plan.cpp plan_chain_widths): asked only where the loop below would end in NOCHAIN
  // because two calls differ in n (a difference in m, or an empty batch, still refuses). widths_w() is the rule's answer, asked at most
  // once: every call is bf16, beta 0, stores no VNNI C, was not dispatched to the generic kernel and has the same B image by
  // bf16_lw_b_kind - the terms of the divisible chain, which every call must ALSO pass in the loop below (a ragged call ends the launch:
  // `divisible`) -, the same m and a batch, and plan_chain_widths names a tile. widw = the launch is the mixed-width one. With the
  // switch off widths_w() is false without a look at the calls and the NOCHAIN is taken exactly as before.
  const int chain_widths = f32 || d256 ? 0 : g_chain_widths.load(std::memory_order_relaxed);
  // COLUMN ROUNDS (xsmm_hip_set_chain_width_rounds, opt-in; gemm_plan.cpp plan_chain_width_rounds): the same question about the same calls,
  // answered inside widths_w(): a forced W (1000 + W) in front of plan_chain_widths, the rule (1) where plan_chain_widths refuses or gates
  // or its switch is off. widw_groups > 0 = the launch is the column-round one on that many workgroup columns. With both switches off
  // widths_w() is false without a look at the calls.
  const int width_rounds = f32 || d256 ? 0 : g_chain_width_rounds.load(std::memory_order_relaxed);
  int widw_state = chain_widths || width_rounds ? -1 : 0, widw_tile = -1, widw_kind = -1, widw_groups = 0; // -1 not asked yet, 0 no, 1 yes
  bool widw = false;
  auto widths_w = [&]() {
    if (widw_state >= 0) return widw_state == 1;
    widw_state = 0;
    const char *w = "a call differs in m, has an empty batch, is not bf16 / beta 0 / on a loader-wave tile, or the calls' B operands differ in kind";
    widw_kind = bf16_lw_b_kind(*d[0]);
    for (int i = 0; i < n && widw_kind >= 0; ++i) {
      const GemmDesc &g = *d[i];
      if (g.dtype != DT_BF16 || g.vnni_c || !g.beta0 || g.variant == V_GENERIC || bf16_lw_b_kind(g) != widw_kind || g.m != m || br[i] < 1) widw_kind = -1;
    }
    if (widw_kind >= 0) {
      int64_t ns[CH_MAXL], ks[CH_MAXL], brs[CH_MAXL];
      for (int i = 0; i < n; ++i) ns[i] = d[i]->n, ks[i] = d[i]->k, brs[i] = br[i];
      const int planned = chain_rounds_planned_tile(n, d);
      const bool strict_ = cfg().strict.load(std::memory_order_relaxed);
      auto ask_width_rounds = [&]() {
        // (mode 1 without a tile all calls were dispatched on: plan_chain_width_rounds' gate, or a refusal in front of it - never a launch.
        // Answered here, without asking for the stream's compute units: on a launch-bound chain the runtime calls behind stream_cus
        // showed - 1024 rows x [1024, 512, 256, 128], gated, call by call with the switch off / on 16.38 / 17.06 us per step in every pair;
        // with this answer 18.65 / 18.65 in a later session, profiles/chain_width_rounds_ab.txt)
        if (width_rounds == 1 && planned < 0) {
          w = "column rounds by rule only on a tile all calls were dispatched on (plan_chain_width_rounds' gate)";
          return;
        }
        const ChainWidthRoundsPlan rp = plan_chain_width_rounds(m, n, ns, ks, brs, stream_cus(s), planned, widw_kind, width_rounds, strict_);
        w = rp.why;
        if (rp.tile < 0 || rp.gated) return; // (gated: the rule's answer is on record in why, nothing is launched)
        widw_tile = rp.tile;
        widw_groups = rp.groups;
        widw_state = 1;
      };
      if (chain_width_rounds_mode_forced(width_rounds)) ask_width_rounds(); // (a forced W that does not fit: everything below as with the switch off)
      if (!widw_state && chain_widths) {
        const ChainWidthsPlan wp = plan_chain_widths(m, n, ns, ks, brs, stream_cus(s), planned, widw_kind, chain_widths, strict_);
        w = wp.why;
        widw_tile = wp.tile;
        if (wp.tile >= 0) widw_state = 1;
      }
      if (!widw_state && width_rounds == 1) ask_width_rounds();
    }
    if (!widw_state && cfg().trace) fprintf(stderr, "[tpp-xsmm-hip] fused_brgemm_chain: no mixed-width launch (%s)\n", w);
    return widw_state == 1;
  };
  // RAGGED MIXED WIDTHS (xsmm_hip_set_chain_widths_ragged, opt-in; gemm_plan.cpp plan_chain_widths_ragged): asked where the loop below meets
  // calls that differ in n and the mixed-width rules above do not take the chain - at the n term itself, or earlier at a call no loader-wave
  // tile takes (k % 64, a ragged m or n) -, and where the launch would end in "different widths combine with no other chain mode".
  // wragged_w() is the rule's answer, asked at most once: the calls differ in n, every call passes chain_widths_ragged_b_kind with the same B
  // image, has the same m and a batch, and plan_chain_widths_ragged names a tile without a gate. wragw = the launch is the ragged mixed-width
  // one: the shape terms below are the rule's then, everything else the chain contract asks is checked as for every launch. With the
  // switch off wragged_w() is false without a look at the calls and every NOCHAIN below is taken exactly as before.
  const int chain_wragged = f32 || d256 ? 0 : g_chain_widths_ragged.load(std::memory_order_relaxed);
  int wragw_state = chain_wragged ? -1 : 0, wragw_tile = -1, wragw_kind = -1; // -1 not asked yet, 0 no, 1 yes
  bool wragw = false;
  auto wragged_w = [&]() {
    if (wragw_state >= 0) return wragw_state == 1;
    wragw_state = 0;
    const char *w = nullptr;
    bool differ = false;
    for (int i = 1; i < n; ++i)
      if (d[i]->n != nn) differ = true;
    if (!differ) w = "every call has the same n: the equal-width chain switches decide";
    else wragw_kind = chain_widths_ragged_b_kind(*d[0], chain_wragged, &w);
    for (int i = 0; i < n && wragw_kind >= 0; ++i)
      if (chain_widths_ragged_b_kind(*d[i], chain_wragged, &w) != wragw_kind || d[i]->m != m || br[i] < 1) wragw_kind = -1;
    if (wragw_kind >= 0) {
      int64_t ns[CH_MAXL], ks[CH_MAXL], brs[CH_MAXL];
      for (int i = 0; i < n; ++i) ns[i] = d[i]->n, ks[i] = d[i]->k, brs[i] = br[i];
      const int et = g_edge_tiles.load(std::memory_order_relaxed);
      const ChainWidthsRaggedPlan rp = plan_chain_widths_ragged(m, n, ns, ks, brs, stream_cus(s), et >= V_BF16_LW_32x64 && et <= V_BF16_LW_128x128 ? et - V_BF16_LW_32x64 : -1,
                                                                wragw_kind, chain_wragged, cfg().strict.load(std::memory_order_relaxed));
      w = rp.why;
      wragw_tile = rp.tile;
      if (rp.tile >= 0 && !rp.gated) wragw_state = 1; // (gated: the rule's answer is on record in why, nothing is launched)
    }
    if (!wragw_state && cfg().trace) fprintf(stderr, "[tpp-xsmm-hip] fused_brgemm_chain: no ragged mixed-width launch (%s)\n", w ? w : "the calls differ in m, have an empty batch, or their B operands differ in kind");
    return wragw_state == 1;
  };
  for (int i = 0; i < n; ++i) {
    const GemmDesc &g = *d[i];
    if (edge_on && !edge_why) {
      const char *w = nullptr;
      if (chain_edge_b_kind(g, chain_edge, &w) != edge_kind) edge_why = w ? w : "the calls' B operands differ in kind (VNNI-2 / flat / VNNI-4)";
    }
    if (f32) {
      if (g.dtype != DT_F32 || !g.beta0 || f32_chain_tile(g) < 0 || f32_chain_tile(g) != f32_tile)
        NOCHAIN("an f32 call is not beta 0 / not planned on the K-split loader-wave tile of the first call");
      if (g.bias && ((uintptr_t)pd[i] & 15)) NOCHAIN("an f32 bias operand is not 16-byte aligned");
      if (g.ldc & 3) NOCHAIN("an f32 output's leading dimension is not a multiple of 4");
    } else if (d256) {
      // (the 256x256 tile's chain: bf16, beta 0, one B image, k in 32-k chunks - plan_chain_dma256 has asked)
    } else
    // every layer the same kind of B operand (VNNI-2, flat or VNNI-4: the B image is a template parameter of the launch)
    if (g.dtype != DT_BF16 || g.vnni_c || !g.beta0 || bf16_lw_b_kind(g) < 0 || bf16_lw_b_kind(g) != bf16_lw_b_kind(*d[0])) {
      if ((!edge_on || edge_why) && rounds_kind < 0 && !ragw && !wragw) { // (edge_why: no ragged launch either - an f32 call, a VNNI C, beta 1, a forced kernel, k % 64, the operands' grid)
        if (ragged_w()) ragw = true;
        else if (wragged_w()) wragw = true;
        else NOCHAIN("a call is not bf16 / beta 0 / aligned for the LDS-DMA tiles, or the calls' B operands differ in kind (VNNI-2 / flat / VNNI-4)");
      }
      divisible = false;
    }
    if (g.m != m || br[i] < 1 || (g.n != nn && !wragw && !widths_w() && !wragged_w())) NOCHAIN("the calls differ in m or n, or a batch is empty");
    if (g.n != nn && !wragw) {
      if (widw_state == 1) widw = true;
      else wragw = true; // (the mixed-width rules do not take the chain, the ragged mixed-width rule does)
    }
    if (g.variant == V_GENERIC && !d256) { // (a forced generic kernel stays generic; one that is generic only because no tile divides m may run ragged)
      if ((!edge_on || edge_why || g.generic_forced) && !ragw && !wragw) {
        if (!g.generic_forced && ragged_w()) ragw = true;
        else if (!g.generic_forced && wragged_w()) wragw = true;
        else NOCHAIN("a call was dispatched to the generic kernel");
      }
      divisible = false;
    }
    if (((uintptr_t)pa[i] | (uintptr_t)pb[i] | (uintptr_t)pc[i]) & 15) NOCHAIN("an operand is not 16-byte aligned");
    if (g.bias && (!pd[i] || ((uintptr_t)pd[i] & 7))) NOCHAIN("a bias operand is not 8-byte aligned");
    if (i > 0 && (pa[i] != pc[i - 1] || g.lda != d[i - 1]->ldc)) NOCHAIN("not a chain: a call does not read its predecessor's output");
    // The kernel hands layer i-1's output over row block by row block (a consumer waits for the producers of ITS rows only): every
    // batch element of layer i must stay inside its own rows, i.e. the batch strides walk along k within one leading dimension.
    // (A row-striding stride_a would read rows that other workgroups may not have stored yet.)
    if (i > 0 && (br[i] - 1) * g.stride_a + g.k > g.lda) NOCHAIN("a later call's batch elements leave the rows of its predecessor's output");
    if (!devmem.is_device(pa[i], 0) || !devmem.is_device(pb[i], 1) || !devmem.is_device(pc[i], 2) || (g.bias && !devmem.is_device(pd[i], 3)))
      NOCHAIN("a host operand");
  }
  if (!divisible && edge_why && rounds_kind < 0 && !ragw && !wragw) {
    if (ragged_w()) ragw = true;
    else if (wragged_w()) wragw = true;
    else NOCHAIN(edge_why);
  }
  // The tile: all workgroups must be co-resident (one per CU by LDS), so the grid may not exceed the CUs. If every layer was planned
  // with the same loader-wave tile and that tile fits, use it - the launch is then bit-identical to the separate launches; else
  // the smallest tile that fits (most CUs busy).
  int tile = -1, bm = 0, bn = 0;
  const int64_t cus = stream_cus(s); // (the stream the launch goes to: ADVICE r4)
  auto fits = [&](int t) {
    if (f32) (void)f32_chain_tile_dims(t, &bm, &bn);
    else blw_tile_dims(t, &bm, &bn);
    return m % bm == 0 && nn % bn == 0 && (m / bm) * (nn / bn) <= cus;
  };
  if (f32 && !fits(f32_tile)) NOCHAIN("more tiles than compute units");
  int b_kind = f32 || !divisible ? 0 : bf16_lw_b_kind(*d[0]);
  const bool strict = cfg().strict.load(std::memory_order_relaxed);
  int shared_tile = -1; // the loader-wave tile ALL calls were planned on (bf16)
  auto ask_rounds = [&]() { // the multi-round rule's tile and groups, or rounds_why
    int64_t ks[CH_MAXL], brs[CH_MAXL];
    for (int i = 0; i < n; ++i) ks[i] = d[i]->k, brs[i] = br[i];
    const ChainRoundsPlan rp = plan_chain_rounds(m, nn, n, ks, brs, cus, shared_tile, rounds_mode, strict);
    rounds_why = rp.why;
    if (rp.tile < 0 || rp.gated) return; // (gated: the rule's answer is on record in why, nothing is launched)
    tile = rp.tile;
    groups = rp.groups;
  };
  if (!ragw && !wragw && !divisible && rounds_kind >= 0) { // (a forced G on calls only the one-round rules' m and n terms refuse)
    shared_tile = chain_rounds_planned_tile(n, d);
    ask_rounds();
    if (tile >= 0) b_kind = rounds_kind;
    else if (!edge_on || edge_why) NOCHAIN(rounds_why);
  }
  // the one-round ragged-m rule's answer, asked at most once (only with xsmm_hip_set_chain_edge on and every call passing chain_edge_b_kind)
  ChainEdgePlan edge_plan{-1, nullptr};
  bool edge_asked = false;
  auto ask_edge = [&]() -> const ChainEdgePlan & {
    if (edge_asked) return edge_plan;
    edge_asked = true;
    int64_t ks[CH_MAXL], brs[CH_MAXL];
    for (int i = 0; i < n; ++i) ks[i] = d[i]->k, brs[i] = br[i];
    const int et = g_edge_tiles.load(std::memory_order_relaxed);
    edge_plan = plan_chain_edge(m, nn, n, ks, brs, cus, et >= V_BF16_LW_32x64 && et <= V_BF16_LW_128x128 ? et - V_BF16_LW_32x64 : -1, strict);
    return edge_plan;
  };
  if (widw && !wragw && (!divisible || ragw)) {
    if (wragged_w()) wragw = true; // (the rule of the combination, asked instead of the refusal - only with its switch on)
    else NOCHAIN("the calls differ in n and one of them is ragged: different widths combine with no other chain mode");
  }
  if (wragw) widw = ragw = false; // (one launch form: the ragged mixed-width one)
  if (d256) { // the 256x256 tile's chain kernel: no loader-wave tile is chosen (bm = bn = 256 below)
    tile = 3;
    b_kind = d256_kind;
    groups = 0;
  }
  if (divisible && !widw && !wragw && !d256) {
    // (variants 20 .. 23 VNNI-2, 24 .. 27 flat B, 28 .. 31 VNNI-4: the same four tiles)
    const int planned = blw_variant_tile(d[0]->variant, b_kind);
    bool same = !f32 && planned >= 0 && planned < 4;
    for (int i = 1; i < n && same; ++i) same = d[i]->variant == d[0]->variant;
    if (rounds_mode) shared_tile = chain_rounds_planned_tile(n, d); // (= same ? planned : -1 for a bf16 chain)
    if (f32) tile = f32_tile;
    if (chain_rounds_mode_forced(rounds_mode)) ask_rounds(); // (a forced G that does not fit: everything below as with the switch off)
    if (tile < 0 && same && fits(planned)) tile = planned;
    // the tile all calls were planned on has more tiles than compute units: several rounds on THAT tile - the descriptors' own, G
    // changes no bit, so strict mode takes it too - in front of one round on another tile, whose bits need not be the calls'. Not where
    // the one-round ragged launch applies (xsmm_hip_set_chain_edge on, a tile of other rows fits on its ceil-divided grid): the two
    // switches never combine, and there the ragged launch wins - 32 * 257 rows x 64 of flat B, planned on 32x64 (257 tiles), run as 129
    // edge row blocks of 64x64 with both switches on as with xsmm_hip_set_chain_edge alone (tests/test_chain_dispatch.py found the rounds)
    if (tile < 0 && rounds_mode == 1 && same && !(edge_on && !edge_why && ask_edge().tile >= 0)) ask_rounds();
    if (tile < 0 && strict) NOCHAIN(rounds_why && rounds_mode == 1 ? rounds_why : "strict mode: one launch only on the tile the layers were planned on");
    for (int t = 0; t < 4 && tile < 0; ++t)
      if (fits(t)) tile = t;
    if (tile < 0 && (!edge_on || edge_why)) {
      if (rounds_mode == 1) ask_rounds();
      if (tile < 0) NOCHAIN(rounds_mode == 1 ? rounds_why : "more tiles than compute units");
    }
  }
  if (ragw) { // the ragged-width launch: the rule's tile and the calls' B image
    tile = ragw_tile;
    b_kind = ragw_kind;
  }
  if (widw) { // the mixed-width launch: the rule's tile (whole tiles of m and of every n, the widest layer's grid within the compute units)
    tile = widw_tile;
    b_kind = widw_kind;
  }
  if (wragw) { // the ragged mixed-width launch: the rule's tile (ceil-divided both ways, the widest layer's grid within the compute units)
    tile = wragw_tile;
    b_kind = wragw_kind;
    groups = 0;
  }
  bool ragged = tile < 0; // (only with a switch on: every path to here with both off has a tile)
  if (ragged) {
    // the ragged launch: the tile a forcing edge-tile mode names if it fits, else the smallest that fits - counted on the ceil-divided grid
    const ChainEdgePlan &ep = ask_edge();
    if (ep.tile >= 0) {
      tile = ep.tile;
      b_kind = edge_kind;
    } else {
      // the two switches never combine: the one-round ragged launch is asked first, and only a shape every tile of which divides - one
      // the ragged rule has just refused - may run in several rounds
      if (divisible && rounds_mode == 1) ask_rounds();
      if (tile < 0 && !divisible && ragged_w()) { // (plan_chain_edge's refusal of calls no tile divides: n not in whole column tiles)
        ragw = true;
        tile = ragw_tile;
        b_kind = ragw_kind;
      }
      if (tile < 0) NOCHAIN(ep.why);
      ragged = false;
    }
  }
  if (f32) (void)f32_chain_tile_dims(tile, &bm, &bn); // bm, bn of the chosen tile
  else blw_tile_dims(tile, &bm, &bn);
  if (d256) bm = bn = D256C_BM;
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
  c.m = (int)m;
  c.n = (int)nn;
  c.nlayers = n;
  for (int i = 0; i < n; ++i)
    c.L[i] = ChainLayer{pb[i], pd[i], pc[i], d[i]->ldb, d[i]->ldc, d[i]->stride_a, d[i]->stride_b, (int)d[i]->k, (int)br[i],
                        EP_BETA0 | (d[i]->bias ? EP_BIAS : 0) | (d[i]->relu ? EP_RELU : 0), widw || wragw ? (int)d[i]->n : 0};
  int widw_tiles[CH_MAXL] = {}; // a mixed-width chain: column tiles per layer; the grid is the widest layer's
  if (widw) {
    for (int i = 0; i < n; ++i) {
      widw_tiles[i] = (int)(d[i]->n / bn);
      if (d[i]->n > c.n) c.n = (int)d[i]->n;
    }
  }
  if (wragw) { // (a ragged mixed-width chain: the same key, ceil-divided - the arrivals a launch adds to layer i's counters)
    for (int i = 0; i < n; ++i) {
      widw_tiles[i] = (int)((d[i]->n + bn - 1) / bn);
      if (d[i]->n > c.n) c.n = (int)d[i]->n;
    }
  }
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
  // (a ragged chain: keyed on ceil(m / BM), the counters it uses; a ragged-width chain on ceil(n / BN) as well - the arrivals per counter)
  // (a mixed-width chain: on the widest layer's column tiles AND every layer's own - two chains with one grid but different inner widths
  // add different numbers to a layer's counters and may not share them)
  ChainBlock &blk = wragw ? chain_block(s, (int)((m + bm - 1) / bm), (c.n + bn - 1) / bn, n, widw_tiles)
                    : widw ? chain_block(s, (int)(m / bm), c.n / bn, n, widw_tiles)
                         : chain_block(s, (int)((m + bm - 1) / bm), (int)(ragw ? (nn + bn - 1) / bn : nn / bn), n);
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
  c.target = ++blk.epoch * (unsigned)blk.tiles_n;
  if (widw || wragw) c.target = blk.epoch; // (the kernel multiplies by the producing layer's column tiles: chain_widths_target / chain_wragged_target)
  if (f32) HIP_OK(launch_f32_chain(tile, c, s));
  else if (d256) {
    c.groups = d256_groups;
    HIP_OK(launch_bf16_dma256_chain(b_kind, c, s));
    g_chain_dma256_stats[1].store(d256_groups, std::memory_order_relaxed);
    g_chain_dma256_stats[2].store(chain_rounds_rounds((int)(m / bm), d256_groups), std::memory_order_relaxed);
    g_chain_dma256_stats[3].store(b_kind, std::memory_order_relaxed);
    g_chain_dma256_stats[0].fetch_add(1, std::memory_order_relaxed);
  }
  else if (wragw) {
    HIP_OK(launch_bf16_chain_wragged(tile, b_kind, c, s));
    g_chain_widths_ragged_stats[1].store((m + bm - 1) / bm, std::memory_order_relaxed);
    g_chain_widths_ragged_stats[2].store((c.n + bn - 1) / bn, std::memory_order_relaxed);
    g_chain_widths_ragged_stats[3].store(blw_variant(tile, b_kind), std::memory_order_relaxed);
    g_chain_widths_ragged_stats[0].fetch_add(1, std::memory_order_relaxed);
  }
  else if (widw && widw_groups > 0) {
    c.groups = widw_groups;
    HIP_OK(launch_bf16_chain_wrounds(tile, b_kind, c, s));
    g_chain_width_rounds_stats[1].store(m / bm, std::memory_order_relaxed);
    g_chain_width_rounds_stats[2].store(widw_groups, std::memory_order_relaxed);
    g_chain_width_rounds_stats[3].store(blw_variant(tile, b_kind), std::memory_order_relaxed);
    g_chain_width_rounds_stats[0].fetch_add(1, std::memory_order_relaxed);
  } else if (widw) {
    HIP_OK(launch_bf16_chain_widths(tile, b_kind, c, s));
    g_chain_widths_stats[1].store(m / bm, std::memory_order_relaxed);
    g_chain_widths_stats[2].store(c.n / bn, std::memory_order_relaxed);
    g_chain_widths_stats[3].store(blw_variant(tile, b_kind), std::memory_order_relaxed);
    g_chain_widths_stats[0].fetch_add(1, std::memory_order_relaxed);
  } else if (ragw) {
    HIP_OK(launch_bf16_chain_ragged(tile, b_kind, c, s));
    g_chain_ragged_stats[1].store((m + bm - 1) / bm, std::memory_order_relaxed);
    g_chain_ragged_stats[2].store((nn + bn - 1) / bn, std::memory_order_relaxed);
    g_chain_ragged_stats[3].store(blw_variant(tile, b_kind), std::memory_order_relaxed);
    g_chain_ragged_stats[0].fetch_add(1, std::memory_order_relaxed);
  } else if (groups > 0) {
    c.groups = groups;
    HIP_OK(launch_bf16_chain(BLW_CHAIN_ROUNDS, tile, b_kind, c, s));
    g_chain_rounds_stats[1].store(groups, std::memory_order_relaxed);
    g_chain_rounds_stats[2].store((m / bm + groups - 1) / groups, std::memory_order_relaxed);
    g_chain_rounds_stats[3].store(blw_variant(tile, b_kind), std::memory_order_relaxed);
    g_chain_rounds_stats[0].fetch_add(1, std::memory_order_relaxed);
  } else if (ragged) {
    HIP_OK(launch_bf16_chain(BLW_CHAIN_EDGE, tile, b_kind, c, s));
    g_chain_edge_stats[1].store((m + bm - 1) / bm, std::memory_order_relaxed);
    g_chain_edge_stats[2].store(nn / bn, std::memory_order_relaxed);
    g_chain_edge_stats[3].store(blw_variant(tile, b_kind), std::memory_order_relaxed);
    g_chain_edge_stats[0].fetch_add(1, std::memory_order_relaxed);
  } else HIP_OK(launch_bf16_chain(BLW_LAYER, tile, b_kind, c, s));
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
