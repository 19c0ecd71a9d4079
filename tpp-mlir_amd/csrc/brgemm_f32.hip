// brgemm_f32.hip - f32 batch-reduce GEMM for gfx950 on v_mfma_f32_32x32x2_f32.
//
// Semantics (reference: xsmm.brgemm / xsmm.fused_brgemm, XsmmOps.td:128-181,281-308;
// runtime/Xsmm/XsmmRunnerUtils.cpp:288-457):
//   C[m x n] = relu?( (beta0 ? 0 : C) + sum_{b<br} A_b[m x k] * B_b[k x n]  (+ bias[n]) )
// row-major, A_b = A + b*stride_a, B_b = B + b*stride_b (elements).
//
// Kernel structure (one workgroup per output tile; no split-K across workgroups,
// so results are deterministic and each element is an f32 fma chain):
//   * workgroup tile (32*WM) x (32*WN), WM*WN*WK waves; each wave owns one 32x32
//     accumulator tile (16 VGPRs) and 1/WK of every K chunk; WK>1 partial sums are
//     combined once through LDS at the end.
//   * the batch-reduce loop IS the K loop: chunk t = (batch t / (k/64), 64 columns of
//     k). A/B panels go HBM -> VGPR (global_load_dwordx4, issued 1.5 chunks ahead)
//     -> LDS (ds_write_b128) -> MFMA fragments, through a 3-slot LDS ring.
//   * ONE barrier per chunk, placed in the MIDDLE of the chunk's MFMA stream: chunk
//     t+1 is published while chunk t still has MFMAs to issue, so no wave ever
//     waits for data at a chunk boundary.
//   * A is stored in LDS as [row][64 k] with the 16-byte column index XOR (row&15):
//     the per-lane ds_read_b128 of 4 consecutive k is bank-conflict free. A lane's
//     4 values feed 4 successive MFMAs; lane-half h therefore covers k = 8q+4h+s at
//     step s (a fixed permutation of k inside each block of 8 - any order is a valid
//     summation order). B is stored [k][n] linear and read with ds_read_b32
//     (conflict free: 32 consecutive columns per lane group).
#include "gemm_common.h"
#include "xsmm_desc.h"
#include "chain_args.h"
#include "gemm_plan.h"
#include "mode_switches.h"
#include "brgemm_f32_lw_kedge.h"
#include "brgemm_bf16_lw_kedge.h"
#include "brgemm_bf16_dma256_edge.h"
#include "brgemm_bf16_skinny_split.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <type_traits>

namespace tpp {

constexpr int BK = 64;     // k columns per chunk
constexpr int NSTAGE = 3;  // LDS ring slots
constexpr int NSET = 3;    // staging register sets = chunks of global loads in flight per lane

typedef __attribute__((address_space(3))) void lds_void_f;

// One LDS-DMA instruction: 64 lanes x 16 bytes from (panel base, per-lane offset) to 1 KiB of the
// dynamic LDS at byte offset lds_off. A plain function on purpose: called from the kernel TEMPLATE with
// template-dependent operands, the builtin made hipcc drop the kernels' host stubs without a diagnostic.
static __device__ __forceinline__ void lds_dma_16B(const void *panel, unsigned lds_off, unsigned voff) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dyn_lds_f32[];
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void *)panel, 0, 0x7fffffff, 0x00020000);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_void_f *)(dyn_lds_f32 + lds_off), 16, voff, 0, 0, 0);
}

// DMA = true: panels go HBM -> LDS directly (buffer_load_dwordx4 ... lds, 1 KiB per wave-instruction):
// no staging registers and no ds_write_b128 (13 LDS cycles each) competing with the fragment reads.
// Chunk t+2 is fetched during the second half of chunk t into the ring slot chunk t-1 has left; the
// A swizzle is applied to the source address. Everything else (fragments, barrier placement,
// epilogue) is shared with the register-staged path.
// items != nullptr: GROUPED mode (tile queue) - the grid is (items, tiles_n, tiles_m) and workgroup
// (x, y, z) computes tile (z, y) of queued invoke x, whose operand pointers and batch count come from
// items[x]; the descriptor fields (m, n, k, leading dimensions, strides, epilogue) are shared.
template <int WM, int WN, int WK, bool DMA>
__global__ __launch_bounds__(64 * WM * WN * WK) void brgemm_f32_fast(GemmArgs p, const WorkItem *__restrict__ items) {
  if (items) { // wave-uniform: overwrite the per-invoke fields of the (by-value) argument block
    const WorkItem it = items[blockIdx.x];
    p.A = it.A; p.B = it.B; p.C = it.C; p.D = it.D; p.br = (int)it.br;
  }
  constexpr int BM = 32 * WM, BN = 32 * WN, NT = 64 * WM * WN * WK;
  constexpr int A_STAGE = BM * BK, B_STAGE = BK * BN; // floats
  constexpr int LA = (BM * BK / 4) / NT, LB = (BK * BN / 4) / NT;
  constexpr int KB_PER_WAVE = 8 / WK;                  // k-blocks (of 8) per wave per chunk
  constexpr int KB_HALF = KB_PER_WAVE / 2;
  constexpr int NP = LA + LB;                          // staging pieces per thread per chunk
  // MFMA slots that carry the LDS writes: they end one step before the barrier so the
  // barrier's lgkmcnt(0) finds them retired
  constexpr int WSLOTS = KB_HALF >= 2 ? 4 * (KB_HALF - 1) : 4 * KB_HALF;
  static_assert(LA >= 1 && LB >= 1 && KB_HALF >= 1, "tile too small for this thread count");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float *As = smem;
  float *Bs = smem + NSTAGE * A_STAGE;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wk = wave / (WM * WN), wmn = wave % (WM * WN), wm = wmn / WN, wn = wmn % WN;
  const int li = lane & 31, lh = lane >> 5;
  // Output tile from the 3-D grid, no divisions (launch_fast picks the shape): XCD-blocked
  // grids are (8, bn, bm): blockIdx.x is the XCD slot (workgroups go to XCDs round-robin in
  // linear-id order, x fastest), and each XCD owns a compact bm x bn block of tiles so the
  // A row-panels / B column-panels it streams are shared in its private L2. Plain grids are
  // (1, tiles_n, tiles_m) with the same formula (blockIdx.x == 0).
  const int tm = items ? (int)blockIdx.z : (int)(blockIdx.x >> 1) * p.tiles_m + (int)blockIdx.z;
  const int tn = items ? (int)blockIdx.y : (int)(blockIdx.x & 1) * p.tiles_n + (int)blockIdx.y;
  const int m0 = tm * BM, n0 = tn * BN;

  const float *__restrict__ A = (const float *)p.A;
  const float *__restrict__ B = (const float *)p.B;
  float *__restrict__ C = (float *)p.C;
  const int kchunks = p.k / BK;
  const int T = p.br * kchunks;

  // ONE accumulator chain per wave: measured +0.9 % on C2 over two, and it is the oracle's summation order
  f32x16 acc; // initialised after the first loads are on their way

  // staging registers of the chunk in flight (HBM -> VGPR -> LDS). Pieces 0..LA-1 are
  // A, LA..LA+LB-1 are B (16 bytes per lane each). The LDS writes of a chunk are spread
  // over the MFMA slots of the FIRST half of the previous chunk's steps and its global
  // loads over the SECOND half, so neither the LDS nor the vector-memory path sees a
  // burst. Loads are buffer loads: wave-uniform 64-bit panel base in the descriptor
  // (advanced by scalar adds once per chunk), per-lane byte offset constant for the
  // whole kernel -> one instruction per 16 bytes, no per-load vector address math.
  f32x4 rs[DMA ? 1 : NSET][NP];
  unsigned voff[NP];
#pragma unroll
  for (int u = 0; u < NP; ++u) {
    if (DMA) {
      // DMA instruction v of this panel fills 1 KiB of the LDS image linearly: lane -> (row, piece)
      // of the image; the source piece of A is XOR-ed with (row & 15) (the read applies it again)
      if (u < LA) {
        const int v = wave * LA + u, row = 4 * v + (lane >> 4), c = lane & 15;
        voff[u] = (unsigned)((row * (int)p.lda + 4 * (c ^ (row & 15))) * 4);
      } else {
        constexpr int RPI = 256 / BN; // B rows per instruction
        const int v = wave * LB + (u - LA), krow = RPI * v + lane / (BN / 4), c = lane % (BN / 4);
        voff[u] = (unsigned)((krow * (int)p.ldb + 4 * c) * 4);
      }
    } else if (u < LA) {
      const int q = tid + u * NT, row = q >> 4, c = q & 15;
      voff[u] = (unsigned)((row * (int)p.lda + 4 * c) * 4);
    } else {
      const int q = tid + (u - LA) * NT, krow = q / (BN / 4), c = q % (BN / 4);
      voff[u] = (unsigned)((krow * (int)p.ldb + 4 * c) * 4);
    }
  }
  // panel base of the chunk being loaded (wave-uniform) and its position in the batch
  const float *gA = A + (int64_t)m0 * p.lda, *gB = B + n0;
  int kc = 0; // chunk index inside the current batch element
  const int64_t dA_wrap = p.stride_a - (int64_t)(kchunks - 1) * BK;
  const int64_t dB_in = (int64_t)BK * p.ldb, dB_wrap = p.stride_b - (int64_t)(kchunks - 1) * BK * p.ldb;
  auto gadvance = [&]() __attribute__((always_inline)) { // next chunk: +64 k inside a batch element, else next batch element
    if (++kc == kchunks) {
      kc = 0;
      gA += dA_wrap;
      gB += dB_wrap;
    } else {
      gA += BK;
      gB += dB_in;
    }
  };
  auto gload_piece = [&](int set, int u) __attribute__((always_inline)) {
    // descriptor built from wave-uniform scalars right at the load (kept in SGPRs)
    const __amdgpu_buffer_rsrc_t r =
        __builtin_amdgcn_make_buffer_rsrc((void *)(u < LA ? gA : gB), 0, 0x7fffffff, 0x00020000);
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, voff[u], 0, 0);
    rs[set][u] = __builtin_bit_cast(f32x4, v);
  };
  auto dma_piece = [&](int stage, int u) __attribute__((always_inline)) {
    if (u < LA) lds_dma_16B(gA, (unsigned)((stage * A_STAGE + (wave * LA + u) * 256) * 4), voff[u]);
    else lds_dma_16B(gB, (unsigned)((NSTAGE * A_STAGE + stage * B_STAGE + (wave * LB + (u - LA)) * 256) * 4), voff[u]);
  };
  auto swrite_piece = [&](int stage, int u) __attribute__((always_inline)) {
    float *as = As + stage * A_STAGE, *bs = Bs + stage * B_STAGE;
    if (u < LA) {
      const int q = tid + u * NT, row = q >> 4, c = q & 15;
      *(f32x4 *)(as + row * BK + ((c ^ (row & 15)) << 2)) = rs[stage][u];
    } else {
      const int q = tid + (u - LA) * NT, krow = q / (BN / 4), c = q % (BN / 4);
      *(f32x4 *)(bs + krow * BN + 4 * c) = rs[stage][u];
    }
  };
  // MFMA fragments of one k-block (8 k): 4 A values (one ds_read_b128) and 4 B values
  // per lane; double-buffered so block q+1 is read while block q multiplies.
  f32x4 fa[2];
  float fb[2][4];
  const int a_off = (wm * 32 + li) * BK, b_off = wn * 32 + li;
  auto frag_load = [&](int buf, int stage, int kb) __attribute__((always_inline)) {
    const float *as = As + stage * A_STAGE + a_off;
    const float *bs = Bs + stage * B_STAGE + b_off;
    fa[buf] = *(const f32x4 *)(as + (((2 * kb + lh) ^ (li & 15)) << 2));
#pragma unroll
    for (int s = 0; s < 4; ++s) fb[buf][s] = bs[(8 * kb + 4 * lh + s) * BN];
  };

  const int kbw = wk * KB_PER_WAVE;
  // One chunk = KB_PER_WAVE k-block steps of 4 MFMAs, ring slot STAGE known at compile
  // time (every LDS address is base VGPR + immediate). Register set s holds the chunk
  // that goes to ring slot s (NSET == NSTAGE). HAS_NEXT: chunk t+1 exists: set STAGE+1
  // is written to slot STAGE+1 during the first half of the steps, then ONE barrier
  // publishes it. HAS_LOAD: chunk t+1+NSET exists: its global loads refill the set just
  // written, during the second half - they have NSET-0.5 chunks of MFMAs to land. The
  // last step prefetches the first fragments of chunk t+1.
  auto chunk = [&](auto stage_c, auto has_next, auto has_load) __attribute__((always_inline)) {
    constexpr int STAGE = decltype(stage_c)::value, NSTG = (STAGE + 1) % NSTAGE;
    constexpr bool HAS_NEXT = decltype(has_next)::value, HAS_LOAD = decltype(has_load)::value;
#pragma unroll
    for (int q = 0; q < KB_PER_WAVE; ++q) {
      const int cur = q & 1, nxt = cur ^ 1;
      if (q + 1 < KB_PER_WAVE) frag_load(nxt, STAGE, kbw + q + 1);
      else if (HAS_NEXT) frag_load(nxt, NSTG, kbw);
      // pin the issue order: the fragment reads of step q+1 stay ABOVE the MFMAs of
      // step q, and each piece of staging work sits in the shadow of one MFMA (the
      // wave is in-order: it idles at the next MFMA until the matrix pipe frees up).
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[cur][s], fb[cur][s], acc, 0, 0, 0);
        if (!DMA && HAS_LOAD && q == 0 && s == 0) {
          // panel base of the next chunk to load: scalar work in the shadow of the MFMA above
          if (++kc == kchunks) {
            kc = 0;
            gA += dA_wrap;
            gB += dB_wrap;
          } else {
            gA += BK;
            gB += dB_in;
          }
        }
#pragma unroll
        for (int u = 0; u < NP; ++u) {
          if (!DMA && HAS_NEXT && (u * WSLOTS) / NP == q * 4 + s) swrite_piece(NSTG, u);
          if (HAS_LOAD && (u * 4 * (KB_PER_WAVE - KB_HALF)) / NP == (q - KB_HALF) * 4 + s) {
            if (DMA) dma_piece((STAGE + 2) % NSTAGE, u); // chunk t+2 into the slot chunk t-1 has left (after the barrier)
            else gload_piece(NSTG, u);
          }
        }
        if (DMA && HAS_LOAD && q == KB_PER_WAVE - 1 && s == 3) {
          if (++kc == kchunks) { // panel base of the chunk after the one just requested
            kc = 0;
            gA += dA_wrap;
            gB += dB_wrap;
          } else {
            gA += BK;
            gB += dB_in;
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      if (q == KB_HALF - 1) {
        // DMA: this wave's pieces of chunk t+1 have landed in the LDS (the fence of __syncthreads
        // does not wait for LDS-DMA), then everybody's
        if (DMA && HAS_NEXT) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
      }
    }
  };
  using yes = std::integral_constant<bool, true>;
  using no = std::integral_constant<bool, false>;
  using S0 = std::integral_constant<int, 0>;
  using S1 = std::integral_constant<int, 1>;
  using S2 = std::integral_constant<int, 2>;
  static_assert(NSET == NSTAGE && NSTAGE == 3, "the chunk schedule below is written for 3 slots / 3 sets");

  // prologue: chunk 0 -> set 0 -> slot 0; chunks 1, 2, 3 -> sets 1, 2, 0 (in flight)
  if (T > 0) { // first thing the kernel does: get chunk 0 moving
#pragma unroll
    for (int u = 0; u < NP; ++u) {
      if (DMA) dma_piece(0, u);
      else gload_piece(0, u);
    }
    if (DMA && T > 1) { // chunk 1 right behind it; afterwards the panel base points at chunk 2
      gadvance();
#pragma unroll
      for (int u = 0; u < NP; ++u) dma_piece(1, u);
      gadvance();
    }
  }
  __builtin_amdgcn_sched_barrier(0);
  // accumulators: wk == 0 starts from C (beta = 1) so the chain is C + sum, as in
  // the reference; other K groups start from zero.
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  // C tile through buffer ops: wave-uniform tile base in the descriptor, per-lane offset
  // constant, the row of accumulator register r as a scalar offset -> one instruction per
  // register, no 64-bit vector address math in the epilogue.
  const int ccol = n0 + wn * 32 + li;
  const __amdgpu_buffer_rsrc_t rsrcC =
      __builtin_amdgcn_make_buffer_rsrc((void *)(C + (int64_t)m0 * p.ldc + n0), 0, 0x7fffffff, 0x00020000);
  const unsigned voffC = (unsigned)(((wm * 32 + 4 * lh) * (int)p.ldc + wn * 32 + li) * 4);
  const unsigned ldcb = (unsigned)((int)p.ldc * 4);
  if (!(p.ep & EP_BETA0) && wk == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r)
      acc[r] = __builtin_bit_cast(
          float, __builtin_amdgcn_raw_buffer_load_b32(rsrcC, voffC, (unsigned)((r & 3) + 8 * (r >> 2)) * ldcb, 0));
  }

  if (!DMA && T > 0) {
#pragma unroll
    for (int c = 1; c <= NSET; ++c) {
      if (c == NSET) { // set 0 is reused for chunk NSET: chunk 0 must be in LDS first
#pragma unroll
        for (int u = 0; u < NP; ++u) swrite_piece(0, u);
      }
      if (c < T) {
        gadvance();
#pragma unroll
        for (int u = 0; u < NP; ++u) gload_piece(c % NSET, u);
      }
    }
  }
  if (DMA) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (T > 0) frag_load(0, 0, kbw);
  int t = 0;
  constexpr int AHEAD = DMA ? 2 : NSET + 1; // chunk t + AHEAD is the one fetched during chunk t
  for (; t + 2 + AHEAD < T; t += 3) { // steady state: three chunks per trip, ring slots 0, 1, 2
    chunk(S0{}, yes{}, yes{});
    chunk(S1{}, yes{}, yes{});
    chunk(S2{}, yes{}, yes{});
  }
  auto tail = [&](auto stage_c) __attribute__((always_inline)) { // last chunks: same bodies minus what no longer exists
    const int left = T - t;
    if (left > AHEAD) chunk(stage_c, yes{}, yes{});
    else if (left >= 2) chunk(stage_c, yes{}, no{});
    else chunk(stage_c, no{}, no{});
    ++t;
  };
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    if (t < T) tail(S0{});
    if (t < T) tail(S1{});
    if (t < T) tail(S2{});
  }

  if constexpr (WK > 1) {
    // combine the K groups through LDS: group g>0 parks its 32x32 partial, group 0 adds
    __syncthreads();
    float *red = smem; // (WK-1) * WM*WN * 16 * 64 floats, fits in the ring
    if (wk > 0) {
      float *dst = red + ((wk - 1) * (WM * WN) + wmn) * 1024 + lane;
#pragma unroll
      for (int r = 0; r < 16; ++r) dst[r * 64] = acc[r];
    }
    __syncthreads();
    if (wk > 0) return;
#pragma unroll
    for (int g = 1; g < WK; ++g) {
      const float *src = red + ((g - 1) * (WM * WN) + wmn) * 1024 + lane;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] += src[r * 64];
    }
  }

  const float bias = (p.ep & EP_BIAS) ? ((const float *)p.D)[ccol] : 0.0f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float v = acc[r] + bias;
    if (p.ep & EP_RELU) v = v > 0.0f ? v : 0.0f;
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rsrcC, voffC,
                                          (unsigned)((r & 3) + 8 * (r >> 2)) * ldcb, C_STORE_AUX);
  }
}

// ---- grouped kernel: many invokes of one small-tile descriptor in ONE launch ----------
// The compiler's native call pattern is hundreds of invokes per layer on 32x32x32 tiles with
// batch 32 from OpenMP workers (test/Passes/pass-convert-mlp-to-parallel-tile.mlir:80-88); one
// GPU launch per invoke would be pure launch latency. The runtime's tile queue (runtime.cpp)
// collects such invokes and runs them here: grid = (32x32 tiles per item, items), one
// workgroup of 4 waves per tile; wave w takes the K chunks (32 k of one batch element)
// c = w, w+4, ... so all four SIMDs of a CU work on the tile, each with a private
// double-buffered LDS panel pair (no workgroup barrier in the K loop); the four partial
// accumulators are combined through LDS once. It is also the GENERIC kernel of the runtime
// (items == nullptr: one invoke described by the arguments themselves): any m/n/k/ld and
// alignment, f32 or bf16 storage (elements are widened to f32 on the way into LDS, bf16 x
// bf16 products are exact in f32, accumulation is f32 - the reference's "f32 compute for
// bf16" rule, XsmmRunnerUtils.cpp:127-129 - one rounding at the store), flat or VNNI-2 B.
// VEC selects 16-byte loads when shape, strides and pointers allow.
// FORM (f32, flat B): an operand is the SOURCE of a transpose the runtime folded into this gemm (rt_rewrites.h, mode 2 of
// xsmm_hip_set_fold_transpose) and is read transposed. The two operands then swap their staging and LDS image, nothing else:
//   FORM_BT  B[k][j] = src[j * ldb + k] is contiguous in k like a row of A: the 32 j-rows x 32 k of a chunk are loaded, clamped, cut off
//            at k and laid out in LDS exactly as the A panel is, and a lane's fragment - four consecutive k of column li - is ONE
//            16-byte read instead of four 4-byte reads 128 bytes apart;
//   FORM_AT  A[i][k] = src[k * lda + i] is contiguous in m like a row of B: the 32 k-rows x 32 m of a chunk are staged and laid out
//            as the B panel is (4-row pieces of m, a piece at or beyond m clamped to piece 0), a lane's fragment is four 4-byte reads
//            one k-row apart.
// The LDS footprint, the order of the MFMAs and the value each MFMA sees are those of the element path (VEC = false: FORM_AT by the
// index expression below, a transposed B by the run-time branch on p.b_trans of the FORM_NONE instance): the same bits come out.
constexpr int GK = 32; // k per chunk of the grouped kernel
enum : int { FORM_NONE = 0, FORM_BT = 1, FORM_AT = 2 };

template <typename T, bool VNNI, bool VEC, int VF = 2, int FORM = FORM_NONE>
__global__ __launch_bounds__(256) void brgemm_grouped(GemmArgs p, const WorkItem *__restrict__ items) {
  static_assert(FORM == FORM_NONE || (sizeof(T) == 4 && !VNNI), "transposed operands: f32, flat B");
  static_assert(FORM != FORM_BT || VEC, "a transposed B on element loads is the FORM_NONE instance (p.b_trans)");
  extern __shared__ __attribute__((aligned(16))) float smem_g[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const WorkItem it = items ? items[blockIdx.y] : WorkItem{p.A, p.B, p.C, p.D, (int64_t)p.br};
  g_cvoid *gA = (g_cvoid *)it.A, *gB = (g_cvoid *)it.B, *gD = (g_cvoid *)it.D; // global, not flat, accesses
  g_void *gC = (g_void *)it.C;


  const int tm = blockIdx.x / p.tiles_n, tn = blockIdx.x % p.tiles_n;
  const int m0 = tm * 32, n0 = tn * 32;
  const int kchunks = (p.k + GK - 1) / GK;
  const int nchunk = (int)it.br * kchunks;
  // per-wave LDS: 2 buffers x (A 32x32 + B 32x32) floats
  float *wl = smem_g + wave * (2 * 2 * 32 * GK);

  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;

  // staging registers: A tile rows [m0, m0+32) x k [kk0, kk0+32); B tile k x n
  // two staging register sets: 32 x 32 floats = 256 pieces of 16 B per panel, 4 per lane and panel
  f32x4 rs[2][2][4];
  // f32 with 16-byte loads (the compiler-native packed 32x32x32 tiles): per-lane byte offsets inside a chunk, fixed for the kernel.
  // Rows / 4-column pieces beyond a ragged edge (m not a multiple of 32, n only of 4, e.g. --tiles=64,48,64) are loaded from
  // a CLAMPED address and left as they are: an output element depends on its own A row and B column only, and the
  // epilogue stores nothing beyond the edge.
  unsigned voffA[4] = {0, 0, 0, 0}, voffB[4] = {0, 0, 0, 0};
  if constexpr (VEC && sizeof(T) == 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = lane + 64 * u, row = q >> 3, c4 = q & 7; // 32 rows x 8 pieces of 4 floats
      // offsets are relative to the TILE (the 64-bit descriptor base carries m0 * lda and n0): 32 rows x ld x 4 B stays below
      // 2^31 for every ld the launcher admits (< 2^24), whatever m is - an absolute row here would wrap past 2 GiB of A
      const int a_row = m0 + row < p.m ? row : p.m - 1 - m0, b_col = n0 + 4 * c4 < p.n ? 4 * c4 : 0;
      if constexpr (FORM == FORM_AT) { // k-row `row`, rows m0 + 4 c4 .. + 3 of the tile
        const int a_col = m0 + 4 * c4 < p.m ? 4 * c4 : 0;
        voffA[u] = (unsigned)((row * (int)p.lda + a_col) * 4);
      } else {
        voffA[u] = (unsigned)((a_row * (int)p.lda + 4 * c4) * 4);
      }
      if constexpr (FORM == FORM_BT) { // column n0 + row (clamped like a row of A), k piece c4
        const int b_row = n0 + row < p.n ? row : p.n - 1 - n0;
        voffB[u] = (unsigned)((b_row * (int)p.ldb + 4 * c4) * 4);
      } else {
        voffB[u] = (unsigned)((row * (int)p.ldb + b_col) * 4);
      }
    }
  }
  // live = false: the chunk does not exist. The f32 16-byte path then still ISSUES its loads, switched off through the buffer
  // descriptor (num_records = 0, no memory traffic): a branch around a load makes hipcc wait with vmcnt(0) at the next use of
  // ANY staged register, which would serialise the two chunks kept in flight.
  auto gload = [&](int c, int set, bool live) __attribute__((always_inline)) {
    f32x4(&ra)[4] = rs[set][0];
    f32x4(&rb)[4] = rs[set][1];
    const int b = c / kchunks, kk0 = (c - b * kchunks) * GK;
    const int64_t abase = (int64_t)b * p.stride_a, bbase = (int64_t)b * p.stride_b;
    if constexpr (VEC && sizeof(T) == 4) {
      const int nrec = __builtin_amdgcn_readfirstlane(live ? 0x7fffffff : 0);
      // the chunk of this tile as the operand lies in memory: rows m0.. x k kk0.. of A (FORM_AT: k-rows kk0.. x m0..), k-rows kk0.. x
      // columns n0.. of B (FORM_BT: rows n0.. x k kk0..)
      constexpr bool AT = FORM == FORM_AT, BT = FORM == FORM_BT;
      const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc(
          (void *)((const float *)it.A + abase + (int64_t)(AT ? kk0 : m0) * p.lda + (AT ? m0 : kk0)), 0, nrec, 0x00020000);
      const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc(
          (void *)((const float *)it.B + bbase + (int64_t)(BT ? n0 : kk0) * p.ldb + (BT ? kk0 : n0)), 0, nrec, 0x00020000);
      // k need only be a multiple of 4: in the last chunk of a batch element the 16-byte pieces at or beyond k (A: k piece c4, B: k
      // row) are requested at an offset past the descriptor's end and come back as zeros - no branch, no select on loaded data
      const int klim = p.k - kk0; // >= 32 in every chunk but a ragged last one
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int q = lane + 64 * u;
        // (k runs along the pieces of a row of A and of a transposed B, along the rows of B and of a transposed A)
        const unsigned oa = (AT ? (q >> 3) : 4 * (q & 7)) < klim ? voffA[u] : 0x80000000u, ob = (BT ? 4 * (q & 7) : (q >> 3)) < klim ? voffB[u] : 0x80000000u;
        ra[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rA, oa, 0, 0));
        rb[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rB, ob, 0, 0));
      }
      return;
    }
    if (!live) return;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = lane + 64 * u, row = q >> 3, c4 = q & 7; // 32 rows x 8 pieces of 4 floats
      { // element-wise loads: any shape, stride and alignment
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int gr = m0 + row, gk = kk0 + 4 * c4 + e;
          // (FORM_AT: element [gr][gk] of A is element [gk][gr] of the transpose's source)
          ra[u][e] = (gr < p.m && gk < p.k) ? Elem<T>::load(gA, abase + (FORM == FORM_AT ? (int64_t)gk * p.lda + gr : (int64_t)gr * p.lda + gk)) : 0.0f;
          const int bk = kk0 + row, bj = n0 + 4 * c4 + e;
          float v = 0.0f;
          if (bk < p.k && bj < p.n) {
            // VNNI-v B [k/v][ldb][v] (v = p.vf: 2 or 4; the oracle's b_index)
            // (b_trans: the operand is the SOURCE of a transpose the runtime folded into this gemm - element [bk][bj] of B is
            // element [bj][bk] of the source)
            const int64_t idx = VNNI ? (int64_t)(bk / p.vf) * (p.vf * p.ldb) + p.vf * (int64_t)bj + (bk % p.vf)
                                     : p.b_trans ? (int64_t)bj * p.ldb + bk : (int64_t)bk * p.ldb + bj;
            v = Elem<T>::load(gB, bbase + idx);
          }
          rb[u][e] = v;
        }
      }
    }
  };
  // piece u (one A quad + one B quad per lane) of staging set `set` into LDS buffer `buf`
  auto swrite_piece = [&](int buf, int set, int u) __attribute__((always_inline)) {
    f32x4(&ra)[4] = rs[set][0];
    f32x4(&rb)[4] = rs[set][1];
    float *as = wl + buf * (2 * 32 * GK), *bs = as + 32 * GK;
    const int q = lane + 64 * u;
    const int row = q >> 3, krow = row, c4 = q & 7, c4b = c4;
    // (16-byte loads of a transposed operand arrive in the OTHER operand's shape and keep it: see FORM above)
    if constexpr (VEC && FORM == FORM_AT) *(f32x4 *)(as + krow * 32 + 4 * c4b) = ra[u];
    else *(f32x4 *)(as + row * GK + ((c4 ^ ((row >> 1) & 7)) << 2)) = ra[u]; // 128-byte rows: XOR on (row>>1)
    if constexpr (VEC && FORM == FORM_BT) *(f32x4 *)(bs + row * GK + ((c4 ^ ((row >> 1) & 7)) << 2)) = rb[u];
    else *(f32x4 *)(bs + krow * 32 + 4 * c4b) = rb[u];
  };
  auto swrite = [&](int buf, int set) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < 4; ++u) swrite_piece(buf, set, u);
  };
  // The 16 MFMAs of the chunk in LDS buffer `buf`, software-pipelined: the fragments of k-block kb + 1 are read while the four
  // MFMAs of k-block kb run, and (stage) the staging set `set` = the NEXT chunk of this wave goes into the other LDS buffer one
  // piece per k-block - a wave is alone on its SIMD here, so whatever is not overlapped inside the wave is idle matrix-core time
  // (before: 2300 cycles per chunk for 1024 cycles of MFMA).
  auto compute = [&](int buf, bool stage, int set) __attribute__((always_inline)) {
    constexpr bool A_ROWS = !(VEC && FORM == FORM_AT), B_ROWS = VEC && FORM == FORM_BT; // image = 128-byte rows of k (else k-rows of 32)
    const float *as = wl + buf * (2 * 32 * GK) + (A_ROWS ? li * GK : li), *bs = wl + buf * (2 * 32 * GK) + 32 * GK + (B_ROWS ? li * GK : li);
    f32x4 a4[2];
    float b4[2][4];
    auto frag = [&](int kb, int to) __attribute__((always_inline)) {
      if constexpr (A_ROWS) a4[to] = *(const f32x4 *)(as + (((2 * kb + lh) ^ ((li >> 1) & 7)) << 2));
      else {
#pragma unroll
        for (int s = 0; s < 4; ++s) a4[to][s] = as[(8 * kb + 4 * lh + s) * 32];
      }
      if constexpr (B_ROWS) {
        const f32x4 b = *(const f32x4 *)(bs + (((2 * kb + lh) ^ ((li >> 1) & 7)) << 2));
#pragma unroll
        for (int s = 0; s < 4; ++s) b4[to][s] = b[s];
      } else {
#pragma unroll
        for (int s = 0; s < 4; ++s) b4[to][s] = bs[(8 * kb + 4 * lh + s) * 32];
      }
    };
    frag(0, 0);
#pragma unroll
    for (int kb = 0; kb < GK / 8; ++kb) {
      if (kb + 1 < GK / 8) frag(kb + 1, (kb + 1) & 1);
      if (stage) swrite_piece(buf ^ 1, set, kb);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s = 0; s < 4; ++s)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[kb & 1][s], b4[kb & 1][s], acc, 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  // wave-private pipeline, TWO chunks of loads in flight: while chunk c multiplies out of LDS buffer i & 1, chunk c + 4 sits in
  // (or is on its way to) register set (i + 1) & 1 and the loads of chunk c + 8 are issued into set i & 1. With one chunk in
  // flight a wave waited out most of an L2 round trip per chunk (0.5 us of MFMA against 0.6-0.8 us of latency): the tile-queue
  // launches of the reference's 32x32x32 pattern took 12.7 us per 256 tiles against 7.4 us for the whole-layer kernel.
  // The loop runs whole PAIRS of chunks (one per staging set / LDS buffer) with ONE exit and no branch inside: loads of chunks
  // that do not exist are switched off (f32 16-byte path) and staging them moves zeros / stale registers into an LDS
  // buffer nobody computes from. (With an exit per chunk hipcc keeps the accumulator in two register sets and moves it -
  // 16 v_accvgpr_read + 16 v_accvgpr_write behind every chunk's last MFMA; a branch around loads defeats the counted waits.)
  const int mine = nchunk > wave ? (nchunk - wave + 3) >> 2 : 0; // chunks of this wave: wave, wave + 4, ...
  int c = wave;
  if constexpr (sizeof(T) == 2 && VNNI && VEC) {
    // bf16 + VNNI-2 B with 16-byte loads (ragged bf16 tiles, e.g. mlir-gen --tiles=64,48,64 --vnni=2): the panels stay bf16 in
    // LDS and the chunk is TWO v_mfma_f32_32x32x16_bf16 (f32 accumulate, the arithmetic of the other bf16 kernels) instead of
    // sixteen f32 MFMAs on widened operands. Same pipeline: two chunks of loads in flight, switched off past the stream's end.
    //   A image [32 rows][32 k] bf16, row pitch 80 B (16-byte fragment reads of 16 consecutive rows hit 16 different bank quads);
    //   B image = the 16 VNNI pair-rows x 32 columns as they are (a lane's fragment: 4 dwords one pair-row apart).
    typedef __bf16 bf16x8_g __attribute__((ext_vector_type(8)));
    constexpr int APITCH = 80, ABYTES = 32 * APITCH, BUFB = ABYTES + 16 * 128;
    unsigned char *wlb = (unsigned char *)smem_g + wave * 16384;
    unsigned vA[2], vB[2];
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int q = lane + 64 * v;
      // tile-relative (see the f32 path): the descriptor base carries m0 * lda and 2 * n0
      // B: a 16-byte piece = 4 columns x 2 k (VNNI-2: 16 pair-rows of 128 B) or 2 columns x 4 k (VNNI-4: 8 k-group rows of 256 B)
      constexpr int CPP = 8 / VF, PPR = 32 / CPP; // columns per piece, pieces per row of the 32-column panel
      const int a_row = m0 + (q >> 2) < p.m ? (q >> 2) : p.m - 1 - m0, b_col = n0 + CPP * (q % PPR) < p.n ? CPP * (q % PPR) : 0;
      vA[v] = (unsigned)((a_row * (int)p.lda + 8 * (q & 3)) * 2);
      vB[v] = (unsigned)(((q / PPR) * VF * (int)p.ldb + VF * b_col) * 2);
    }
    u32x4 sa[2][2], sb[2][2];
    auto gload_bf = [&](int cc, int set, bool live) __attribute__((always_inline)) {
      const int b = cc / kchunks, kk0 = (cc - b * kchunks) * GK;
      const int nrec = __builtin_amdgcn_readfirstlane(live ? 0x7fffffff : 0);
      const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc(
          (void *)((const unsigned short *)it.A + (int64_t)b * p.stride_a + (int64_t)m0 * p.lda + kk0), 0, nrec, 0x00020000);
      const __amdgpu_buffer_rsrc_t rB = __builtin_amdgcn_make_buffer_rsrc(
          (void *)((const unsigned short *)it.B + (int64_t)b * p.stride_b + (int64_t)(kk0 / VF) * (VF * p.ldb) + VF * (int64_t)n0), 0, nrec, 0x00020000);
#pragma unroll
      for (int v = 0; v < 2; ++v) {
        sa[set][v] = __builtin_amdgcn_raw_buffer_load_b128(rA, vA[v], 0, 0);
        sb[set][v] = __builtin_amdgcn_raw_buffer_load_b128(rB, vB[v], 0, 0);
      }
    };
    auto swrite_bf = [&](int buf, int set, int v) __attribute__((always_inline)) {
      const int q = lane + 64 * v;
      unsigned char *ab = wlb + buf * BUFB;
      *(u32x4 *)(ab + (q >> 2) * APITCH + (q & 3) * 16) = sa[set][v];
      *(u32x4 *)(ab + ABYTES + q * 16) = sb[set][v]; // (the rows follow each other: [16][128 B] or [8][256 B], both = piece q at 16 q)
    };
    auto compute_bf = [&](int buf, bool stage, int set) __attribute__((always_inline)) {
      const unsigned char *ab = wlb + buf * BUFB;
      bf16x8_g af[2];
      u32x4 bfr[2];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        af[ks] = *(const bf16x8_g *)(ab + li * APITCH + (2 * ks + lh) * 16);
        if constexpr (VF == 4) { // k-groups 4 ks + 2 lh and + 1 of this lane's column: two 8-byte pieces
          typedef unsigned int u32x2_g __attribute__((ext_vector_type(2)));
          const u32x2_g q0 = *(const u32x2_g *)(ab + ABYTES + (4 * ks + 2 * lh) * 256 + li * 8);
          const u32x2_g q1 = *(const u32x2_g *)(ab + ABYTES + (4 * ks + 2 * lh + 1) * 256 + li * 8);
          bfr[ks] = u32x4{q0[0], q0[1], q1[0], q1[1]};
        } else {
#pragma unroll
          for (int t = 0; t < 4; ++t) bfr[ks][t] = *(const unsigned int *)(ab + ABYTES + (8 * ks + 4 * lh + t) * 128 + li * 4);
        }
      }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        if (stage) swrite_bf(buf ^ 1, set, ks);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ks], __builtin_bit_cast(bf16x8_g, bfr[ks]), acc, 0, 0, 0);
      }
    };
    gload_bf(c, 0, mine > 0);
    gload_bf(c + 4, 1, mine > 1);
    if (mine > 0) {
      swrite_bf(0, 0, 0);
      swrite_bf(0, 0, 1);
    }
    for (int i = 0; i + 1 < mine; i += 2) {
      gload_bf(c + 8, 0, i + 2 < mine);
      compute_bf(0, true, 1);
      gload_bf(c + 12, 1, i + 3 < mine);
      compute_bf(1, true, 0);
      c += 8;
    }
    if (mine & 1) compute_bf(0, false, 0);
  } else {
    gload(c, 0, mine > 0);
    gload(c + 4, 1, mine > 1);
    if (mine > 0) swrite(0, 0);
    for (int i = 0; i + 1 < mine; i += 2) {
      gload(c + 8, 0, i + 2 < mine);
      compute(0, true, 1);
      gload(c + 12, 1, i + 3 < mine);
      compute(1, true, 0);
      c += 8;
    }
    if (mine & 1) compute(0, false, 0);
  }
  // combine the four waves' partial sums: every wave parks all of its 16 accumulator registers, then wave w finishes the four
  // registers 4w .. 4w+3 (rows 8w + 4 lh + 0..3 of the tile): a quarter of the reads and stores per wave (one wave doing all of
  // it kept the other three idle for the whole tail). Summation order as before: wave 0 + wave 1 + wave 2 + wave 3, (+ C), + bias.
  __syncthreads();
  float *red = smem_g;
#pragma unroll
  for (int r = 0; r < 16; ++r) red[wave * 1024 + r * 64 + lane] = acc[r];
  __syncthreads();
  const int col = n0 + li;
  const float bias = ((p.ep & EP_BIAS) && col < p.n) ? Elem<T>::load(gD, col) : 0.0f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = 4 * wave + j;
    const int row = m0 + 4 * lh + j + 8 * wave;
    float v = red[r * 64 + lane];
#pragma unroll
    for (int g = 1; g < 4; ++g) v += red[g * 1024 + r * 64 + lane];
    if (row < p.m && col < p.n) {
      // C element (row, col): row-major, or VNNI-2 [m/2][n][2] (wire flag 8192, see the oracle's c_index)
      const int64_t ci = (p.ep & EP_VNNI_C) ? (int64_t)(row >> 1) * (2 * p.ldc) + 2 * (int64_t)col + (row & 1)
                                            : (int64_t)row * p.ldc + col;
      if (!(p.ep & EP_BETA0)) v += Elem<T>::load((g_cvoid *)gC, ci);
      v += bias;
      if (p.ep & EP_RELU) v = v > 0.0f ? v : 0.0f;
      Elem<T>::store(gC, ci, v);
    }
  }
}

// ---- host side: carrying out the plans of gemm_plan.cpp ---------------------------------------------------------------------------
template <int WM, int WN, int WK, bool DMA>
static hipError_t launch_fast(const GemmArgs &a, hipStream_t s) {
  constexpr int BM = 32 * WM, BN = 32 * WN, NT = 64 * WM * WN * WK;
  constexpr size_t lds = (size_t)NSTAGE * (BM * BK + BK * BN) * sizeof(float);
  static std::atomic<unsigned long long> lds_set{0};
  if (hipError_t e = ensure_dynamic_lds((const void *)brgemm_f32_fast<WM, WN, WK, DMA>, (int)lds, lds_set); e != hipSuccess) return e;
  GemmArgs args = a;
  const int tiles_m = a.m / BM, tiles_n = a.n / BN;
  dim3 grid;
  if ((tiles_m & 3) == 0 && (tiles_n & 1) == 0 && tiles_m / 4 <= 65535 && tiles_n / 2 <= 65535) {
    args.tiles_m = tiles_m / 4; // XCD-blocked: 4 (M) x 2 (N) XCD blocks of tiles_m/4 x tiles_n/2 tiles
    args.tiles_n = tiles_n / 2;
    grid = dim3(8, args.tiles_n, args.tiles_m);
  } else {
    args.tiles_m = args.tiles_n = 0;
    if (tiles_m > 65535 || tiles_n > 65535) return hipErrorInvalidValue;
    grid = dim3(1, tiles_n, tiles_m);
  }
  hipLaunchKernelGGL((brgemm_f32_fast<WM, WN, WK, DMA>), grid, dim3(NT), lds, s, args, (const WorkItem *)nullptr);
  return hipGetLastError();
}

hipError_t launch_gemm_bf16_fast(int tile, const GemmArgs &a, hipStream_t s); // brgemm_bf16.hip
hipError_t launch_bf16_dma256_image(int b_kind, const GemmArgs &a, hipStream_t s); // brgemm_bf16_dma256.hip
hipError_t launch_bf16_dma256_edge(int b_kind, const GemmArgs &a, hipStream_t s); // brgemm_bf16_dma256_edge.hip: m or n not a multiple of 256; hipErrorInvalidValue: not launched
hipError_t launch_bf16_skinny(int b_kind, int bn, const GemmArgs &a, hipStream_t s); // brgemm_bf16_skinny.hip: 1 <= m <= 31 on column blocks of bn; hipErrorInvalidValue: not launched
hipError_t launch_bf16_skinny_split(int b_kind, int bn, int parts, const GemmArgs &a, hipStream_t s); // brgemm_bf16_skinny_split.hip: the same over parts workgroups per column block; hipErrorInvalidValue: not launched
hipError_t launch_f32_lw(int tile, const GemmArgs &a, hipStream_t s);         // brgemm_f32_lw.hip (tile 4: 128x64, forced variant 10 only - it measures within 2 % of brgemm_f32_fast<128x64>)
hipError_t launch_f32_lw_grouped(int tile, const GemmArgs &a, const WorkItem *items, int n_items, int split, hipStream_t s);
hipError_t launch_f32_lw_split(int tile, const GemmArgs &a, int split, hipStream_t s); // hipErrorOutOfMemory / InvalidValue: not launched
hipError_t launch_f32_lw_tail(int tile, const GemmArgs &a, int tail_tiles, int split, hipStream_t s); // the same
hipError_t launch_f32_lw_halves(const GemmArgs &a, hipStream_t s); // tile 1 as two 64x32 + K2 workgroups per tile, the same bits; hipErrorInvalidValue: not launched
hipError_t launch_f32_lw_edge(int tile, const GemmArgs &a, hipStream_t s); // m or n not a multiple of the tile; hipErrorInvalidValue: not launched
hipError_t launch_f32_lw_kedge(int tile, const GemmArgs &a, hipStream_t s); // k a multiple of 8 but not of 64 (m, n ragged or not); hipErrorInvalidValue: not launched
hipError_t launch_f32_lw16(int tile, const GemmArgs &a, const WorkItem *items, int n_items, bool grouped, hipStream_t s); // brgemm_f32_lw16.hip: tile 0 = 32x16
hipError_t launch_f32_x6(int tile, const GemmArgs &a, bool vec, hipStream_t s); // brgemm_f32_x6.hip: tile = variant - V_F32_X6_64x64
hipError_t launch_bf16_grouped64(const GemmArgs &a, const WorkItem *items, int n_items, hipStream_t s); // brgemm_bf16.hip
hipError_t launch_bf16_small32(const GemmArgs &a, const WorkItem *items, int n_items, hipStream_t s, int split = 1, bool *split_ran = nullptr); // brgemm_bf16_small.hip

template <typename T, bool VNNI, bool VEC, int VF = 2, int FORM = FORM_NONE>
static hipError_t launch_grouped_t(const GemmArgs &a, const WorkItem *items, int n_items, hipStream_t s) {
  constexpr size_t lds = 4 * 2 * 2 * 32 * GK * sizeof(float); // 64 KiB: 4 waves x 2 buffers x (A + B)
  auto kern = brgemm_grouped<T, VNNI, VEC, VF, FORM>;
  static std::atomic<unsigned long long> lds_set{0};
  if (hipError_t e = ensure_dynamic_lds((const void *)kern, (int)lds, lds_set); e != hipSuccess) return e;
  GemmArgs args = a;
  args.tiles_m = (a.m + 31) / 32;
  args.tiles_n = (a.n + 31) / 32;
  for (int done = 0; done < n_items; done += 65535) { // gridDim.y limit
    const int n = n_items - done < 65535 ? n_items - done : 65535;
    hipLaunchKernelGGL(kern, dim3(args.tiles_m * args.tiles_n, n), dim3(256), lds, s, args, items ? items + done : items);
  }
  return hipGetLastError();
}

// xsmm_hip_force_split / TPP_HIP_SPLIT: 0 / 1 = never split, n > 1 = always n (clamped to the chunks), -1 = the split model (gemm_plan.cpp)
static std::atomic<int> g_forced_split{[] {
  const char *e = getenv("TPP_HIP_SPLIT");
  return e ? atoi(e) : -1;
}()};
int force_gemm_split(int v) { return g_forced_split.exchange(v < -1 ? -1 : v); }
static std::atomic<int> g_strict_kernels{0};
int set_strict_kernels(int on) { return g_strict_kernels.exchange(on != 0); }
bool strict_kernels() { return g_strict_kernels.load(std::memory_order_relaxed) != 0; }
static GemmPlanEnv gemm_plan_env() {
  return gemm_plan_env_of(device_cu_count(), strict_kernels(), g_forced_split.load(std::memory_order_relaxed)); // (the switches: mode_switches.h)
}
bool plan_gemm(GemmDesc &d, int forced_variant) { return plan_gemm(d, forced_variant, gemm_plan_env()); }
bool gemm_quads_pay(const GemmDesc &d, int n_items, int64_t br) { return gemm_quads_pay(d, n_items, br, gemm_plan_env()); }

// name of the kernel family of the most recent grouped GEMM launch (xsmm_hip_last_grouped_kernel: tests and tools/tpp_replay
// report which kernel a tile-queue group ran on - the descriptor's own name is what a SINGLE invoke would run on)
static std::atomic<const char *> g_last_grouped{""};
const char *last_grouped_kernel() { return g_last_grouped.load(std::memory_order_relaxed); }
// the same for single launches whose kernel was refined at INVOKE time (the batch count arrives with the invoke): "" = the
// descriptor's own kernel (xsmm_hip_kernel_name) ran
static std::atomic<const char *> g_last_refined{""};
const char *last_refined_kernel() { return g_last_refined.load(std::memory_order_relaxed); }

static GemmArgs gemm_args(const GemmDesc &d, const void *A, const void *B, void *C, const void *D, int br) {
  GemmArgs a;
  a.A = A; a.B = B; a.C = C; a.D = D;
  a.lda = d.lda; a.ldb = d.ldb; a.ldc = d.ldc; a.stride_a = d.stride_a; a.stride_b = d.stride_b;
  a.m = (int)d.m; a.n = (int)d.n; a.k = (int)d.k; a.br = br;
  a.ep = (d.beta0 ? EP_BETA0 : 0) | (d.bias ? EP_BIAS : 0) | (d.relu ? EP_RELU : 0) | (d.vnni_c ? EP_VNNI_C : 0);
  a.tiles_m = a.tiles_n = 0;
  a.vf = d.vnni_factor ? d.vnni_factor : 2;
  a.split = 0; a.scratch = nullptr; a.split_cnt = nullptr;
  a.b_trans = d.b_trans;
  a.tail_body = 0;
  return a;
}
// the one-layer ChainArgs of the bf16 loader-wave launchers (brgemm_bf16_lw.hip); br: the batch count (grouped: the first item's), m x n:
// the output (of one item, grouped; of a 2 x 2 block of items, quads)
static ChainArgs one_layer(const GemmArgs &a, int br, int m, int n) {
  ChainArgs c;
  memset(&c, 0, sizeof(c));
  c.A = a.A, c.lda = a.lda, c.m = m, c.n = n, c.nlayers = 1;
  c.L[0] = ChainLayer{a.B, a.D, a.C, a.ldb, a.ldc, a.stride_a, a.stride_b, a.k, br, a.ep, 0};
  return c;
}

// carries out a plan of gemm_plan.cpp. items / n_items: the work list (WorkItem, QuadItem for quads; nullptr and 1 for a single
// invoke); br: the batch count of the loader-wave bf16 launches (a group's: the first item's)
static hipError_t run_gemm_launch(const GemmLaunch &p, const GemmArgs &a, int br, const void *items, int n_items, bool grouped, hipStream_t s,
                                  bool *small_split_ran = nullptr) {
  const WorkItem *wi = (const WorkItem *)items;
  switch (p.launcher) {
  case GL_NONE: return hipSuccess;
  case GL_INVALID: return hipErrorInvalidValue;
  // LDS-DMA panels for every tile but the smallest: measured C2 +3 %, C3 +8 %, 4096^3 +3 %, 3 x 1024 MLP
  // at batch 512 / 1024 +5 % / +3 % over register staging. 32x32 tiles with 4 K-split waves have
  // 512-cycle chunks and short kernels: in a chain of dependent layers (3 x 1024 MLP, batch 256) the DMA
  // path's 2-chunk lead and slower prologue (an LDS-DMA instruction takes ~60 cycles to issue) cost more
  // than the ds_write path saves (32.4 vs 29.2 us); deeper rings (5-6 slots) made the prologue worse.
  case GL_F32_FAST:
    switch (p.tile) {
    case V_F32_64x64: return launch_fast<2, 2, 1, true>(a, s);
    case V_F32_64x32K2: return launch_fast<2, 1, 2, true>(a, s);
    case V_F32_32x32K4: return launch_fast<1, 1, 4, false>(a, s);
    case V_F32_128x64: return launch_fast<4, 2, 1, true>(a, s);
    case V_F32_64x64K2: return launch_fast<2, 2, 2, true>(a, s);
    default: return hipErrorInvalidValue;
    }
  case GL_F32_LW: return p.edge_k ? launch_f32_lw_kedge(p.tile, a, s) : p.edge ? launch_f32_lw_edge(p.tile, a, s) : launch_f32_lw(p.tile, a, s);
  case GL_F32_LW16: return launch_f32_lw16(p.tile, a, wi, n_items, grouped, s);
  case GL_F32_LW_GROUPED: return launch_f32_lw_grouped(p.tile, a, wi, n_items, p.split, s);
  case GL_F32_X6: return launch_f32_x6(p.tile, a, p.vec, s);
  case GL_BF16_FAST:
    if (p.edge) return p.tile == 2 ? launch_bf16_dma256_edge(p.b_kind, a, s) : hipErrorInvalidValue;
    return p.b_kind != 0 ? (p.tile == 2 ? launch_bf16_dma256_image(p.b_kind, a, s) : hipErrorInvalidValue) : launch_gemm_bf16_fast(p.tile, a, s);
  case GL_BF16_SKINNY: return p.split > 1 ? launch_bf16_skinny_split(p.b_kind, p.tile, p.split, a, s) : launch_bf16_skinny(p.b_kind, p.tile, a, s);
  case GL_BF16_SMALL32: return launch_bf16_small32(a, wi, n_items, s, p.split, small_split_ran);
  case GL_BF16_GROUPED64: return launch_bf16_grouped64(a, wi, n_items, s);
  case GL_BF16_LW:
    return launch_bf16_lw(p.edge_k8 ? BLW_KEDGE8 : p.edge_k ? BLW_KEDGE : p.edge ? BLW_EDGE : BLW_LAYER, p.tile, p.b_kind, one_layer(a, br, a.m, a.n), s);
  case GL_BF16_LW_GROUPED: return launch_bf16_lw_grouped(p.tile, p.b_kind, one_layer(a, br, a.m, a.n), items, n_items, p.even, s);
  case GL_BF16_LW_QUADS: return launch_bf16_lw_quads(p.b_kind, one_layer(a, br, 128, 128), items, n_items, s);
  case GL_GENERIC:
    switch (p.generic) {
    case GG_F32: return launch_grouped_t<float, false, false>(a, wi, n_items, s);
    case GG_F32_VEC: return launch_grouped_t<float, false, true>(a, wi, n_items, s);
    case GG_BF16_VNNI2: return launch_grouped_t<unsigned short, true, false>(a, wi, n_items, s);
    case GG_BF16_VNNI2_VEC: return launch_grouped_t<unsigned short, true, true>(a, wi, n_items, s);
    case GG_BF16_VNNI4_VEC: return launch_grouped_t<unsigned short, true, true, 4>(a, wi, n_items, s);
    case GG_BF16_FLAT: return launch_grouped_t<unsigned short, false, false>(a, wi, n_items, s);
    case GG_F32_BT_VEC: return launch_grouped_t<float, false, true, 2, FORM_BT>(a, wi, n_items, s);
    case GG_F32_AT_VEC: return launch_grouped_t<float, false, true, 2, FORM_AT>(a, wi, n_items, s);
    case GG_F32_AT: return launch_grouped_t<float, false, false, 2, FORM_AT>(a, wi, n_items, s);
    }
  }
  return hipErrorInvalidValue;
}

hipError_t launch_gemm(const GemmDesc &d, const void *A, const void *B, void *C, const void *D, int64_t br,
                       hipStream_t stream) {
  const uintptr_t ab = (uintptr_t)A | (uintptr_t)B, c = (uintptr_t)C, dp = (uintptr_t)D;
  const GemmAlign al{!(ab & 15), !(c & 15), !(c & 7), !(dp & 7), !(dp & 15)};
  GemmPlanEnv env = gemm_plan_env();
  GemmLaunch p = plan_gemm_call(d, br, al, env);
  if (p.launcher == GL_NONE) return hipSuccess;
  const GemmArgs a = gemm_args(d, A, B, C, D, (int)(br < 0 ? 0 : br));
  if (p.launcher == GL_BF16_SKINNY) { // a skinny-batch bf16 layer (mode_switches.h MS_SKINNY_BF16; brgemm_bf16_skinny.h)
    hipError_t e = run_gemm_launch(p, a, a.br, nullptr, 1, false, stream);
    if (e == hipErrorInvalidValue && p.split > 1) { // the split refused by its launcher (mode_switches.h MS_SKINNY_SPLIT): the unsplit skinny launch of the same BN
      (void)hipGetLastError();
      env.skinny_split = 0;
      p = plan_gemm_call(d, br, al, env);
      e = run_gemm_launch(p, a, a.br, nullptr, 1, false, stream);
    }
    if (e != hipErrorInvalidValue) {
      if (e == hipSuccess) {
        const long long s_all = (long long)a.br * skn_steps(a.k);
        if (p.split > 1) count_mode_launch(MS_SKINNY_SPLIT, {p.split, sks_grid(skn_blocks(a.n, p.tile), p.split)});
        count_mode_launch(MS_SKINNY_BF16, {sks_grid(skn_blocks(a.n, p.tile), p.split), p.split > 1 ? sks_block_waves(p.split, (int)s_all) : skn_waves(s_all), p.tile, p.b_kind});
      }
      return g_last_refined.store(p.text, std::memory_order_relaxed), e;
    }
    (void)hipGetLastError(); // refused by the launcher: the launch the call has with the mode off
    env.skinny_bf16 = 0;
    p = plan_gemm_call(d, br, al, env);
  }
  if (p.launcher == GL_BF16_FAST && p.edge) { // edge tiles on the 256x256 tile (mode_switches.h MS_DMA256_EDGE; brgemm_bf16_dma256_edge.h)
    const hipError_t e = run_gemm_launch(p, a, a.br, nullptr, 1, false, stream);
    if (e != hipErrorInvalidValue) {
      if (e == hipSuccess) count_mode_launch(MS_DMA256_EDGE, {d256e_tiles((int)d.m), d256e_tiles((int)d.n), p.b_kind});
      return g_last_refined.store(p.text, std::memory_order_relaxed), e;
    }
    (void)hipGetLastError(); // refused by the launcher: the launch the call has with the mode off
    env.dma256_edge = 0;
    p = plan_gemm_call(d, br, al, env);
  }
  if (p.launcher == GL_BF16_FAST && p.b_kind != 0) { // a flat or VNNI-4 B on the 256x256 tile (mode_switches.h MS_DMA256_IMAGES; brgemm_bf16_dma256_images.h)
    const hipError_t e = run_gemm_launch(p, a, a.br, nullptr, 1, false, stream);
    if (e != hipErrorInvalidValue) {
      if (e == hipSuccess) count_mode_launch(MS_DMA256_IMAGES, {d.m / 256, d.n / 256, p.b_kind});
      return g_last_refined.store(p.text, std::memory_order_relaxed), e;
    }
    (void)hipGetLastError(); // refused by the launcher: the launch the call has with the mode off
    env.dma256_images = 0;
    p = plan_gemm_call(d, br, al, env);
  }
  if (p.edge_k8 && p.launcher == GL_BF16_LW) { // a bf16 half-step ragged-k launch (mode_switches.h MS_EDGE_K8_BF16; brgemm_bf16_lw_kedge.h bkedge8_*)
    const hipError_t e = run_gemm_launch(p, a, a.br, nullptr, 1, false, stream);
    if (e != hipErrorInvalidValue) {
      if (e == hipSuccess) // the tile with its B image: 20 + t VNNI-2, 24 + t flat, 28 + t VNNI-4
        count_mode_launch(MS_EDGE_K8_BF16, {bkedge_chunks(a.k), bkedge_overlap(a.k), blw_variant(p.tile, p.b_kind)});
      return g_last_refined.store(p.text, std::memory_order_relaxed), e;
    }
    (void)hipGetLastError(); // refused by the launcher: the launch the call has with the mode off
    env.edge_k8_bf16 = 0;
    p = plan_gemm_call(d, br, al, env);
  }
  if (p.edge_k && p.launcher == GL_BF16_LW) { // a bf16 ragged-k launch (mode_switches.h MS_EDGE_K_BF16; brgemm_bf16_lw_kedge.h)
    const hipError_t e = run_gemm_launch(p, a, a.br, nullptr, 1, false, stream);
    if (e != hipErrorInvalidValue) {
      if (e == hipSuccess) // the tile with its B image: 20 + t VNNI-2, 24 + t flat, 28 + t VNNI-4
        count_mode_launch(MS_EDGE_K_BF16, {bkedge_chunks(a.k), bkedge_overlap(a.k), blw_variant(p.tile, p.b_kind)});
      return g_last_refined.store(p.text, std::memory_order_relaxed), e;
    }
    (void)hipGetLastError(); // refused by the launcher: the launch the call has with the mode off
    env.edge_k_bf16 = 0;
    p = plan_gemm_call(d, br, al, env);
  }
  if (p.edge_k) { // a ragged-k launch (mode_switches.h MS_EDGE_K; brgemm_f32_lw_kedge.h)
    const hipError_t e = run_gemm_launch(p, a, a.br, nullptr, 1, false, stream);
    if (e != hipErrorInvalidValue) {
      if (e == hipSuccess) {
        static const int variant[5] = {0, V_F32_LW_64x64K2, V_F32_LW_64x32K2, V_F32_LW_32x32K4, V_F32_LW_128x64};
        count_mode_launch(MS_EDGE_K, {kedge_chunks(a.k), kedge_overlap(a.k), variant[p.tile >= 0 && p.tile < 5 ? p.tile : 0]});
      }
      return g_last_refined.store(p.text, std::memory_order_relaxed), e;
    }
    (void)hipGetLastError(); // refused by the launcher: the launch the call has with the mode off
    env.edge_k = 0;
    p = plan_gemm_call(d, br, al, env);
  }
  if (p.edge) { // a launch on edge tiles (mode_switches.h MS_EDGE_TILES)
    const hipError_t e = run_gemm_launch(p, a, a.br, nullptr, 1, false, stream);
    if (e != hipErrorInvalidValue) {
      if (e == hipSuccess) {
        static const int bm[5] = {0, 64, 64, 32, 128}, bn[5] = {0, 64, 32, 32, 64}, variant[5] = {0, V_F32_LW_64x64K2, V_F32_LW_64x32K2, V_F32_LW_32x32K4, V_F32_LW_128x64};
        const int ft = p.launcher == GL_F32_LW && p.tile >= 0 && p.tile < 5 ? p.tile : 0;
        int tbm = bm[ft], tbn = bn[ft], tv = variant[ft];
        if (p.launcher == GL_BF16_LW) // the tile with its B image: 20 + t VNNI-2, 24 + t flat, 28 + t VNNI-4
          blw_tile_dims(p.tile, &tbm, &tbn), tv = blw_variant(p.tile, p.b_kind);
        count_mode_launch(MS_EDGE_TILES, {(d.m + tbm - 1) / tbm, (d.n + tbn - 1) / tbn, tv});
      }
      return g_last_refined.store(p.text, std::memory_order_relaxed), e;
    }
    (void)hipGetLastError(); // refused by the launcher: the launch the call has with the mode off
    env.edge_tiles = 0;
    p = plan_gemm_call(d, br, al, env);
  }
  const char *text = p.text;
  if (p.split > 1 && (p.launcher == GL_F32_LW || p.launcher == GL_F32_LW16)) { // a SPLIT launch (its scratch block may be missing)
    const hipError_t e = launch_f32_lw_split(p.launcher == GL_F32_LW ? p.tile : 3, a, p.split, stream);
    if (e != hipErrorOutOfMemory && e != hipErrorInvalidValue) return g_last_refined.store(text, std::memory_order_relaxed), e;
    (void)hipGetLastError(); // no scratch block: the unsplit launch
    text = "";
  }
  if (p.tail_tiles > 0 && p.launcher == GL_F32_LW) { // a launch with a split tail (mode_switches.h MS_TAIL_SPLIT; its scratch block may be missing)
    const hipError_t e = launch_f32_lw_tail(p.tile, a, p.tail_tiles, p.tail_split, stream);
    if (e != hipErrorOutOfMemory && e != hipErrorInvalidValue) {
      if (e == hipSuccess) {
        const int64_t tiles = (d.m / (p.tile == 3 ? 32 : 64)) * (d.n / (p.tile == 1 ? 64 : 32));
        count_mode_launch(MS_TAIL_SPLIT, {p.tail_tiles, p.tail_split, tiles - p.tail_tiles});
      }
      return g_last_refined.store(text, std::memory_order_relaxed), e;
    }
    (void)hipGetLastError(); // no scratch block: the plain launch
    text = "";
  }
  g_last_refined.store(text, std::memory_order_relaxed);
  if (p.halves && p.launcher == GL_F32_LW && p.tile == 1) { // the tiles as two halves each (mode_switches.h MS_F32_HALVES): the same kernel name and text
    const hipError_t e = launch_f32_lw_halves(a, stream);
    if (e != hipErrorInvalidValue) {
      if (e == hipSuccess) count_mode_launch(MS_F32_HALVES, {d.m / 64, d.n / 64}); // (word 3 stays 0)
      return e;
    }
    (void)hipGetLastError(); // refused by the launcher: the launch the call has with the mode off
  }
  return run_gemm_launch(p, a, a.br, nullptr, 1, false, stream);
}

hipError_t launch_gemm_grouped(const GemmDesc &d, const WorkItem *items, int n_items, bool vec_ok, bool out_ok, bool pair_ok,
                               int64_t br_hint, hipStream_t stream) {
  const GemmLaunch p = plan_gemm_group(d, n_items, vec_ok, out_ok, pair_ok, br_hint, gemm_plan_env());
  if (p.launcher == GL_NONE || p.launcher == GL_INVALID) return p.launcher == GL_NONE ? hipSuccess : hipErrorInvalidValue;
  bool split_ran = false;
  const hipError_t e = run_gemm_launch(p, gemm_args(d, nullptr, nullptr, nullptr, nullptr, 0), (int)br_hint, items, n_items, true, stream, &split_ran);
  // (a group planned on the split of brgemm_bf16_small.hip whose stream has no scratch block ran unsplit: the report says what ran)
  g_last_grouped.store(p.launcher == GL_BF16_SMALL32 && p.split > 1 && !split_ran ? p.text_unsplit : p.text, std::memory_order_relaxed);
  return e;
}

// QUADS (round 6; xsmm_desc.h QuadItem, brgemm_bf16_lw.hip GRP = 2): a group of 64x64 bf16 tile invokes that forms a grid of item rows and
// item columns runs as 2 x 2 blocks on the 128x128 loader-wave tile when the tile model says so (gemm_quads_pay) - the kernel the same
// layer gets as ONE whole-layer call once it is large enough. 1024 x 2560 x 1024 as 640 invokes: 3 rounds of 64x64 tiles (15.3 us)
// against 160 workgroups of 128x128 (whole-layer call 10.2 us).
hipError_t launch_gemm_quads(const GemmDesc &d, const QuadItem *quads, int n_quads, int64_t br, hipStream_t stream) {
  const GemmLaunch p = plan_gemm_quads(d, n_quads, br);
  if (p.launcher == GL_INVALID) return hipErrorInvalidValue;
  g_last_grouped.store(p.text, std::memory_order_relaxed);
  return run_gemm_launch(p, gemm_args(d, nullptr, nullptr, nullptr, nullptr, 0), (int)br, quads, n_quads, true, stream);
}

} // namespace tpp
