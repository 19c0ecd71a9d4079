// xsmm_desc.h - immutable kernel descriptors behind the i64 handles of the C-ABI,
// and the launch interface between the ABI layer (runtime.cpp) and the gfx950
// kernels (*.hip). Not part of the public ABI (that is include/tpp_xsmm_abi.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <atomic>

namespace tpp {

enum : int { KIND_GEMM = 0x47454d4d /*'GEMM'*/, KIND_UNARY = 0x554e4152, KIND_BINARY = 0x42494e41,
             KIND_AMX = 0x414d5843 };
enum : int64_t { DT_F32 = 1, DT_BF16 = 2 };
enum : int { EP_BETA0 = 1, EP_BIAS = 2, EP_RELU = 4, EP_VNNI_C = 8 }; // epilogue bits of the kernel argument blocks

// One descriptor type for gemm / brgemm / fused_brgemm (a gemm is a brgemm with
// one batch and no strides; a brgemm is a fused_brgemm with no epilogue).
struct GemmDesc {
  int kind;             // KIND_GEMM
  int has_batch;        // 0: dispatched through xsmm_gemm_dispatch
  int fused;            // dispatched through xsmm_fused_brgemm_dispatch (invoke takes D)
  int64_t dtype, m, n, k, lda, ldb, ldc, stride_a, stride_b;
  int64_t wire_flags;   // as received (BETA_0 = 4, VNNI_B wire = 2048, ...)
  int beta0, vnni_b, bias, relu;
  int vnni_c;           // C stored / read as VNNI-2 [m/2][n][2] (wire flag 8192): generic kernel only
  int vnni_factor;      // blocking factor v of a VNNI B operand [k/v][n][v]: 2, or 4 (xsmm_hip_set_vnni_factor at dispatch time; the
                        // factor is not on the wire - the reference asks libxsmm_cpuid_dot_pack_factor, VNNIUtils.cpp:25-45)
  int f32_prec;         // f32 arithmetic: 0 = exact f32 MFMA, 6 = bf16x6 split (xsmm_hip_set_f32_precision at dispatch time; part of the
                        // descriptor key; 0 for bf16 descriptors). plan_gemm runs brgemm_f32_x6.hip where a split tile is forced and fits, else the exact kernel
  int variant;          // kernel variant chosen at dispatch (gemm_plan.h GemmVariant), -1 = by invoke
  int generic_forced;   // variant = generic because it was asked for (xsmm_hip_force_variant / a VNNI C store), not because no fast tile fits
  int variant_forced;   // variant is the one xsmm_hip_force_variant asked for: invoke-time refinements (batch-count dependent) leave it alone
  int b_trans;          // runtime-made sibling of a dispatched descriptor (never on the wire): B is read TRANSPOSED, B[k][j] = ptr[j * ldb + k] -
                        // the source of an xsmm.unary transpose that fed this gemm's B operand (rt_rewrites.h, deferred transposes); generic kernel only
  int a_trans;          // the same for the A operand (mode 2 of xsmm_hip_set_fold_transpose only): A[i][k] = ptr[k * lda + i]; never together with b_trans
  int trans_mode;       // the mode of xsmm_hip_set_fold_transpose a sibling was made under (1 or 2; 0: no sibling): a mode-2 sibling may run on
                        // the 16-byte instances of the generic kernel (gemm_plan.cpp trans_launch), a mode-1 sibling never leaves the element path
  char name[64];        // kernel name for profiles
  char trace[160];      // dispatch tuple + kernel name as text (trace ranges)
};

struct UnaryDesc {
  int kind;             // KIND_UNARY
  int64_t op, dtype, m, n, ldi, ldo, flags;
  char trace[96];       // dispatch tuple as text (trace ranges)
};

struct BinaryDesc {
  int kind;             // KIND_BINARY
  int64_t op, dtype, m, n, ldi_lhs, ldi_rhs, ldo, flags;
  char trace[96];
};

struct AmxDesc {
  int kind;             // KIND_AMX (no-op on this hardware)
};

// One queued invoke (tile queue, runtime.cpp): operands with element offsets applied. GEMM family:
// A, B, C, D + batch count; unary: A = in, C = out; binary: A = lhs, B = rhs, C = out. The array is
// host-pinned and read by the grouped kernels directly.
struct WorkItem {
  const void *A;
  const void *B;
  void *C;
  const void *D;
  int64_t br;
};

// A 2 x 2 block of queued 64x64 bf16 invokes (tile queue, rt_rewrites.h detect_quads): item rows r0 < r1 (A blocks), item columns
// c0 < c1 (B blocks). A / B: the (r0, c0) item's; da = (byte distance of r1's A block from r0's) - 64 rows of lda, db = byte distance
// of c1's B block from c0's; C[2 r + c], D[c]: the four outputs and the two bias pieces. brgemm_bf16_lw's 128x128 tile (GRP = 2).
struct QuadItem {
  const void *A;
  const void *B;
  void *C[4];
  const void *D[2];
  int64_t br;
  uint32_t da, db;
};

// One run of a RELAYOUT GRID (tile queue, rt_relayout.h): R x C blocks of one unary identity / VNNI-2 descriptor, block (r, c) reads
// in + r in_r + c in_c and writes out + r out_r + c out_c (strides in ELEMENTS). wg0: the first workgroup of the run (runs in
// ascending order); vec: bases and strides allow 16-byte accesses (else the kernel's element path).
struct RelayoutRun {
  const void *in;
  void *out;
  int64_t in_r, in_c, out_r, out_c;
  int32_t R, C;
  int32_t wg0, vec;
};

// EPILOGUE PROGRAMS (tile queue, rt_tile_queue.h "epilogue fold"): the element-wise invokes the compiler leaves behind a GEMM tile
// (binary add / mul / sub / div with any broadcast of the other operand, unary identity / relu / zero) folded into the GEMM group they
// follow. One program per launch - at most two post-ops, the same handles in the same order for every item; stage s continues the
// value of stage s - 1 (stage 0 = the GEMM's stored output C) and rounds at its own store, as the invoke it replaces does.
enum : int { PO_ADD = 1, PO_MUL = 2, PO_SUB = 3, PO_DIV = 4, PO_IDENTITY = 5, PO_RELU = 6, PO_ZERO = 7 };
struct PostOp {
  int op;     // PO_*
  int pos;    // binary: operand position of the continued value (0 = lhs, 1 = rhs)
  int bc;     // broadcast of the OTHER operand: 0 none, 1 row, 2 col, 3 scalar (eltwise.hip BC_*)
  int pad;
  int64_t ld;  // leading dimension of the other operand (elements)
  int64_t ldo; // ... of the stage's output
};
struct PostProgram {
  int n;          // post-ops (1 or 2)
  int m, cols;    // tile shape = the GEMM's m x n
  int pad;
  int64_t dtype;  // DT_F32 / DT_BF16
  int64_t ldc;    // leading dimension of the GEMM's output C
  PostOp op[2];
};
// one GEMM item's chain: its output tile, the other operand and the output of each stage (a side array next to the work list -
// WorkItem is not widened). out[s] == out[s + 1]: the stage is in place and only the later value is stored.
struct PostItem {
  const void *C;
  const void *other[2];
  void *out[2];
};

// ---- kernel launchers (all enqueue on `stream`, never synchronise) --------------
// pointers are device pointers with element offsets already applied.
hipError_t launch_gemm(const GemmDesc &d, const void *A, const void *B, void *C, const void *D,
                       int64_t br, hipStream_t stream);
// n_items invokes of ONE descriptor in one launch (items: device array of WorkItem)
// vec_ok: every item's A and B are 16-byte aligned; out_ok: every item's C is 16-byte and D 8-byte aligned;
// pair_ok: every item's batch count is even (32-k tiles on the loader-wave kernels)
// br_hint: the batch count of the first item - only a hint for how many workgroups share a tile's batch-reduce range (split
// launches of skinny groups); the kernels take every item's own count from the list
hipError_t launch_gemm_grouped(const GemmDesc &d, const WorkItem *items, int n_items, bool vec_ok, bool out_ok, bool pair_ok,
                               int64_t br_hint, hipStream_t stream);
int force_gemm_split(int workgroups_per_tile); // xsmm_hip_force_split (brgemm_f32.hip); returns the previous setting
// STRICT mode (round 6; xsmm_hip_set_strict / TPP_HIP_STRICT=1): the kernel an invoke runs on - and with it the order of its additions -
// is a function of its descriptor, its batch count and its own pointers' alignment only, never of the group it is queued with.
// launch_gemm_grouped then takes every decision that depends on the size of the work list as if the list held ONE item.
// QUADS: would a group of n_items invokes of `d` (batch count br each, all operands 16-byte aligned) run faster as n_items / 4
// 2 x 2 blocks on the 128x128 loader-wave tile than as items on the grouped 64x64 / 32x64 tiles? (the tile model of pick_bf16_lw_tile;
// bf16 VNNI-2 / VNNI-4, m = n = 64, k a multiple of 64; never in strict mode; gemm_plan.h)
bool gemm_quads_pay(const GemmDesc &d, int n_items, int64_t br);
hipError_t launch_gemm_quads(const GemmDesc &d, const QuadItem *quads, int n_quads, int64_t br, hipStream_t stream);
int set_strict_kernels(int on); // returns the previous setting
bool strict_kernels();
const char *last_grouped_kernel(); // kernel family of the most recent launch_gemm_grouped ("" before the first)
const char *last_refined_kernel(); // most recent launch_gemm: the kernel an invoke-time refinement chose, "" = the descriptor's own
// fills d.variant / d.name for this device (gemm_plan.h plan_gemm); returns false if no kernel can run the descriptor
bool plan_gemm(GemmDesc &d, int forced_variant);
hipError_t launch_unary(const UnaryDesc &d, const void *in, float scalar, bool use_scalar, void *out,
                        hipStream_t stream);
hipError_t launch_binary(const BinaryDesc &d, const void *lhs, const void *rhs, void *out,
                         hipStream_t stream);
// most recent launch_unary / launch_binary: the kernel instance it ran (a static string such as "unary_kernel<f32,v4>, flat",
// "transpose_vec<bf16,128x128>", "vnni2_rows4<wt>"; "" before the first) and the launch's total block count
// (xsmm_hip_last_eltwise_kernel / _grid: tests assert which path a shape reached and derive every block's span from the grid; the
// grouped kernels of the tile queue do not report). Inline variables like the mode switches' (mode_switches.h): eltwise.hip stores, runtime.cpp reads,
// and the host-only builds of runtime.cpp (tests/tsan) link without any kernel file. Relaxed accesses, as last_refined_kernel.
inline std::atomic<const char *> g_last_eltwise{""};
inline std::atomic<int64_t> g_last_eltwise_grid{0};
// n_items invokes of ONE unary / binary descriptor with m, n <= 64 in one launch
hipError_t launch_unary_grouped(const UnaryDesc &d, const WorkItem *items, int n_items, hipStream_t stream);
hipError_t launch_binary_grouped(const BinaryDesc &d, const WorkItem *items, int n_items, hipStream_t stream);
// n_items epilogue programs (items: device-readable array of PostItem) in ONE launch, one workgroup per item (eltwise.hip). Runs
// behind the GEMM group whose outputs it reads, on the same stream. Weak like launch_relayout_grid: the host-only sanitizer builds
// (tests/tsan) link runtime.cpp without the gfx950 kernels.
__attribute__((weak)) hipError_t launch_postop_grouped(const PostProgram &p, const PostItem *items, int n_items, hipStream_t stream);
// RELAYOUT GRIDS (relayout.hip): the blocks of n_runs runs (device array) of an identity (f32, bf16) or VNNI-2 (bf16) descriptor
// in ONE launch of n_wg workgroups, one block each. Bit-exact word moves. Weak: the host-only sanitizer builds of runtime.cpp
// (tests/tsan) link it without the gfx950 kernels - there it is null and the tile queue never chooses a relayout grid; the product
// library always defines it (relayout.hip).
__attribute__((weak)) hipError_t launch_relayout_grid(const UnaryDesc &d, const RelayoutRun *runs, int n_runs, int n_wg, hipStream_t stream);

} // namespace tpp
