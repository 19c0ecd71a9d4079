// relayout.hip - RELAYOUT GRIDS for gfx950: the per-block xsmm.unary identity / VNNI-2 invokes of a tensor.pack / unpack (the
// compiler lowers them to one 2-D copy per block: LowerPacksAndUnpacks.cpp:45-49,112-121) as ONE launch over a table of affine runs
// (rt_relayout.h finds them in a recorded tile-queue group).
//
// Semantics = unary_grouped_kernel's (eltwise.hip) for the same descriptor, per block:
//   identity  out[i ldo + j] = in[i ldi + j]                                  i < m, j < n      (f32, bf16)
//   VNNI-2    out[r (2 ldo) + 2 j + p] = in[(2 r + p) ldi + j]                 r < m / 2, p < 2  (bf16)
// Raw 32- / 16-bit words are moved, never values: NaN payloads, -0 and subnormals survive bit for bit.
//
// Work mapping: workgroup w owns ONE block of one run (runs[k].wg0 <= w < runs[k + 1].wg0); blocks are numbered r C + c, and the
// run's inner index c is the one with the smaller source stride (rt_relayout.h), so consecutive workgroups read neighbouring pieces
// of the same source rows. Each lane moves 16 bytes per access where the run allows it (RelayoutRun::vec: bases,
// block strides, ldi / ldo and n in whole 16-byte pieces): identity = one 16-byte load + one 16-byte store, VNNI-2 = two 8-byte loads
// of the row pair interleaved in registers + one 16-byte store. RL_U pieces per lane are loaded before any is stored. Runs that do
// not allow it take the element path of the same kernel.
#include "xsmm_desc.h"

namespace tpp {
namespace {

typedef unsigned int rl_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int rl_u32x2 __attribute__((ext_vector_type(2)));
constexpr int64_t RL_OP_IDENTITY = 1, RL_OP_VNNI2 = 28; // xsmm.unary kinds (XSMM_UNARY_IDENTITY / XSMM_UNARY_VNNI2)
constexpr int RL_U = 4;                                 // 16-byte pieces in flight per lane

// 16-byte accesses: plain loads, WRITE-THROUGH (sc1) stores - the lowest kernel time on every pack script of the sweep in
// profiles/r07_relayout_grid_ab.txt (plain and nontemporal stores, 1 / 2 / 4 blocks per workgroup were measured there)
__device__ __forceinline__ rl_u32x4 rl_ld16(const void *p) { return *(const rl_u32x4 *)p; }
__device__ __forceinline__ rl_u32x2 rl_ld8(const void *p) { return *(const rl_u32x2 *)p; }
__device__ __forceinline__ void rl_st16(void *p, rl_u32x4 v) { asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory"); }

template <typename T, bool VNNI>
__global__ __launch_bounds__(256) void relayout_grid_kernel(const RelayoutRun *__restrict__ runs, int n_runs, int m, int n, int64_t ldi,
                                                            int64_t ldo) {
  const int w = blockIdx.x;
  int k = 0;
  while (k + 1 < n_runs && runs[k + 1].wg0 <= w) ++k; // (<= 16 runs, uniform: scalar loads)
  const RelayoutRun ru = runs[k];
  const int C = ru.C, b = w - ru.wg0, r = b / C, c = b - r * C; // this workgroup's block
  const T *in = (const T *)ru.in;
  T *out = (T *)ru.out;
  const int t = threadIdx.x;
  if (ru.vec) {
    // a piece: identity = V consecutive elements of one block row; VNNI-2 = 4 columns of one row pair (8 output elements)
    constexpr int V = VNNI ? 4 : 16 / (int)sizeof(T);
    const int pr = n / V, total = (VNNI ? m / 2 : m) * pr;
    for (int base = 0; base < total; base += 256 * RL_U) {
      rl_u32x4 x[RL_U];
      int64_t o[RL_U];
#pragma unroll
      for (int u = 0; u < RL_U; ++u) {
        const int p = base + u * 256 + t;
        o[u] = -1;
        if (p >= total) continue;
        const int i = p / pr, j = (p - i * pr) * V;
        const T *src = in + r * ru.in_r + c * ru.in_c + j;
        if constexpr (VNNI) {
          const rl_u32x2 e = rl_ld8(src + (int64_t)(2 * i) * ldi), d = rl_ld8(src + (int64_t)(2 * i + 1) * ldi);
          x[u][0] = (e[0] & 0xffffu) | (d[0] << 16); // output dword = (even row element, odd row element)
          x[u][1] = (e[0] >> 16) | (d[0] & 0xffff0000u);
          x[u][2] = (e[1] & 0xffffu) | (d[1] << 16);
          x[u][3] = (e[1] >> 16) | (d[1] & 0xffff0000u);
          o[u] = r * ru.out_r + c * ru.out_c + (int64_t)i * (2 * ldo) + 2 * j;
        } else {
          x[u] = rl_ld16(src + (int64_t)i * ldi);
          o[u] = r * ru.out_r + c * ru.out_c + (int64_t)i * ldo + j;
        }
      }
#pragma unroll
      for (int u = 0; u < RL_U; ++u)
        if (o[u] >= 0) rl_st16(out + o[u], x[u]);
    }
    return;
  }
  // element path: one element per lane per step, consecutive lanes on consecutive output elements
  const int total = VNNI ? (m / 2) * 2 * n : m * n;
  const T *src = in + r * ru.in_r + c * ru.in_c;
  T *dst = out + r * ru.out_r + c * ru.out_c;
  for (int q = t; q < total; q += 256) {
    if constexpr (VNNI) {
      const int i = q / (2 * n), rem = q - i * 2 * n;
      dst[(int64_t)i * (2 * ldo) + rem] = src[(int64_t)(2 * i + (rem & 1)) * ldi + (rem >> 1)];
    } else {
      const int i = q / n, j = q - i * n;
      dst[(int64_t)i * ldo + j] = src[(int64_t)i * ldi + j];
    }
  }
}

template <typename T, bool VNNI> hipError_t launch_t(const UnaryDesc &d, const RelayoutRun *runs, int n_runs, int n_wg, hipStream_t s) {
  hipLaunchKernelGGL((relayout_grid_kernel<T, VNNI>), dim3((unsigned)n_wg), dim3(256), 0, s, runs, n_runs, (int)d.m, (int)d.n, d.ldi, d.ldo);
  return hipGetLastError();
}

} // namespace

hipError_t launch_relayout_grid(const UnaryDesc &d, const RelayoutRun *runs, int n_runs, int n_wg, hipStream_t s) {
  if (n_runs <= 0 || n_wg <= 0) return hipSuccess;
  if (d.m <= 0 || d.n <= 0 || d.m > 64 || d.n > 64 ) return hipErrorInvalidValue;
  if (d.op == RL_OP_VNNI2) {
    if (d.dtype != DT_BF16 || (d.m & 1)) return hipErrorInvalidValue;
    return launch_t<unsigned short, true>(d, runs, n_runs, n_wg, s);
  }
  if (d.op != RL_OP_IDENTITY) return hipErrorInvalidValue;
  if (d.dtype == DT_F32) return launch_t<unsigned int, false>(d, runs, n_runs, n_wg, s);
  return launch_t<unsigned short, false>(d, runs, n_runs, n_wg, s);
}

} // namespace tpp
