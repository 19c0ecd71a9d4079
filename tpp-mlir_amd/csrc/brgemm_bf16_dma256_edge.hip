// brgemm_bf16_dma256_edge.hip - edge tiles on the 256 x 256 bf16 tile (opt-in: xsmm_hip_set_dma256_edge): a large whole-layer call whose m
// or n is not a multiple of 256 on a ceil-divided grid of the tile of brgemm_bf16_dma256_tile.h. The last tile row starts at m - 256, the
// last tile column at n - 256; a shifted tile computes all its 256 x 256 elements - the same k values in the same order on the same MFMA
// as the tile in front of it does for the elements they share - and stores only what no other tile owns (brgemm_bf16_dma256_edge.h).
// beta = 1 reads C before any store of the same workgroup, and the overlap elements it reads are never stored by it.
#include "brgemm_bf16_dma256_tile.h"

namespace tpp {

__global__ __launch_bounds__(256) void brgemm_bf16_dma256_edge(GemmArgs p) { brgemm_bf16_dma256_body<0, true>(p); }
__global__ __launch_bounds__(256) void brgemm_bf16_dma256_edge_flatb(GemmArgs p) { brgemm_bf16_dma256_body<2, true>(p); }
__global__ __launch_bounds__(256) void brgemm_bf16_dma256_edge_vnni4(GemmArgs p) { brgemm_bf16_dma256_body<4, true>(p); }

template <int IMG> static hipError_t launch_bf16_dma256_edge_t(const GemmArgs &a, hipStream_t s) {
  constexpr size_t lds = 4 * 32768;
  static std::atomic<unsigned long long> lds_set{0};
  void (*const kern)(GemmArgs) = IMG == 0 ? brgemm_bf16_dma256_edge : IMG == 2 ? brgemm_bf16_dma256_edge_flatb : brgemm_bf16_dma256_edge_vnni4;
  if (hipError_t e = ensure_dynamic_lds((const void *)kern, (int)lds, lds_set); e != hipSuccess) return e;
  GemmArgs args = a;
  const int tiles_m = d256e_tiles(a.m), tiles_n = d256e_tiles(a.n);
  dim3 grid;
  if ((tiles_m & 3) == 0 && (tiles_n & 1) == 0 && tiles_m / 4 <= 65535 && tiles_n / 2 <= 65535) {
    args.tiles_m = tiles_m / 4; // XCD-blocked, as launch_bf16_dma256_t
    args.tiles_n = tiles_n / 2;
    grid = dim3(8, args.tiles_n, args.tiles_m);
  } else {
    args.tiles_m = args.tiles_n = 0;
    if (tiles_m > 65535 || tiles_n > 65535) return hipErrorInvalidValue;
    grid = dim3(1, tiles_n, tiles_m);
  }
  hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, args);
  return hipGetLastError();
}

// B image b_kind (0 VNNI-2, 2 flat, 4 VNNI-4; gemm_plan.cpp plan_gemm_call). Refuses with hipErrorInvalidValue everything the kernel does
// not assume - the caller then runs the launch the call has with the mode off: at least one whole tile in both dimensions, column shifts
// in whole 16-byte pieces (n % 8), whole 32-k chunks, a batch element, and what launch_bf16_dma256_image asks of leading dimensions,
// strides, alignment and VNNI C.
hipError_t launch_bf16_dma256_edge(int b_kind, const GemmArgs &a, hipStream_t s) {
  if (!d256_image_ok(b_kind) || !d256e_extent_ok(a.m) || !d256e_extent_ok(a.n) || a.n % 8 || a.k <= 0 || a.k % D256_BK || a.br < 1) return hipErrorInvalidValue;
  if (!d256_b_ldb_ok(b_kind, a.ldb) || a.ldb < a.n || a.lda < a.k || a.ldc < a.n || ((a.lda | a.ldc | a.stride_a | a.stride_b) & 7) || a.lda >= (1 << 22) ||
      a.ldc >= (1 << 22))
    return hipErrorInvalidValue;
  if ((((uintptr_t)a.A | (uintptr_t)a.B | (uintptr_t)a.C) & 15) || ((a.ep & EP_BIAS) && (!a.D || ((uintptr_t)a.D & 7))) || (a.ep & EP_VNNI_C)) return hipErrorInvalidValue;
  return b_kind == 0 ? launch_bf16_dma256_edge_t<0>(a, s) : b_kind == 2 ? launch_bf16_dma256_edge_t<2>(a, s) : launch_bf16_dma256_edge_t<4>(a, s);
}

} // namespace tpp
