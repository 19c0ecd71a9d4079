// brgemm_bf16_dma256.hip - the large-shape member of the bf16 BRGEMM family for gfx950: 256 x 256 workgroup tiles for outputs both of whose
// dimensions the tile divides. The kernel's text: brgemm_bf16_dma256_tile.h (its edge-tile instances: brgemm_bf16_dma256_edge.hip).
#include "brgemm_bf16_dma256_tile.h"

namespace tpp {

__global__ __launch_bounds__(256) void brgemm_bf16_dma256(GemmArgs p) { brgemm_bf16_dma256_body<0, false>(p); }
__global__ __launch_bounds__(256) void brgemm_bf16_dma256_flatb(GemmArgs p) { brgemm_bf16_dma256_body<2, false>(p); }
__global__ __launch_bounds__(256) void brgemm_bf16_dma256_vnni4(GemmArgs p) { brgemm_bf16_dma256_body<4, false>(p); }

template <int IMG> static hipError_t launch_bf16_dma256_t(const GemmArgs &a, hipStream_t s) {
  constexpr size_t lds = 4 * 32768;
  static std::atomic<unsigned long long> lds_set{0};
  void (*const kern)(GemmArgs) = IMG == 0 ? brgemm_bf16_dma256 : IMG == 2 ? brgemm_bf16_dma256_flatb : brgemm_bf16_dma256_vnni4;
  if (hipError_t e = ensure_dynamic_lds((const void *)kern, (int)lds, lds_set); e != hipSuccess) return e;
  GemmArgs args = a;
  const int tiles_m = a.m / 256, tiles_n = a.n / 256;
  dim3 grid;
  if ((tiles_m & 3) == 0 && (tiles_n & 1) == 0 && tiles_m / 4 <= 65535 && tiles_n / 2 <= 65535) {
    args.tiles_m = tiles_m / 4; // XCD-blocked, as the other fast kernels
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

hipError_t launch_bf16_dma256(const GemmArgs &a, hipStream_t s) { return launch_bf16_dma256_t<0>(a, s); }

// The same tile with B image b_kind (0 VNNI-2, 2 flat, 4 VNNI-4; xsmm_hip_set_dma256_images, gemm_plan.cpp plan_gemm_call). Unlike the plain
// launcher it checks what the kernel assumes and refuses everything else with hipErrorInvalidValue - the caller then runs the launch the
// call has with the mode off: whole tiles, whole 32-k chunks, a batch element, 16-byte pieces at every DMA lane's source and at every row
// of C, the 8-byte bias reads, the lane offsets in 31 bits.
hipError_t launch_bf16_dma256_image(int b_kind, const GemmArgs &a, hipStream_t s) {
  if (!d256_image_ok(b_kind) || a.m <= 0 || a.n <= 0 || a.m % D256_BM || a.n % D256_BN || a.k <= 0 || a.k % D256_BK || a.br < 1) return hipErrorInvalidValue;
  if (!d256_b_ldb_ok(b_kind, a.ldb) || a.lda < a.k || a.ldc < a.n || ((a.lda | a.ldc | a.stride_a | a.stride_b) & 7) || a.lda >= (1 << 22) || a.ldc >= (1 << 22))
    return hipErrorInvalidValue;
  if ((((uintptr_t)a.A | (uintptr_t)a.B | (uintptr_t)a.C) & 15) || ((a.ep & EP_BIAS) && (!a.D || ((uintptr_t)a.D & 7))) || (a.ep & EP_VNNI_C)) return hipErrorInvalidValue;
  return b_kind == 0 ? launch_bf16_dma256_t<0>(a, s) : b_kind == 2 ? launch_bf16_dma256_t<2>(a, s) : launch_bf16_dma256_t<4>(a, s);
}

} // namespace tpp
