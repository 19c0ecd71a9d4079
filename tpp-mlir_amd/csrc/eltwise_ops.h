// eltwise_ops.h - the element arithmetic of the xsmm binary / unary ops (gfx950), shared by eltwise.hip's kernels and the tile
// queue's epilogue programs (postop_grouped_kernel) so that a folded post-op is the very arithmetic of the invoke it replaces:
// f32 compute, one operation per value (no contraction into an FMA across ops), a correctly rounded divide (HIP's default for
// '/'), relu(NaN) = 0 (the comparison is false for NaN) and relu(-0) = +0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tpp {

enum : int64_t { B_ADD = 1, B_MUL = 2, B_SUB = 3, B_DIV = 4 };

__device__ __forceinline__ float ew_binary(int op, float a, float b) {
#pragma clang fp contract(off)
  switch (op) {
  case (int)B_ADD: return a + b;
  case (int)B_MUL: return a * b;
  case (int)B_SUB: return a - b;
  default: return a / b;
  }
}
__device__ __forceinline__ float ew_relu(float f) { return f > 0.0f ? f : 0.0f; }

} // namespace tpp
