// x6_probe.hip - go / no-go probe of the bf16x6 split f32 GEMM: does v_mfma_f32_32x32x16_bf16 accumulate its 16
// products with f32 care? One wave computes C = A B for ONE 32 x 32 x 1024 problem three ways:
//   x6:    every f32 operand split into hi + mid + lo bf16 parts (RNE one after another), six 32x32x16_bf16 MFMAs per k-step of 16
//          (small terms first: hi.lo, lo.hi, mid.mid, hi.mid, mid.hi, hi.hi) into one f32 accumulator;
//   exact: 512 v_mfma_f32_32x32x2_f32 (the project's exact f32 path);
//   and the host's fp64 product as the truth.
// Two data sets: uniform [-1, 1) and a sign-cancelling one (k pairs whose products nearly cancel: |C| ~ 1e-3 of sum |a||b|).
// Printed per data set and path: the worst |err| / sum_k |a||b| over the elements (the scale the element-wise bar uses), the
// normwise max |err| / max |truth| and the worst relative error over the non-cancelled elements (|truth| >= 1 % of its maximum).
// Verdict: GO if the x6 path's figures are within 2x the exact path's. Build: hipcc --offload-arch=gfx950 -O2 x6_probe.hip -o x6_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
constexpr int K = 1024;

__device__ inline unsigned short rne_bf16(float f) {
  unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40u);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
}
__device__ inline void split3(float a, short &h, short &m, short &l) {
  const unsigned short hb = rne_bf16(a);
  const float r = a - __uint_as_float((unsigned)hb << 16);
  const unsigned short mb = rne_bf16(r);
  const float r2 = r - __uint_as_float((unsigned)mb << 16);
  h = (short)hb, m = (short)mb, l = (short)rne_bf16(r2);
}

// A [32][K] row-major, B [K][32] row-major, C [32][32] row-major
__global__ void probe(const float *A, const float *B, float *Cx6, float *Cex) {
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  f32x16 acc = {};
  for (int s = 0; s < K / 16; ++s) {
    bf16x8 ah, am, al, bh, bm, bl;
    for (int j = 0; j < 8; ++j) {
      const int k = 16 * s + 8 * h + j;
      short x, y, z;
      split3(A[r * K + k], x, y, z);
      ah[j] = x, am[j] = y, al[j] = z;
      split3(B[k * 32 + r], x, y, z);
      bh[j] = x, bm[j] = y, bl[j] = z;
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bm, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bm, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
  }
  f32x16 ex = {};
  for (int s = 0; s < K / 2; ++s) ex = __builtin_amdgcn_mfma_f32_32x32x2f32(A[r * K + 2 * s + h], B[(2 * s + h) * 32 + r], ex, 0, 0, 0);
  for (int q = 0; q < 16; ++q) { // C/D layout: col = lane & 31, row = (q & 3) + 8 (q >> 2) + 4 (lane >> 5)
    const int row = (q & 3) + 8 * (q >> 2) + 4 * h;
    Cx6[row * 32 + r] = acc[q];
    Cex[row * 32 + r] = ex[q];
  }
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

struct Err { double mag, norm, rel; };
static Err errors(const std::vector<float> &C, const std::vector<double> &T, const std::vector<double> &M) {
  double tmax = 0, emax = 0, mag = 0, rel = 0;
  for (int i = 0; i < 1024; ++i) tmax = std::fmax(tmax, std::fabs(T[i]));
  for (int i = 0; i < 1024; ++i) {
    const double e = std::fabs(C[i] - T[i]);
    emax = std::fmax(emax, e);
    mag = std::fmax(mag, e / M[i]);
    if (std::fabs(T[i]) >= 1e-2 * tmax) rel = std::fmax(rel, e / std::fabs(T[i]));
  }
  return {mag, emax / tmax, rel};
}

int main() {
  float *dA, *dB, *dX, *dE;
  CK(hipMalloc(&dA, 32 * K * 4)); CK(hipMalloc(&dB, K * 32 * 4)); CK(hipMalloc(&dX, 4096)); CK(hipMalloc(&dE, 4096));
  bool go = true;
  for (int set = 0; set < 2; ++set) {
    std::vector<float> A(32 * K), B(K * 32);
    srand(7 + set);
    auto u = [] { return 2.0f * (float)rand() / (float)RAND_MAX - 1.0f; };
    for (auto &x : A) x = u();
    for (auto &x : B) x = u();
    if (set == 1) // sign-cancelling: a[2t+1] = a[2t], b[2t+1] = -b[2t] (1 + 1e-3 u): pairs cancel to ~1e-3 of their magnitude
      for (int k = 0; k < K; k += 2) {
        for (int i = 0; i < 32; ++i) A[i * K + k + 1] = A[i * K + k];
        for (int j = 0; j < 32; ++j) B[(k + 1) * 32 + j] = -B[k * 32 + j] * (1.0f + 1e-3f * u());
      }
    std::vector<double> T(1024, 0.0), M(1024, 0.0);
    for (int i = 0; i < 32; ++i)
      for (int j = 0; j < 32; ++j)
        for (int k = 0; k < K; ++k) {
          T[i * 32 + j] += (double)A[i * K + k] * B[k * 32 + j];
          M[i * 32 + j] += std::fabs((double)A[i * K + k] * B[k * 32 + j]);
        }
    CK(hipMemcpy(dA, A.data(), A.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dB, B.data(), B.size() * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, dA, dB, dX, dE);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    std::vector<float> X(1024), E(1024);
    CK(hipMemcpy(X.data(), dX, 4096, hipMemcpyDeviceToHost));
    CK(hipMemcpy(E.data(), dE, 4096, hipMemcpyDeviceToHost));
    const Err ex = errors(E, T, M), x6 = errors(X, T, M);
    const char *name = set ? "sign-cancelling" : "uniform [-1,1)";
    printf("%-16s exact f32 MFMA: max|err|/mag %.3g  normwise %.3g  rel(non-cancelled) %.3g\n", name, ex.mag, ex.norm, ex.rel);
    printf("%-16s bf16x6        : max|err|/mag %.3g  normwise %.3g  rel(non-cancelled) %.3g\n", name, x6.mag, x6.norm, x6.rel);
    if (x6.norm > 2 * ex.norm + 1e-9 || x6.rel > 2 * ex.rel + 1e-9) go = false;
  }
  printf("verdict: %s\n", go ? "GO (bf16x6 within 2x of the exact f32 MFMA)" : "NO-GO (bf16x6 error above 2x the exact path's)");
  return go ? 0 : 1;
}
