// fake_hip_host.h - TEST INFRASTRUCTURE, never part of the product library: the HIP host entry points runtime.cpp uses, over plain
// host memory. Shared by the two host-only stand-in builds: tests/tsan/fake_hip.cpp (sanitizer, host-cache and fold runs: scalar f32
// launch stand-ins) and tests/chain_dispatch/fake_chain.cpp (the layer-chain launch decision on a CPU: computing bf16 stand-ins).
// Include it into exactly ONE translation unit of a build, behind the HIP headers.
//   * "device" allocations are malloc'd blocks kept in a table so that hipPointerGetAttributes / hipMemGetAddressRange answer like
//     the driver; streams are in-order and every operation completes before its call returns;
//   * the device has FAKE_HIP_CUS compute units (default 256): hipDeviceGetAttribute answers it, and the CU mask of every stream
//     has that many bits. fake_hip_cu_mask_queries() counts the calls of hipExtStreamGetCUMask (how often a host path asked for a
//     stream's compute units);
//   * no stream is being captured unless fake_hip_set_capturing(1) says so: hipStreamIsCapturing then answers "active" for every
//     stream until fake_hip_set_capturing(0) (tests/split_scratch/driver.cpp).
#pragma once
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>

namespace {
std::mutex g_mu;
std::map<uintptr_t, size_t> g_dev; // base -> size of live "device" allocations
bool find_alloc(const void *p, uintptr_t *base, size_t *size) {
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_dev.upper_bound((uintptr_t)p);
  if (it == g_dev.begin()) return false;
  --it;
  if ((uintptr_t)p >= it->first + it->second) return false;
  *base = it->first;
  *size = it->second;
  return true;
}
int fake_hip_cus() { // compute units of the fake device
  static const int cus = [] {
    const char *e = getenv("FAKE_HIP_CUS");
    const int v = e ? atoi(e) : 0;
    return v > 0 && v <= 512 ? v : 256;
  }();
  return cus;
}
std::atomic<long> g_cu_mask_queries{0};
std::atomic<bool> g_capturing{false}; // what hipStreamIsCapturing answers for every stream (fake_hip_set_capturing): "none" unless a test says so
} // namespace

extern "C" {
hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
hipError_t hipGetDevice(int *d) { *d = 0; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "fake hip error"; }
hipError_t hipMalloc(void **p, size_t bytes) {
  *p = aligned_alloc(256, (bytes + 255) & ~(size_t)255);
  if (!*p) return hipErrorOutOfMemory;
  std::lock_guard<std::mutex> lk(g_mu);
  g_dev[(uintptr_t)*p] = bytes;
  return hipSuccess;
}
hipError_t hipFree(void *p) {
  if (!p) return hipSuccess;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    g_dev.erase((uintptr_t)p);
  }
  free(p);
  return hipSuccess;
}
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int) {
  *p = aligned_alloc(256, (bytes + 255) & ~(size_t)255);
  return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipHostFree(void *p) { free(p); return hipSuccess; }
hipError_t hipPointerGetAttributes(hipPointerAttribute_t *attr, const void *p) {
  uintptr_t base;
  size_t size;
  if (!find_alloc(p, &base, &size)) return hipErrorInvalidValue; // plain host memory
  memset(attr, 0, sizeof(*attr));
  attr->type = hipMemoryTypeDevice;
  attr->devicePointer = (void *)p;
  return hipSuccess;
}
hipError_t hipMemGetAddressRange(hipDeviceptr_t *base, size_t *size, hipDeviceptr_t p) {
  uintptr_t b;
  size_t s;
  if (!find_alloc((const void *)p, &b, &s)) return hipErrorInvalidValue;
  *base = (hipDeviceptr_t)b;
  *size = s;
  return hipSuccess;
}
hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind) {
  memcpy(dst, src, bytes);
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind, hipStream_t) {
  memcpy(dst, src, bytes);
  return hipSuccess;
}
hipError_t hipMemcpy2DAsync(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height,
                            hipMemcpyKind, hipStream_t) {
  for (size_t r = 0; r < height; ++r) memcpy((char *)dst + r * dpitch, (const char *)src + r * spitch, width);
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamIsCapturing(hipStream_t, hipStreamCaptureStatus *s) {
  *s = g_capturing.load(std::memory_order_relaxed) ? hipStreamCaptureStatusActive : hipStreamCaptureStatusNone;
  return hipSuccess;
}
int fake_hip_set_capturing(int on) { return g_capturing.exchange(on != 0, std::memory_order_relaxed); } // returns the answer before
long fake_hip_cu_mask_queries(void) { return g_cu_mask_queries.load(std::memory_order_relaxed); }
hipError_t hipExtStreamGetCUMask(hipStream_t, uint32_t n, uint32_t *m) {
  g_cu_mask_queries.fetch_add(1, std::memory_order_relaxed);
  const uint32_t cus = (uint32_t)fake_hip_cus();
  for (uint32_t i = 0; i < n; ++i) m[i] = cus >= 32 * (i + 1) ? 0xffffffffu : cus > 32 * i ? (1u << (cus - 32 * i)) - 1u : 0u;
  return hipSuccess;
}
hipError_t hipMemset(void *p, int v, size_t bytes) { memset(p, v, bytes); return hipSuccess; }
hipError_t hipMemsetAsync(void *p, int v, size_t bytes, hipStream_t) { memset(p, v, bytes); return hipSuccess; }
hipError_t hipDeviceGetAttribute(int *v, hipDeviceAttribute_t, int) { *v = fake_hip_cus(); return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { *e = nullptr; return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
}
