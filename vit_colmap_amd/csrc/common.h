// Shared host-side helpers for the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <type_traits>

#include "../../include/vitcolmap_hip.h"

namespace vc {

inline int& last_hip_error_slot() {
  static thread_local int e = 0;
  return e;
}
inline int fail(hipError_t e) {
  last_hip_error_slot() = (int)e;
  return VC_ERR_LAUNCH;
}
// Launch errors are reported synchronously by hipGetLastError(); execution errors surface at
// the caller's next synchronisation (the ABI never synchronises).
inline int check_launch() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? VC_OK : fail(e);
}

// hipFuncSetAttribute applies to the CURRENT device only, so "this kernel is configured" is remembered
// per device (one bit per device ordinal), not per thread: a process that drives several GPUs
// configures every kernel once on each.
struct PerDeviceOnce {
  std::atomic<unsigned long long> done{0};
  template <typename F>
  int run(F configure) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return fail(e);
    const unsigned long long bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return VC_OK;
    e = configure();   // idempotent: two threads racing here both set the same attribute
    if (e != hipSuccess) return fail(e);
    done.fetch_or(bit, std::memory_order_release);
    return VC_OK;
  }
};

// Allows `kernels` up to `bytes` of dynamic LDS, once per device (`once` is the caller's static):
//   static vc::PerDeviceOnce configured;
//   if (int st = vc::allow_dynamic_lds(configured, bytes, kernel_a, kernel_b)) return st;
template <typename... Kernels>
int allow_dynamic_lds(PerDeviceOnce& once, int bytes, Kernels... kernels) {
  return once.run([=] {
    hipError_t e = hipSuccess;
    ((e = e == hipSuccess ? hipFuncSetAttribute((const void*)kernels, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) : e), ...);
    return e;
  });
}

// Compute units of the current device (sizes persistent grids).
inline int cu_count(int* cus) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e == hipSuccess && *cus <= 0) e = hipErrorInvalidDevice;
  return e == hipSuccess ? VC_OK : fail(e);
}

// Runtime value -> template argument: calls f(std::integral_constant<decltype(V), V>{}) for the first V in Vs equal to
// v and returns its status; VC_ERR_UNSUPPORTED when none is.  Only the listed values are instantiated.
template <auto... Vs, typename F>
int dispatch(int v, F&& f) {
  int st = VC_ERR_UNSUPPORTED;
  (void)((v == Vs && (st = f(std::integral_constant<decltype(Vs), Vs>{}), true)) || ...);
  return st;
}

}  // namespace vc
