// free_call.hpp — the scaffold of a call that takes no problem handle and owns its device memory (camera.cpp, chart.cpp, fit.cpp,
// imu_align.cpp, rig.cpp, camera_align.cpp, accel_align.cpp, allan.cpp): where its message goes, how it picks its device, and its buffers. (The three
// alignment calls share more: align_host.hpp.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>

#include "../../include/calico_hip.h"

namespace cal {

// calico_hip.cpp: the calling thread's message of its last non-OK call without a handle (calico_last_error(NULL)); a success keeps it
std::string& handle_free_error();

struct FreeCall {
  const char* name;
  int fail(int code, const std::string& msg) const { handle_free_error() = std::string(name) + ": " + msg; return code; }
  int invalid(const std::string& msg) const { return fail(CALICO_INVALID_ARGUMENT, msg); }
  int hip(hipError_t e) const { return fail(CALICO_INTERNAL, hipGetErrorString(e)); }
  int select_device(int device) const {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count || hipSetDevice(device) != hipSuccess)
      return fail(CALICO_INTERNAL, "no usable HIP device " + std::to_string(device));
    return CALICO_OK;
  }
};
#define FREE_TRY(call, x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return (call).hip(e_); } while (0)

// One hipMalloc per buffer, freed with the call. n == 0 allocates one element: a kernel argument is never null.
template <class T> struct FreeBuf {
  T* p = nullptr;
  ~FreeBuf() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t n) { return hipMalloc(reinterpret_cast<void**>(&p), (n ? n : 1) * sizeof(T)); }
  hipError_t put(const T* src, size_t n) { return n == 0 ? hipSuccess : hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice); }      // (n fits what was allocated)
  hipError_t upload(const T* src, size_t n) { const hipError_t e = alloc(n); return e != hipSuccess ? e : put(src, n); }      // allocates
  hipError_t download(T* dst, size_t n) const { return n == 0 ? hipSuccess : hipMemcpy(dst, p, n * sizeof(T), hipMemcpyDeviceToHost); }
  hipError_t zero(size_t n) { return hipMemset(p, 0, (n ? n : 1) * sizeof(T)); }
};

}  // namespace cal
