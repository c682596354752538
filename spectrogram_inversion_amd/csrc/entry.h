// What the C ABI entry points share (host only): the device guard, and for the plan-free entries (each in its op's tu_*.hip,
// beside the launch) the device-enter step, the dtype check and the alias check.
#pragma once
#include "common.h"

namespace specinv {

// Calls run on the plan's (or the call's) device; the calling thread's current device (which torch reads back with hipGetDevice)
// is restored on every return path.
struct DeviceGuard {
  int prev = -1, want = -1;
  hipError_t enter(int device, int64_t* sink = nullptr) {
    want = device;
    bytes_sink() = sink;
    hipError_t e = hipGetDevice(&prev);
    if (e != hipSuccess) {
      prev = -1;
      return e;
    }
    if (prev == want) {
      prev = -1;                // nothing to restore
      return hipSuccess;
    }
    return hipSetDevice(want);
  }
  ~DeviceGuard() {
    bytes_sink() = nullptr;
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// A plan-free entry, once its argument checks have passed: enters `device` for the rest of the function and declares `stream`.
#define SI_ENTER_DEVICE(device, hip_stream) \
  DeviceGuard guard_;                       \
  SI_HIP(guard_.enter(device));             \
  hipStream_t stream = static_cast<hipStream_t>(hip_stream)

#define SI_CHECK_DTYPE(dtype) SI_CHECK((dtype) == SPECINV_F32 || (dtype) == SPECINV_F64, SPECINV_EINVAL, "bad dtype %d", dtype)

// p[first_out ... n) are the outputs: none that is given may equal an argument in front of it.  For SI_TRY.
inline int no_alias(const char* fn_name, const void* const* p, const char* const* names, int n, int first_out) {
  for (int i = first_out; i < n; ++i)
    for (int j = 0; j < i; ++j)
      SI_CHECK(p[i] == nullptr || p[i] != p[j], SPECINV_EINVAL, "%s: %s must not alias %s", fn_name, names[i], names[j]);
  return SPECINV_OK;
}

}  // namespace specinv
