// DevBuf: the one owner of device memory in the library (plan_impl.h, fast_state.h, lbfgs_dev.h, tu_mel_nnls.hip).
#pragma once
#include "common.h"

namespace specinv {

// Grow-only hipMalloc holder whose bytes are charged to the plan the ABI call entered (account_bytes).  A zero-byte request
// still allocates (and is charged) 16 bytes, so that `p` is always a valid device pointer.
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) {
      (void)hipFree(p);
      account_bytes(-(int64_t)bytes);
    }
    p = nullptr;
    bytes = 0;
  }
  // grow-only allocation
  int reserve(size_t n) {
    if (n <= bytes && p) return SPECINV_OK;
    release();
    if (n == 0) n = 16;
    hipError_t e = hipMalloc(&p, n);
    if (e != hipSuccess) {
      p = nullptr;
      return fail(SPECINV_ENOMEM, "hipMalloc(%zu bytes) failed: %s", n, hipGetErrorString(e));
    }
    bytes = n;
    account_bytes((int64_t)n);
    return SPECINV_OK;
  }
  template <typename U>
  U* as() const { return static_cast<U*>(p); }
};

}  // namespace specinv
