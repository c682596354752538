// k_cgla_step (kernels_cgla.h) and its launch.
#include <algorithm>

#include "kernels_cgla.h"

namespace specinv {

namespace {

template <typename T, int V>
int launch_v(const CglaStepArgs<T>& a0, int batch, hipStream_t stream) {
  CglaStepArgs<T> a = a0;
  a.upr = a.L / V;
  a.n_units = a.upr * batch;
  if (a.n_units == 0) return SPECINV_OK;
  // memory-bound: eight workgroups of four waves per CU cover the chip, the rest is walked (tu_agla.hip)
  const dim3 grid((unsigned)std::min<int64_t>(ceil_div(a.n_units, 256), 256 * 8)), blk(256);
  if (a.d != nullptr) hipLaunchKernelGGL((k_cgla_step<T, V, true>), grid, blk, 0, stream, a);
  else hipLaunchKernelGGL((k_cgla_step<T, V, false>), grid, blk, 0, stream, a);
  SI_HIP(hipGetLastError());
  return SPECINV_OK;
}

}  // namespace

template <typename T>
int cgla_step_launch(CglaStepArgs<T> a, int batch, hipStream_t stream) {
  SI_CHECK(a.x != nullptr && a.t != nullptr && a.offset != nullptr && a.L >= 1 && batch >= 1, SPECINV_EINVAL,
           "cgla step: bad arguments");
  SI_CHECK(a.tail == nullptr || (a.hop >= 1 && a.nb >= 1 && a.nchunks >= 2 && a.n_frames >= 1), SPECINV_EINVAL,
           "cgla step: bad tail geometry");
  // samples per thread: every row (x, t, d, offset, the mask, the tails) starts at a multiple of L (hop) elements from an aligned base
  auto aligned = [](const void* p, int v) { return reinterpret_cast<uintptr_t>(p) % (v * sizeof(T)) == 0; };
  auto divides = [&](int v) {
    return a.L % v == 0 && (a.tail == nullptr || a.hop % v == 0) && aligned(a.x, v) && aligned(a.t, v) && aligned(a.d, v) &&
           aligned(a.offset, v) && aligned(a.tail, v) && reinterpret_cast<uintptr_t>(a.mask) % v == 0;
  };
  if constexpr (sizeof(T) == 4) {
    if (divides(4)) return launch_v<T, 4>(a, batch, stream);
  }
  if (divides(2)) return launch_v<T, 2>(a, batch, stream);
  return launch_v<T, 1>(a, batch, stream);
}

template int cgla_step_launch<float>(CglaStepArgs<float>, int, hipStream_t);
template int cgla_step_launch<double>(CglaStepArgs<double>, int, hipStream_t);

}  // namespace specinv
