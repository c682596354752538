// k_agla_step (kernels_agla.h) and its launch.
#include <algorithm>

#include "kernels_agla.h"

namespace specinv {

namespace {

template <typename T, int V>
int launch_v(const AglaStepArgs<T>& a0, int batch, hipStream_t stream) {
  AglaStepArgs<T> a = a0;
  a.upr = a.L / V;
  a.n_units = a.upr * batch;
  if (a.n_units == 0) return SPECINV_OK;
  // memory-bound: eight workgroups of four waves per CU cover the chip, the rest is walked
  const dim3 grid((unsigned)std::min<int64_t>(ceil_div(a.n_units, 256), 256 * 8)), blk(256);
  if (a.offset != nullptr) {
    if (a.d != nullptr) hipLaunchKernelGGL((k_agla_step<T, V, true, true>), grid, blk, 0, stream, a);
    else hipLaunchKernelGGL((k_agla_step<T, V, false, true>), grid, blk, 0, stream, a);
  } else {
    if (a.d != nullptr) hipLaunchKernelGGL((k_agla_step<T, V, true, false>), grid, blk, 0, stream, a);
    else hipLaunchKernelGGL((k_agla_step<T, V, false, false>), grid, blk, 0, stream, a);
  }
  SI_HIP(hipGetLastError());
  return SPECINV_OK;
}

}  // namespace

template <typename T>
int agla_step_launch(AglaStepArgs<T> a, int batch, hipStream_t stream) {
  SI_CHECK(a.x != nullptr && a.t != nullptr && (a.offset != nullptr || a.mask == nullptr) && a.L >= 1 && batch >= 1, SPECINV_EINVAL,
           "agla step: bad arguments");
  SI_CHECK(a.tail == nullptr || (a.hop >= 1 && a.nb >= 1 && a.nchunks >= 2 && a.n_frames >= 1), SPECINV_EINVAL,
           "agla step: bad tail geometry");
  const int v = misi_vec_width<T>(a.L, a.tail != nullptr ? a.hop : 0, {a.x, a.t, a.d, a.offset, a.tail}, a.mask);
  if constexpr (sizeof(T) == 4) {
    if (v == 4) return launch_v<T, 4>(a, batch, stream);
  }
  if (v == 2) return launch_v<T, 2>(a, batch, stream);
  return launch_v<T, 1>(a, batch, stream);
}

template int agla_step_launch<float>(AglaStepArgs<float>, int, hipStream_t);
template int agla_step_launch<double>(AglaStepArgs<double>, int, hipStream_t);

}  // namespace specinv
