// k_agla_step_adjoint, k_agla_dots_finish (kernels_agla_adjoint.h) and their launch.
#include <algorithm>

#include "kernels_agla_adjoint.h"

namespace specinv {

namespace {

// One workgroup: thread j sums the partial triples j, j + 256, ... in that order, the 256 sums are added like a workgroup's above,
// gamma's sum is divided by gamma_n.  The same partials in the same order at every call: the result is deterministic.
__global__ void __launch_bounds__(256) k_agla_dots_finish(const double* partials, int n_part, double gamma, double* out) {
  __shared__ double red[3][4];
  double s[3] = {0, 0, 0};
  for (int j = threadIdx.x; j < n_part; j += 256) {
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] += partials[(int64_t)j * 3 + k];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) s[k] = wave_scan_inclusive(s[k]);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 63) {
#pragma unroll
    for (int k = 0; k < 3; ++k) red[k][wave] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const double* r = red[threadIdx.x];
    const double tot = ((r[0] + r[1]) + r[2]) + r[3];
    out[threadIdx.x] = threadIdx.x == 2 ? tot / gamma : tot;
  }
}

template <typename T, int V>
int launch_v(const AglaAdjArgs<T>& p0, int batch, double* dots_dev, hipStream_t stream) {
  AglaAdjArgs<T> p = p0;
  p.upr = p.L / V;
  p.n_units = p.upr * batch;
  // memory-bound: eight workgroups of four waves per CU cover the chip, the rest is walked
  const int n_wg = (int)std::min<int64_t>(ceil_div(p.n_units, 256), kAglaAdjMaxGrid);
  const dim3 grid((unsigned)n_wg), blk(256);
  if (p.goff != nullptr) {
    if (p.gd != nullptr) hipLaunchKernelGGL((k_agla_step_adjoint<T, V, true, true>), grid, blk, 0, stream, p);
    else hipLaunchKernelGGL((k_agla_step_adjoint<T, V, false, true>), grid, blk, 0, stream, p);
  } else {
    if (p.gd != nullptr) hipLaunchKernelGGL((k_agla_step_adjoint<T, V, true, false>), grid, blk, 0, stream, p);
    else hipLaunchKernelGGL((k_agla_step_adjoint<T, V, false, false>), grid, blk, 0, stream, p);
  }
  SI_HIP(hipGetLastError());
  if (p.first) return SPECINV_OK;
  hipLaunchKernelGGL(k_agla_dots_finish, dim3(1), dim3(256), 0, stream, p.partials, n_wg, (double)p.gamma, dots_dev);
  SI_HIP(hipGetLastError());
  return SPECINV_OK;
}

}  // namespace

template <typename T>
int agla_step_adjoint_launch(AglaAdjArgs<T> p, int batch, double* dots_dev, hipStream_t stream) {
  SI_CHECK(p.a != nullptr && p.gc != nullptr && (p.goff != nullptr || p.mask == nullptr) && p.env != nullptr && p.L >= 1 && batch >= 1,
           SPECINV_EINVAL, "agla step adjoint: bad arguments");
  SI_CHECK(p.first || (p.tn != nullptr && p.tp != nullptr && p.c_prev != nullptr && p.partials != nullptr && dots_dev != nullptr),
           SPECINV_EINVAL, "agla step adjoint: bad arguments");
  const int v = misi_vec_width<T>(p.L, 0, {p.a, p.gc, p.gd, p.goff, p.tn, p.tp, p.tpp, p.env, p.c_prev}, p.mask);
  if constexpr (sizeof(T) == 4) {
    if (v == 4) return launch_v<T, 4>(p, batch, dots_dev, stream);
  }
  if (v == 2) return launch_v<T, 2>(p, batch, dots_dev, stream);
  return launch_v<T, 1>(p, batch, dots_dev, stream);
}

template int agla_step_adjoint_launch<float>(AglaAdjArgs<float>, int, double*, hipStream_t);
template int agla_step_adjoint_launch<double>(AglaAdjArgs<double>, int, double*, hipStream_t);

}  // namespace specinv
