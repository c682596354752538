// k_cgla_step_adjoint (kernels_cgla_adjoint.h) and its launch.
#include <algorithm>

#include "kernels_cgla_adjoint.h"

namespace specinv {

namespace {

template <typename T, int V>
int launch_v(const CglaAdjArgs<T>& p0, int batch, double* dots_dev, hipStream_t stream) {
  CglaAdjArgs<T> p = p0;
  p.upr = p.L / V;
  p.n_units = p.upr * batch;
  // memory-bound: eight workgroups of four waves per CU cover the chip, the rest is walked (tu_agla_adjoint.hip)
  const int n_wg = (int)std::min<int64_t>(ceil_div(p.n_units, 256), kAglaAdjMaxGrid);
  const dim3 grid((unsigned)n_wg), blk(256);
  if (p.gd != nullptr) hipLaunchKernelGGL((k_cgla_step_adjoint<T, V, true>), grid, blk, 0, stream, p);
  else hipLaunchKernelGGL((k_cgla_step_adjoint<T, V, false>), grid, blk, 0, stream, p);
  SI_HIP(hipGetLastError());
  if (p.first) return SPECINV_OK;
  return agla_dots_finish_launch(p.partials, n_wg, (double)p.gamma, dots_dev, stream);
}

}  // namespace

template <typename T>
int cgla_step_adjoint_launch(CglaAdjArgs<T> p, int batch, double* dots_dev, hipStream_t stream) {
  SI_CHECK(p.a != nullptr && p.gc != nullptr && p.goff != nullptr && p.env != nullptr && p.L >= 1 && batch >= 1, SPECINV_EINVAL,
           "cgla step adjoint: bad arguments");
  SI_CHECK(p.first || (p.tn != nullptr && p.tp != nullptr && p.c_prev != nullptr && p.partials != nullptr && dots_dev != nullptr),
           SPECINV_EINVAL, "cgla step adjoint: bad arguments");
  // samples per thread: every row (the cotangents, the t's, c_prev, the mask, the envelope) starts at a multiple of L elements from
  // an aligned base
  auto aligned = [](const void* q, int v) { return reinterpret_cast<uintptr_t>(q) % (v * sizeof(T)) == 0; };
  auto divides = [&](int v) {
    return p.L % v == 0 && aligned(p.a, v) && aligned(p.gc, v) && aligned(p.gd, v) && aligned(p.goff, v) && aligned(p.tn, v) &&
           aligned(p.tp, v) && aligned(p.tpp, v) && aligned(p.env, v) && aligned(p.c_prev, v) &&
           reinterpret_cast<uintptr_t>(p.mask) % v == 0;
  };
  if constexpr (sizeof(T) == 4) {
    if (divides(4)) return launch_v<T, 4>(p, batch, dots_dev, stream);
  }
  if (divides(2)) return launch_v<T, 2>(p, batch, dots_dev, stream);
  return launch_v<T, 1>(p, batch, dots_dev, stream);
}

template int cgla_step_adjoint_launch<float>(CglaAdjArgs<float>, int, double*, hipStream_t);
template int cgla_step_adjoint_launch<double>(CglaAdjArgs<double>, int, double*, hipStream_t);

}  // namespace specinv
