// k_misi_mix_adjoint, k_misi_proj_adjoint (kernels_misi_adjoint.h) and their launches.
#include <algorithm>

#include "kernels_misi_adjoint.h"

namespace specinv {

namespace {

// memory-bound: eight workgroups of four waves per CU cover the chip, the rest is walked
dim3 walk_grid(int64_t n_units) { return dim3((unsigned)std::min<int64_t>(ceil_div(n_units, 256), 256 * 8)); }

template <typename T, int V, bool DIV_ENV>
int launch_v(const MisiMixAdjArgs<T>& a0, int n_mix, hipStream_t stream) {
  MisiMixAdjArgs<T> a = a0;
  a.upr = a.L / V;
  a.n_units = a.upr * n_mix;
  if (a.n_units == 0) return SPECINV_OK;
  const dim3 grid = walk_grid(a.n_units), blk(256);
  switch (a.K) {
    case 2: hipLaunchKernelGGL((k_misi_mix_adjoint<T, 2, V, DIV_ENV>), grid, blk, 0, stream, a); break;
    case 3: hipLaunchKernelGGL((k_misi_mix_adjoint<T, 3, V, DIV_ENV>), grid, blk, 0, stream, a); break;
    case 4: hipLaunchKernelGGL((k_misi_mix_adjoint<T, 4, V, DIV_ENV>), grid, blk, 0, stream, a); break;
    default: hipLaunchKernelGGL((k_misi_mix_adjoint<T, 0, V, DIV_ENV>), grid, blk, 0, stream, a); break;
  }
  SI_HIP(hipGetLastError());
  return SPECINV_OK;
}

template <typename T, bool DIV_ENV>
int launch_env(const MisiMixAdjArgs<T>& a, int n_mix, hipStream_t stream) {
  const int v = misi_vec_width<T>(a.L, 0, {a.g, a.gmix, a.env});
  if constexpr (sizeof(T) == 4) {
    if (v == 4) return launch_v<T, 4, DIV_ENV>(a, n_mix, stream);
  }
  if (v == 2) return launch_v<T, 2, DIV_ENV>(a, n_mix, stream);
  return launch_v<T, 1, DIV_ENV>(a, n_mix, stream);
}

}  // namespace

template <typename T>
int misi_mix_adjoint_launch(MisiMixAdjArgs<T> a, int n_mix, hipStream_t stream) {
  SI_CHECK(a.g != nullptr && a.gmix != nullptr && a.K >= 1 && a.L >= 1 && n_mix >= 1, SPECINV_EINVAL, "misi mix adjoint: bad arguments");
  return a.env != nullptr ? launch_env<T, true>(a, n_mix, stream) : launch_env<T, false>(a, n_mix, stream);
}

template <typename T>
int misi_proj_adjoint_launch(MisiProjAdjArgs<T> a, hipStream_t stream) {
  SI_CHECK(a.y != nullptr && a.r != nullptr && a.m != nullptr && a.gm != nullptr && a.F >= 1 && a.total >= 0 && a.total % a.F == 0,
           SPECINV_EINVAL, "misi projection adjoint: bad arguments");
  if (a.total == 0) return SPECINV_OK;
  hipLaunchKernelGGL((k_misi_proj_adjoint<T>), walk_grid(a.total), dim3(256), 0, stream, a);
  SI_HIP(hipGetLastError());
  return SPECINV_OK;
}

template int misi_mix_adjoint_launch<float>(MisiMixAdjArgs<float>, int, hipStream_t);
template int misi_mix_adjoint_launch<double>(MisiMixAdjArgs<double>, int, hipStream_t);
template int misi_proj_adjoint_launch<float>(MisiProjAdjArgs<float>, hipStream_t);
template int misi_proj_adjoint_launch<double>(MisiProjAdjArgs<double>, hipStream_t);

}  // namespace specinv
