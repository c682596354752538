// k_misi_mix (kernels_misi.h) and its launch.
#include <algorithm>

#include "kernels_misi.h"

namespace specinv {

namespace {

template <typename T, int V>
int launch_v(const MisiMixArgs<T>& a0, int n_mix, hipStream_t stream) {
  MisiMixArgs<T> a = a0;
  a.upr = a.L / V;
  a.n_units = a.upr * n_mix;
  if (a.n_units == 0) return SPECINV_OK;
  // memory-bound: eight workgroups of four waves per CU cover the chip, the rest is walked
  const dim3 grid((unsigned)std::min<int64_t>(ceil_div(a.n_units, 256), 256 * 8)), blk(256);
  switch (a.K) {
    case 2: hipLaunchKernelGGL((k_misi_mix<T, 2, V>), grid, blk, 0, stream, a); break;
    case 3: hipLaunchKernelGGL((k_misi_mix<T, 3, V>), grid, blk, 0, stream, a); break;
    case 4: hipLaunchKernelGGL((k_misi_mix<T, 4, V>), grid, blk, 0, stream, a); break;
    default: hipLaunchKernelGGL((k_misi_mix<T, 0, V>), grid, blk, 0, stream, a); break;
  }
  SI_HIP(hipGetLastError());
  return SPECINV_OK;
}

}  // namespace

template <typename T>
int misi_mix_launch(MisiMixArgs<T> a, int n_mix, hipStream_t stream) {
  SI_CHECK(a.x != nullptr && a.mix != nullptr && a.K >= 1 && a.L >= 1 && n_mix >= 1, SPECINV_EINVAL, "misi mix: bad arguments");
  SI_CHECK(a.tail == nullptr || (a.hop >= 1 && a.nb >= 1 && a.nchunks >= 2 && a.n_frames >= 1), SPECINV_EINVAL,
           "misi mix: bad tail geometry");
  const int v = misi_vec_width<T>(a.L, a.tail != nullptr ? a.hop : 0, {a.x, a.mix, a.tail});
  if constexpr (sizeof(T) == 4) {
    if (v == 4) return launch_v<T, 4>(a, n_mix, stream);
  }
  if (v == 2) return launch_v<T, 2>(a, n_mix, stream);
  return launch_v<T, 1>(a, n_mix, stream);
}

template int misi_mix_launch<float>(MisiMixArgs<float>, int, hipStream_t);
template int misi_mix_launch<double>(MisiMixArgs<double>, int, hipStream_t);

}  // namespace specinv
