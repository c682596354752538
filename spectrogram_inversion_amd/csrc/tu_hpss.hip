// k_hpss (kernels_hpss.h) and its launch.
#include "kernels_hpss.h"

namespace specinv {

template <typename T>
int hpss_launch(const T* spec, T* out_a, T* out_b, int64_t batch, int n_freq, int n_frames, int k_h, int k_p, double power,
                double m_h, double m_p, int mode, bool is_complex, hipStream_t stream) {
  SI_CHECK(spec != nullptr && out_a != nullptr && out_b != nullptr && batch >= 1 && n_freq >= 1 && n_frames >= 1 && k_h >= 1 &&
               k_h <= kHpssMaxWin && (k_h & 1) && k_p >= 1 && k_p <= kHpssMaxWin && (k_p & 1) && power > 0 && m_h >= 1 && m_p >= 1,
           SPECINV_EINVAL, "hpss: bad arguments");
  HpssArgs a;
  size_t lds = 0;
  a.tile_f = hpss_tile_rows(k_h, k_p, is_complex ? sizeof(double) : sizeof(T), &lds);
  SI_CHECK(lds <= (size_t)kHpssLdsBytes, SPECINV_EINVAL, "hpss: a tile of %zu bytes", lds);
  a.tiles_f = ceil_div(n_freq, a.tile_f);
  a.tiles_t = ceil_div(n_frames, kHpssTileT);
  a.n_freq = n_freq;
  a.n_frames = n_frames;
  a.k_h = k_h;
  a.k_p = k_p;
  a.mode = mode;
  a.power_kind = std::isinf(power) ? 3 : power == 1.0 ? 1 : power == 2.0 ? 2 : 0;
  a.split = m_h == 1.0 && m_p == 1.0;
  a.power = power;
  a.m_h = m_h;
  a.m_p = m_p;
  const __int128 blocks = (__int128)batch * a.tiles_f * a.tiles_t;
  SI_CHECK(blocks < ((__int128)1 << 62), SPECINV_EINVAL, "hpss: %lld items of %d x %d bins exceed the launch grid", (long long)batch,
           n_freq, n_frames);
  const int64_t per_launch = (int64_t)1 << 22;
  for (int64_t b0 = 0; b0 < (int64_t)blocks; b0 += per_launch) {
    const int64_t nb = (int64_t)blocks - b0 < per_launch ? (int64_t)blocks - b0 : per_launch;
    if (is_complex)
      hipLaunchKernelGGL((k_hpss<T, true>), dim3((unsigned)nb), dim3(kHpssThreads), lds, stream, spec, out_a, out_b, b0, a);
    else
      hipLaunchKernelGGL((k_hpss<T, false>), dim3((unsigned)nb), dim3(kHpssThreads), lds, stream, spec, out_a, out_b, b0, a);
    SI_HIP(hipGetLastError());
  }
  return SPECINV_OK;
}

template int hpss_launch<float>(const float*, float*, float*, int64_t, int, int, int, int, double, double, double, int, bool,
                                hipStream_t);
template int hpss_launch<double>(const double*, double*, double*, int64_t, int, int, int, int, double, double, double, int, bool,
                                 hipStream_t);

}  // namespace specinv
