// specinv_hpss: the entry point, and the launch of k_hpss (kernels_hpss.h).
#include "entry.h"
#include "kernels_hpss.h"

namespace specinv {

// Batch and the two tile counts are one flattened grid, in as many launches as 2^22 workgroups each take.
template <typename T>
static int hpss_launch(const T* spec, T* out_a, T* out_b, int64_t batch, int n_freq, int n_frames, int k_h, int k_p, double power,
                       double m_h, double m_p, int mode, bool is_complex, hipStream_t stream) {
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

}  // namespace specinv

using namespace specinv;

extern "C" int specinv_hpss(const void* spec, void* out_a, void* out_b, int64_t batch, int32_t n_freq, int32_t n_frames,
                            int32_t win_harm, int32_t win_perc, double power, double margin_harm, double margin_perc, int32_t out_mode,
                            int32_t is_complex, int32_t dtype, int32_t device, void* hip_stream) {
  // (the argument errors before the device is touched, in the header's order)
  SI_CHECK(spec && out_a && out_b, SPECINV_EINVAL, "specinv_hpss: NULL %s", !spec ? "spec" : !out_a ? "out_a" : "out_b");
  SI_CHECK(out_a != spec && out_b != spec && out_a != out_b, SPECINV_EINVAL, "specinv_hpss: %s",
           out_a == out_b ? "out_b must not alias out_a" : "an output must not alias spec");
  SI_CHECK(batch >= 1 && n_freq >= 1 && n_frames >= 1, SPECINV_EINVAL,
           "specinv_hpss: batch, n_freq and n_frames must be >= 1, got %lld, %d and %d", (long long)batch, n_freq, n_frames);
  SI_CHECK(win_harm >= 1 && win_harm <= kHpssMaxWin && (win_harm & 1), SPECINV_EINVAL,
           "specinv_hpss: win_harm must be odd in 1 ... %d, got %d", kHpssMaxWin, win_harm);
  SI_CHECK(win_perc >= 1 && win_perc <= kHpssMaxWin && (win_perc & 1), SPECINV_EINVAL,
           "specinv_hpss: win_perc must be odd in 1 ... %d, got %d", kHpssMaxWin, win_perc);
  SI_CHECK(power > 0, SPECINV_EINVAL, "specinv_hpss: power must be > 0 (inf included), got %g", power);
  SI_CHECK(margin_harm >= 1 && std::isfinite(margin_harm), SPECINV_EINVAL, "specinv_hpss: margin_harm must be finite and >= 1, got %g",
           margin_harm);
  SI_CHECK(margin_perc >= 1 && std::isfinite(margin_perc), SPECINV_EINVAL, "specinv_hpss: margin_perc must be finite and >= 1, got %g",
           margin_perc);
  SI_CHECK(out_mode == SPECINV_HPSS_COMPONENTS || out_mode == SPECINV_HPSS_MASKS || out_mode == SPECINV_HPSS_MEDIANS, SPECINV_EINVAL,
           "specinv_hpss: out_mode must be SPECINV_HPSS_COMPONENTS, _MASKS or _MEDIANS, got %d", out_mode);
  SI_CHECK_DTYPE(dtype);
  SI_ENTER_DEVICE(device, hip_stream);
  if (dtype == SPECINV_F32)
    return hpss_launch<float>((const float*)spec, (float*)out_a, (float*)out_b, batch, n_freq, n_frames, win_harm, win_perc, power,
                              margin_harm, margin_perc, out_mode, is_complex != 0, stream);
  return hpss_launch<double>((const double*)spec, (double*)out_a, (double*)out_b, batch, n_freq, n_frames, win_harm, win_perc, power,
                             margin_harm, margin_perc, out_mode, is_complex != 0, stream);
}
