// k_resample (kernels_resample.h) and its launch.
#include "kernels_resample.h"

namespace specinv {

template <typename T>
int resample_launch(const T* x, T* y, int64_t batch, int64_t n_in, int64_t n_out, int64_t o, int64_t n, int width, double rolloff,
                    hipStream_t stream) {
  SI_CHECK(x != nullptr && y != nullptr && batch >= 1 && n_in >= 1 && n_out >= 1 && o >= 1 && n >= 1 && width >= 1 &&
               rolloff > 0 && rolloff <= 1,
           SPECINV_EINVAL, "resample: bad arguments");
  const double pi = 3.14159265358979323846;
  const double base = (double)(o < n ? o : n) * rolloff;
  const double half = std::ceil((double)width * (double)o / base);
  SI_CHECK(half < 1073741824.0, SPECINV_EINVAL, "resample: %lld:%lld at width %d reads %g samples per output", (long long)o,
           (long long)n, width, 2 * half + 1);
  ResampleArgs a;
  a.o = o;
  a.n = n;
  a.n_in = n_in;
  a.n_out = n_out;
  a.tiles = ceil_div(n_out, kResampleTile);
  a.J = (int)half;
  a.scale = base / (double)o / (double)n;
  a.delta = base / (double)o;
  a.width = (double)width;
  a.sin_d = std::sin(pi * a.delta);
  a.cos_d = std::cos(pi * a.delta);
  a.sin_w = std::sin(pi * a.delta / a.width);
  a.cos_w = std::cos(pi * a.delta / a.width);
  // the longest span a workgroup reads: its first and last centres lie at most (tile - 1) o / n + 1 apart, J samples either side
  const __int128 span = (__int128)(kResampleTile - 1) * o / n + 2 + 2 * (__int128)a.J + 1;
  const bool stage = span <= (__int128)(kResampleLdsBytes / sizeof(T));
  const __int128 blocks = (__int128)batch * a.tiles;
  SI_CHECK(blocks < ((__int128)1 << 62), SPECINV_EINVAL, "resample: %lld rows of %lld outputs exceed the launch grid",
           (long long)batch, (long long)n_out);
  const int64_t per_launch = (int64_t)1 << 22;
  for (int64_t b0 = 0; b0 < (int64_t)blocks; b0 += per_launch) {
    const int64_t nb = (int64_t)blocks - b0 < per_launch ? (int64_t)blocks - b0 : per_launch;
    if (stage)
      hipLaunchKernelGGL((k_resample<T, true>), dim3((unsigned)nb), dim3(kResampleTile), 0, stream, x, y, b0, a);
    else
      hipLaunchKernelGGL((k_resample<T, false>), dim3((unsigned)nb), dim3(kResampleTile), 0, stream, x, y, b0, a);
    SI_HIP(hipGetLastError());
  }
  return SPECINV_OK;
}

template int resample_launch<float>(const float*, float*, int64_t, int64_t, int64_t, int64_t, int64_t, int, double, hipStream_t);
template int resample_launch<double>(const double*, double*, int64_t, int64_t, int64_t, int64_t, int64_t, int, double, hipStream_t);

}  // namespace specinv
