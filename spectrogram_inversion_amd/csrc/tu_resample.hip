// specinv_resample: the entry point, and the launch of k_resample (kernels_resample.h).
#include "entry.h"
#include "kernels_resample.h"

namespace specinv {

template <typename T>
static int resample_launch(const T* x, T* y, int64_t batch, int64_t n_in, int64_t n_out, int64_t o, int64_t n, int width,
                           double rolloff, hipStream_t stream) {
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

}  // namespace specinv

using namespace specinv;

extern "C" int specinv_resample(const void* x, void* y, int64_t batch, int64_t n_in, int64_t n_out, int64_t orig_freq, int64_t new_freq,
                                int32_t lowpass_filter_width, double rolloff, int32_t dtype, int32_t device, void* hip_stream) {
  // (the argument errors before the device is touched)
  SI_CHECK(x && y, SPECINV_EINVAL, "specinv_resample: NULL %s", x ? "y" : "x");
  SI_CHECK(x != y, SPECINV_EINVAL, "specinv_resample: y must not alias x");
  SI_CHECK(batch >= 1 && n_in >= 1, SPECINV_EINVAL, "specinv_resample: batch and n_in must be >= 1, got %lld and %lld",
           (long long)batch, (long long)n_in);
  SI_CHECK(orig_freq >= 1 && new_freq >= 1, SPECINV_EINVAL, "specinv_resample: orig_freq and new_freq must be >= 1, got %lld and %lld",
           (long long)orig_freq, (long long)new_freq);
  SI_CHECK(lowpass_filter_width >= 1, SPECINV_EINVAL, "lowpass_filter_width must be >= 1, got %d", lowpass_filter_width);
  SI_CHECK(rolloff > 0 && rolloff <= 1, SPECINV_EINVAL, "rolloff must be in (0, 1], got %g", rolloff);
  int64_t g = orig_freq, t = new_freq;
  while (t != 0) {
    const int64_t u = g % t;
    g = t;
    t = u;
  }
  const int64_t o = orig_freq / g, n = new_freq / g;
  const __int128 want = ((__int128)n * n_in + o - 1) / o;
  // (the kernel forms m * o for every output m in 64 bits)
  SI_CHECK(want < ((__int128)1 << 62) && want * o < ((__int128)1 << 62), SPECINV_EINVAL,
           "specinv_resample: %lld samples at %lld:%lld index beyond 62 bits", (long long)n_in, (long long)o, (long long)n);
  SI_CHECK((__int128)n_out == want, SPECINV_EINVAL, "specinv_resample: n_out is %lld, %lld samples at %lld:%lld give %lld",
           (long long)n_out, (long long)n_in, (long long)o, (long long)n, (long long)want);
  SI_CHECK_DTYPE(dtype);
  SI_ENTER_DEVICE(device, hip_stream);
  if (o == n) {                           // the same rate: a copy
    SI_HIP(hipMemcpyAsync(y, x, (size_t)batch * (size_t)n_in * (dtype == SPECINV_F32 ? 4 : 8), hipMemcpyDeviceToDevice, stream));
    return SPECINV_OK;
  }
  if (dtype == SPECINV_F32)
    return resample_launch<float>((const float*)x, (float*)y, batch, n_in, n_out, o, n, lowpass_filter_width, rolloff, stream);
  return resample_launch<double>((const double*)x, (double*)y, batch, n_in, n_out, o, n, lowpass_filter_width, rolloff, stream);
}
