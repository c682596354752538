// k_wsola_lags, k_wsola_ola (kernels_wsola.h) and their launch.
#include "kernels_wsola.h"

namespace specinv {

template <typename T>
int wsola_launch(const T* x, const int64_t* centres, const T* window, int32_t* lags, T* y, int64_t batch, int64_t n_in,
                 int64_t n_out, int n_frames, int frame, int hop, int tol, hipStream_t stream) {
  SI_CHECK(x != nullptr && centres != nullptr && window != nullptr && lags != nullptr && y != nullptr && batch >= 1 && n_in >= 1 &&
               n_out >= 1 && n_frames >= 1 && frame >= 2 && frame <= kWsolaMaxFrame && !(frame & 1) && hop >= 1 && hop <= frame &&
               tol >= 0 && tol <= kWsolaMaxTol,
           SPECINV_EINVAL, "wsola: bad arguments");
  WsolaArgs a;
  a.n_in = n_in;
  a.n_out = n_out;
  a.tiles = ceil_div(n_out, kWsolaTile);
  a.n_frames = n_frames;
  a.frame = frame;
  a.hop = hop;
  a.tol = tol;
  a.len = frame + 2 * tol + hop + kWsolaPad;
  a.groups = (int)ceil_div(2 * tol + 1, kWsolaRun);
  const int wanted = kWsolaThreads / a.groups;                                        // >= 2: at most 228 groups
  a.slice_len = (int)ceil_div(ceil_div(frame, wanted), kWsolaRun) * kWsolaRun;
  a.slices = (int)ceil_div(frame, a.slice_len);                                       // <= wanted: no slice is empty
  const __int128 blocks = (__int128)batch * a.tiles;
  SI_CHECK(blocks < ((__int128)1 << 62) && (__int128)batch * n_frames < ((__int128)1 << 62), SPECINV_EINVAL,
           "wsola: %lld rows of %lld outputs exceed the launch grid", (long long)batch, (long long)n_out);
  const int64_t per_launch = (int64_t)1 << 22;
  if (tol == 0 || n_frames == 1) {
    SI_HIP(hipMemsetAsync(lags, 0, (size_t)batch * (size_t)n_frames * sizeof(int32_t), stream));
  } else {
    const size_t lds = ((size_t)kWsolaRun * kWsolaThreads + 16) * sizeof(double) + 2 * (size_t)a.len * sizeof(T);
    SI_HIP(hipFuncSetAttribute((const void*)k_wsola_lags<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    for (int64_t b0 = 0; b0 < batch; b0 += per_launch) {
      const int64_t nb = batch - b0 < per_launch ? batch - b0 : per_launch;
      hipLaunchKernelGGL((k_wsola_lags<T>), dim3((unsigned)nb), dim3(kWsolaThreads), lds, stream, x, centres, lags, b0, a);
      SI_HIP(hipGetLastError());
    }
  }
  for (int64_t b0 = 0; b0 < (int64_t)blocks; b0 += per_launch) {
    const int64_t nb = (int64_t)blocks - b0 < per_launch ? (int64_t)blocks - b0 : per_launch;
    hipLaunchKernelGGL((k_wsola_ola<T>), dim3((unsigned)nb), dim3(kWsolaTile), 0, stream, x, centres, window, lags, y, b0, a);
    SI_HIP(hipGetLastError());
  }
  return SPECINV_OK;
}

template int wsola_launch<float>(const float*, const int64_t*, const float*, int32_t*, float*, int64_t, int64_t, int64_t, int, int,
                                 int, int, hipStream_t);
template int wsola_launch<double>(const double*, const int64_t*, const double*, int32_t*, double*, int64_t, int64_t, int64_t, int,
                                  int, int, int, hipStream_t);

}  // namespace specinv
