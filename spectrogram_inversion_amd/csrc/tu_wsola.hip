// specinv_wsola: the entry point, and the launch of k_wsola_lags and k_wsola_ola (kernels_wsola.h).
#include "entry.h"
#include "kernels_wsola.h"

namespace specinv {

// lags is always written (zeros without a chain: tol 0 or one frame).  Batch is part of grid x, in as many launches as 2^22
// workgroups each take.
template <typename T>
static int wsola_launch(const T* x, const int64_t* centres, const T* window, int32_t* lags, T* y, int64_t batch, int64_t n_in,
                        int64_t n_out, int n_frames, int frame, int hop, int tol, hipStream_t stream) {
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

}  // namespace specinv

using namespace specinv;

extern "C" int specinv_wsola(const void* x, const int64_t* centres, const void* window, int32_t* lags, void* y, int64_t batch,
                             int64_t n_in, int64_t n_out, int32_t n_frames, int32_t frame, int32_t hop, int32_t tol, int32_t dtype,
                             int32_t device, void* hip_stream) {
  // (the argument errors before the device is touched, in the header's order)
  SI_CHECK(x && centres && window && lags && y, SPECINV_EINVAL, "specinv_wsola: NULL %s",
           !x ? "x" : !centres ? "centres" : !window ? "window" : !lags ? "lags" : "y");
  SI_CHECK(y != x, SPECINV_EINVAL, "specinv_wsola: y must not alias x");
  SI_CHECK(batch >= 1 && n_in >= 1 && n_out >= 1, SPECINV_EINVAL,
           "specinv_wsola: batch, n_in and n_out must be >= 1, got %lld, %lld and %lld", (long long)batch, (long long)n_in,
           (long long)n_out);
  SI_CHECK(frame >= 2 && frame <= kWsolaMaxFrame && !(frame & 1), SPECINV_EINVAL, "specinv_wsola: frame must be even in 2 ... %d, got %d",
           kWsolaMaxFrame, frame);
  SI_CHECK(hop >= 1 && hop <= frame, SPECINV_EINVAL, "specinv_wsola: hop must be in 1 ... frame = %d, got %d", frame, hop);
  SI_CHECK(tol >= 0 && tol <= kWsolaMaxTol, SPECINV_EINVAL, "specinv_wsola: tol must be in 0 ... %d, got %d", kWsolaMaxTol, tol);
  const __int128 want = ((__int128)n_out - 1 + frame / 2) / hop + 1;
  SI_CHECK((__int128)n_frames == want, SPECINV_EINVAL, "specinv_wsola: n_frames is %d, %lld outputs at frame %d and hop %d take %lld",
           n_frames, (long long)n_out, frame, hop, (long long)want);
  SI_CHECK_DTYPE(dtype);
  SI_ENTER_DEVICE(device, hip_stream);
  if (dtype == SPECINV_F32)
    return wsola_launch<float>((const float*)x, centres, (const float*)window, lags, (float*)y, batch, n_in, n_out, n_frames, frame,
                               hop, tol, stream);
  return wsola_launch<double>((const double*)x, centres, (const double*)window, lags, (double*)y, batch, n_in, n_out, n_frames,
                              frame, hop, tol, stream);
}
