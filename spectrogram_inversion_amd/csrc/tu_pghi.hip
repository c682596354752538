// k_pghi (kernels_pghi.h) and its launch.
#include "kernels_pghi.h"

namespace specinv {

template <typename T, int K>
static int pghi_run(const T* mag, cplx<T>* out, double* phase_out, int8_t* parents_out, const PghiArgs& a, hipStream_t stream) {
  const size_t lds = pghi_lds_bytes(a.n_freq, sizeof(T));
  SI_HIP(hipFuncSetAttribute((const void*)k_pghi<T, kPghiThreads, K>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int64_t grid = a.batch < 65536 ? a.batch : 65536;
  hipLaunchKernelGGL((k_pghi<T, kPghiThreads, K>), dim3((unsigned)grid), dim3(kPghiThreads), lds, stream, mag, out, phase_out,
                     parents_out, a);
  SI_HIP(hipGetLastError());
  return SPECINV_OK;
}

template <typename T>
int pghi_launch(const T* mag, cplx<T>* out, double* phase_out, int8_t* parents_out, int64_t batch, int n_freq, int n_frames,
                int n_fft, int hop, double gamma, double tol, hipStream_t stream) {
  SI_CHECK(mag != nullptr && out != nullptr && batch >= 1 && n_frames >= 1 && n_fft >= 2 && !(n_fft & 1) && n_freq == n_fft / 2 + 1 &&
               n_freq <= kPghiMaxFreq && hop >= 1 && gamma > 0 && tol > 0 && tol < 1,
           SPECINV_EINVAL, "pghi: bad arguments");
  PghiArgs a;
  a.batch = batch;
  a.n_freq = n_freq;
  a.n_frames = n_frames;
  a.n_fft = n_fft;
  a.hop_mod = (unsigned)(hop % n_fft);
  a.kt = (double)hop * (double)n_fft / gamma;
  a.kf = gamma / ((double)hop * (double)n_fft);
  a.w0 = 2.0 * 3.14159265358979323846 / (double)n_fft;
  a.tol = tol;
  switch ((int)ceil_div(n_freq, kPghiThreads) | 1) {                                  // bins per lane, odd: see the kernel's layout
    case 1: return pghi_run<T, 1>(mag, out, phase_out, parents_out, a, stream);
    case 3: return pghi_run<T, 3>(mag, out, phase_out, parents_out, a, stream);
    case 5: return pghi_run<T, 5>(mag, out, phase_out, parents_out, a, stream);
    case 7: return pghi_run<T, 7>(mag, out, phase_out, parents_out, a, stream);
    case 9: return pghi_run<T, 9>(mag, out, phase_out, parents_out, a, stream);
    case 11: return pghi_run<T, 11>(mag, out, phase_out, parents_out, a, stream);
    case 13: return pghi_run<T, 13>(mag, out, phase_out, parents_out, a, stream);
  }
  return fail(SPECINV_EUNSUPPORTED, "pghi: %d bins are more than %d per lane", n_freq, kPghiMaxChunk);
}

template int pghi_launch<float>(const float*, cplx<float>*, double*, int8_t*, int64_t, int, int, int, int, double, double, hipStream_t);
template int pghi_launch<double>(const double*, cplx<double>*, double*, int8_t*, int64_t, int, int, int, int, double, double,
                                 hipStream_t);

}  // namespace specinv
