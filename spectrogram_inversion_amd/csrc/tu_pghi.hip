// specinv_pghi: the entry point, and the launch of k_pghi (kernels_pghi.h).
#include "entry.h"
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

// One launch; the grid is min(batch, 2^16) workgroups.
template <typename T>
static int pghi_launch(const T* mag, cplx<T>* out, double* phase_out, int8_t* parents_out, int64_t batch, int n_freq, int n_frames,
                       int n_fft, int hop, double gamma, double tol, hipStream_t stream) {
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

}  // namespace specinv

using namespace specinv;

extern "C" int specinv_pghi(const void* mag, void* spec_out, double* phase_out, int8_t* parents_out, int64_t batch, int32_t n_freq,
                            int32_t n_frames, int32_t n_fft, int32_t hop, double gamma, double tol, int32_t dtype, int32_t device,
                            void* hip_stream) {
  // (the argument errors before the device is touched, in the header's order)
  SI_CHECK(mag && spec_out, SPECINV_EINVAL, "specinv_pghi: NULL %s", !mag ? "mag" : "spec_out");
  SI_CHECK(spec_out != mag, SPECINV_EINVAL, "specinv_pghi: spec_out must not alias mag");
  SI_CHECK(batch >= 1 && n_freq >= 1 && n_frames >= 1, SPECINV_EINVAL,
           "specinv_pghi: batch, n_freq and n_frames must be >= 1, got %lld, %d and %d", (long long)batch, n_freq, n_frames);
  SI_CHECK(n_fft >= 2 && !(n_fft & 1) && n_freq == n_fft / 2 + 1, SPECINV_EINVAL,
           "specinv_pghi: n_fft must be even and n_freq = n_fft / 2 + 1, got n_fft %d and n_freq %d", n_fft, n_freq);
  SI_CHECK(hop >= 1, SPECINV_EINVAL, "specinv_pghi: hop must be >= 1, got %d", hop);
  SI_CHECK(gamma > 0 && gamma <= 1.7976931348623157e308, SPECINV_EINVAL, "specinv_pghi: gamma must be finite and > 0, got %g", gamma);
  SI_CHECK(tol > 0 && tol < 1, SPECINV_EINVAL, "specinv_pghi: tol must be in (0, 1), got %g", tol);
  SI_CHECK_DTYPE(dtype);
  SI_CHECK(n_fft <= kPghiMaxFft, SPECINV_EUNSUPPORTED, "specinv_pghi: n_fft %d is beyond %d, where a frame's state fills the LDS",
           n_fft, kPghiMaxFft);
  SI_ENTER_DEVICE(device, hip_stream);
  if (dtype == SPECINV_F32)
    return pghi_launch<float>((const float*)mag, (cplx<float>*)spec_out, phase_out, parents_out, batch, n_freq, n_frames, n_fft, hop,
                              gamma, tol, stream);
  return pghi_launch<double>((const double*)mag, (cplx<double>*)spec_out, phase_out, parents_out, batch, n_freq, n_frames, n_fft,
                             hop, gamma, tol, stream);
}
