// specinv_pvoc_pghi: the entry point, and the launch of k_pvoc_pghi (kernels_pvoc_pghi.h).
#include "entry.h"
#include "kernels_pvoc_pghi.h"

namespace specinv {

template <typename T, int K>
static int pvoc_pghi_run(const cplx<T>* in, cplx<T>* out, int8_t* parents_out, const PvocPghiArgs& a, hipStream_t stream) {
  const int64_t grid = a.batch < 65536 ? a.batch : 65536;
  hipLaunchKernelGGL((k_pvoc_pghi<T, kPghiThreads, K>), dim3((unsigned)grid), dim3(kPghiThreads), 0, stream, in, out, parents_out, a);
  SI_HIP(hipGetLastError());
  return SPECINV_OK;
}

// One launch; the grid is min(batch, 2^16) workgroups.
template <typename T>
static int pvoc_pghi_launch(const cplx<T>* in, cplx<T>* out, int8_t* parents_out, int64_t batch, int n_freq, int n_in, int n_out,
                            int n_fft, int hop, double rate, double tol, hipStream_t stream) {
  PvocPghiArgs a;
  a.batch = batch;
  a.n_freq = n_freq;
  a.n_in = n_in;
  a.n_out = n_out;
  a.n_fft = n_fft;
  a.hop = hop;
  a.rate = rate;
  a.tol = tol;
  switch ((int)ceil_div(n_freq, kPghiThreads) | 1) {                                  // bins per lane, odd: as k_pghi
    case 1: return pvoc_pghi_run<T, 1>(in, out, parents_out, a, stream);
    case 3: return pvoc_pghi_run<T, 3>(in, out, parents_out, a, stream);
    case 5: return pvoc_pghi_run<T, 5>(in, out, parents_out, a, stream);
    case 7: return pvoc_pghi_run<T, 7>(in, out, parents_out, a, stream);
    case 9: return pvoc_pghi_run<T, 9>(in, out, parents_out, a, stream);
    case 11: return pvoc_pghi_run<T, 11>(in, out, parents_out, a, stream);
    case 13: return pvoc_pghi_run<T, 13>(in, out, parents_out, a, stream);
  }
  return fail(SPECINV_EUNSUPPORTED, "pvoc_pghi: %d bins are more than %d per lane", n_freq, kPghiMaxChunk);
}

}  // namespace specinv

using namespace specinv;

extern "C" int specinv_pvoc_pghi(const void* spec_in, void* spec_out, int8_t* parents_out, int64_t batch, int32_t n_freq,
                                 int32_t n_frames_in, int32_t n_frames_out, int32_t n_fft, int32_t hop, double rate, double tol,
                                 int32_t dtype, int32_t device, void* hip_stream) {
  // (the argument errors before the device is touched, in the header's order)
  SI_CHECK(spec_in && spec_out, SPECINV_EINVAL, "specinv_pvoc_pghi: NULL %s", !spec_in ? "spec_in" : "spec_out");
  SI_CHECK(spec_out != spec_in, SPECINV_EINVAL, "specinv_pvoc_pghi: spec_out must not alias spec_in");
  SI_CHECK(batch >= 1 && n_freq >= 1 && n_frames_in >= 1 && n_frames_out >= 1 && n_fft >= 1, SPECINV_EINVAL,
           "specinv_pvoc_pghi: batch, n_freq, n_frames_in, n_frames_out and n_fft must be >= 1, got %lld, %d, %d, %d and %d",
           (long long)batch, n_freq, n_frames_in, n_frames_out, n_fft);
  SI_CHECK(n_freq == n_fft / 2 + 1, SPECINV_EINVAL,
           "specinv_pvoc_pghi: one-sided spectra only, n_freq = n_fft / 2 + 1; got n_fft %d and n_freq %d", n_fft, n_freq);
  SI_CHECK(hop >= 1, SPECINV_EINVAL, "specinv_pvoc_pghi: hop must be >= 1, got %d", hop);
  SI_CHECK(rate > 0 && std::isfinite(rate), SPECINV_EINVAL, "specinv_pvoc_pghi: rate must be finite and > 0, got %g", rate);
  const int64_t want = pvoc_stretched_frames(n_frames_in, rate);
  SI_CHECK(want == (int64_t)n_frames_out, SPECINV_EINVAL, "specinv_pvoc_pghi: n_frames_out is %d, %d frames at rate %g stretch to %lld",
           n_frames_out, n_frames_in, rate, (long long)want);
  SI_CHECK(tol > 0 && tol < 1, SPECINV_EINVAL, "specinv_pvoc_pghi: tol must be in (0, 1), got %g", tol);
  SI_CHECK_DTYPE(dtype);
  SI_CHECK(n_freq <= kPghiMaxFreq, SPECINV_EUNSUPPORTED, "specinv_pvoc_pghi: n_freq %d is beyond %d, the bins a workgroup holds", n_freq,
           kPghiMaxFreq);
  SI_ENTER_DEVICE(device, hip_stream);
  if (dtype == SPECINV_F32)
    return pvoc_pghi_launch<float>((const cplx<float>*)spec_in, (cplx<float>*)spec_out, parents_out, batch, n_freq, n_frames_in,
                                   n_frames_out, n_fft, hop, rate, tol, stream);
  return pvoc_pghi_launch<double>((const cplx<double>*)spec_in, (cplx<double>*)spec_out, parents_out, batch, n_freq, n_frames_in,
                                  n_frames_out, n_fft, hop, rate, tol, stream);
}
