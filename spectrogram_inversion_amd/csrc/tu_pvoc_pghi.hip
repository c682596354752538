// k_pvoc_pghi (kernels_pvoc_pghi.h) and its launch.
#include "kernels_pvoc_pghi.h"

namespace specinv {

template <typename T, int K>
static int pvoc_pghi_run(const cplx<T>* in, cplx<T>* out, int8_t* parents_out, const PvocPghiArgs& a, hipStream_t stream) {
  const int64_t grid = a.batch < 65536 ? a.batch : 65536;
  hipLaunchKernelGGL((k_pvoc_pghi<T, kPghiThreads, K>), dim3((unsigned)grid), dim3(kPghiThreads), 0, stream, in, out, parents_out, a);
  SI_HIP(hipGetLastError());
  return SPECINV_OK;
}

template <typename T>
int pvoc_pghi_launch(const cplx<T>* in, cplx<T>* out, int8_t* parents_out, int64_t batch, int n_freq, int n_in, int n_out,
                     int n_fft, int hop, double rate, double tol, hipStream_t stream) {
  SI_CHECK(in != nullptr && out != nullptr && batch >= 1 && n_in >= 1 && n_out >= 1 && n_fft >= 1 && n_freq == n_fft / 2 + 1 &&
               n_freq <= kPghiMaxFreq && hop >= 1 && rate > 0 && tol > 0 && tol < 1 &&
               (int64_t)n_out == pvoc_stretched_frames(n_in, rate),
           SPECINV_EINVAL, "pvoc_pghi: bad arguments");
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

template int pvoc_pghi_launch<float>(const cplx<float>*, cplx<float>*, int8_t*, int64_t, int, int, int, int, int, double, double,
                                     hipStream_t);
template int pvoc_pghi_launch<double>(const cplx<double>*, cplx<double>*, int8_t*, int64_t, int, int, int, int, int, double, double,
                                      hipStream_t);

}  // namespace specinv
