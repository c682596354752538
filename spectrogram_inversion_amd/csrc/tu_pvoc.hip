// k_phase_vocoder (kernels_pvoc.h) and its launch.
#include "kernels_pvoc.h"

namespace specinv {

template <typename T>
int pvoc_launch(const cplx<T>* in, cplx<T>* out, int batch, int n_freq, int n_in, int n_out, double rate, int n_fft, int hop,
                hipStream_t stream) {
  SI_CHECK(in != nullptr && out != nullptr && batch >= 1 && n_freq >= 1 && n_in >= 1 && n_fft >= 1 && hop >= 1, SPECINV_EINVAL,
           "phase vocoder: bad arguments");
  // the kernel reads source frames floor(j * rate) and the one after it for j < n_out: they stay below n_in + 1 only for this n_out
  SI_CHECK(pvoc_stretched_frames(n_in, rate) == (int64_t)n_out, SPECINV_EINVAL,
           "phase vocoder: %d output frames are not the stretched count of %d frames at rate %g", n_out, n_in, rate);
  const int64_t rows = (int64_t)batch * n_freq;
  SI_CHECK(rows <= 0x7fffffff - 4, SPECINV_EINVAL, "phase vocoder: %lld rows exceed the launch grid", (long long)rows);
  hipLaunchKernelGGL((k_phase_vocoder<T>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, in, out, (int)rows, n_freq,
                     n_in, n_out, rate, n_fft, hop);
  SI_HIP(hipGetLastError());
  return SPECINV_OK;
}

template int pvoc_launch<float>(const cplx<float>*, cplx<float>*, int, int, int, int, double, int, int, hipStream_t);
template int pvoc_launch<double>(const cplx<double>*, cplx<double>*, int, int, int, int, double, int, int, hipStream_t);

}  // namespace specinv
