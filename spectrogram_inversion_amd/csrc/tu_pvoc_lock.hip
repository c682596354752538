// k_pvoc_lock_scan / k_pvoc_lock_apply (kernels_pvoc_lock.h) and their launch.
#include "kernels_pvoc_lock.h"

namespace specinv {

template <typename T>
int pvoc_lock_launch(const cplx<T>* in, cplx<T>* out, double* phi, int batch, int n_freq, int n_in, int n_out, double rate,
                     int n_fft, int hop, bool two_sided, hipStream_t stream) {
  SI_CHECK(in != nullptr && out != nullptr && phi != nullptr && batch >= 1 && n_freq >= 2 && n_in >= 1 && n_fft >= 2 && hop >= 1,
           SPECINV_EINVAL, "locked phase vocoder: bad arguments");
  SI_CHECK(n_freq == (two_sided ? n_fft : n_fft / 2 + 1), SPECINV_EINVAL, "locked phase vocoder: %d bins are not those of n_fft %d",
           n_freq, n_fft);
  // both kernels read source frames floor(j * rate) and the one after it for j < n_out: they stay below n_in + 1 only for this n_out
  SI_CHECK(pvoc_stretched_frames(n_in, rate) == (int64_t)n_out, SPECINV_EINVAL,
           "locked phase vocoder: %d output frames are not the stretched count of %d frames at rate %g", n_out, n_in, rate);
  const int64_t rows = (int64_t)batch * n_freq;
  SI_CHECK(rows <= 0x7fffffff - 4, SPECINV_EINVAL, "locked phase vocoder: %lld rows exceed the launch grid", (long long)rows);
  const int chunks = (n_out + 63) / 64;
  const int bands = (n_freq + kPvocLockBand - 1) / kPvocLockBand;
  const int64_t waves = (int64_t)batch * chunks * bands;
  SI_CHECK(waves <= 0x7fffffff - 4, SPECINV_EINVAL, "locked phase vocoder: %lld waves exceed the launch grid", (long long)waves);
  hipLaunchKernelGGL((k_pvoc_lock_scan<T>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, in, phi, (int)rows, n_freq,
                     n_in, n_out, rate, n_fft, hop);
  SI_HIP(hipGetLastError());
  hipLaunchKernelGGL((k_pvoc_lock_apply<T>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, stream, in, (const double*)phi, out,
                     batch, n_freq, n_in, n_out, rate, two_sided ? 1 : 0, chunks, bands);
  SI_HIP(hipGetLastError());
  return SPECINV_OK;
}

template int pvoc_lock_launch<float>(const cplx<float>*, cplx<float>*, double*, int, int, int, int, double, int, int, bool,
                                     hipStream_t);
template int pvoc_lock_launch<double>(const cplx<double>*, cplx<double>*, double*, int, int, int, int, double, int, int, bool,
                                      hipStream_t);

}  // namespace specinv
