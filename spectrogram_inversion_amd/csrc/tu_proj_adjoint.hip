// k_wave_proj_adjoint and k_project (kernels_proj_adjoint.h) and their launches.
#include "kernels_proj_adjoint.h"

namespace specinv {

bool proj_adjoint_covers(int n_fft, int elem_size) {
  return (elem_size == 4 || elem_size == 8) && (n_fft == 128 || n_fft == 256 || n_fft == 512 || n_fft == 1024 || n_fft == 2048);
}

template <typename T>
int proj_adjoint_launch(const ProjAdjArgs<T>& a, hipStream_t stream) {
  SI_CHECK(a.x && a.g && a.env && a.mag && a.gmag && a.frames && a.batch >= 1 && a.c.n_frames >= 1, SPECINV_EINVAL,
           "projection adjoint: bad arguments");
  SI_CHECK(a.c.onesided && a.c.n_freq == a.c.n_fft / 2 + 1, SPECINV_EUNSUPPORTED, "k_wave_proj_adjoint takes one-sided spectrograms");
  switch (a.c.n_fft) {
    case 128: return wave::proj_adjoint_launch_one<T, 6>(a, stream);
    case 256: return wave::proj_adjoint_launch_one<T, 7>(a, stream);
    case 512: return wave::proj_adjoint_launch_one<T, 8>(a, stream);
    case 1024: return wave::proj_adjoint_launch_one<T, 9>(a, stream);
    case 2048: return wave::proj_adjoint_launch_one<T, 10>(a, stream);
    default: break;
  }
  SI_CHECK(false, SPECINV_EUNSUPPORTED, "k_wave_proj_adjoint does not cover n_fft=%d", a.c.n_fft);
  return SPECINV_EUNSUPPORTED;
}

template <typename T>
int project_launch(cplx<T>* spec, const T* mag_fm, int64_t n, hipStream_t stream) {
  SI_CHECK(spec && mag_fm && n >= 1, SPECINV_EINVAL, "projection: bad arguments");
  hipLaunchKernelGGL((k_project<T>), dim3((unsigned)std::min<int64_t>(ceil_div(n, 256), 8192)), dim3(256), 0, stream, spec, mag_fm, n);
  SI_HIP(hipGetLastError());
  return SPECINV_OK;
}

template int proj_adjoint_launch<float>(const ProjAdjArgs<float>&, hipStream_t);
template int proj_adjoint_launch<double>(const ProjAdjArgs<double>&, hipStream_t);
template int project_launch<float>(cplx<float>*, const float*, int64_t, hipStream_t);
template int project_launch<double>(cplx<double>*, const double*, int64_t, hipStream_t);

}  // namespace specinv
