// k_enhance (kernels_enhance.h) and its launch.
#include "kernels_enhance.h"

namespace specinv {

template <typename T, bool CPLX, bool FRAME_MAJOR, int RULE>
static int enhance_launch_k(const EnhArgs& a, hipStream_t stream) {
  const int64_t groups = FRAME_MAJOR ? a.batch * ceil_div(a.n_freq, kEnhBins) : ceil_div(a.batch * a.n_freq, kEnhBins);
  const unsigned grid = (unsigned)(groups < kEnhMaxGrid ? groups : kEnhMaxGrid);
  if (FRAME_MAJOR) {
    hipLaunchKernelGGL((k_enhance<T, CPLX, FRAME_MAJOR, RULE>), dim3(grid), dim3(kEnhBins), 0, stream, a);
  } else {
    static_assert(enhance_lds_bytes() <= 160 * 1024, "the tiles must fit a CU's LDS");
    if (enhance_lds_bytes() > 64 * 1024)
      SI_HIP(hipFuncSetAttribute((const void*)k_enhance<T, CPLX, FRAME_MAJOR, RULE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)enhance_lds_bytes()));
    hipLaunchKernelGGL((k_enhance<T, CPLX, FRAME_MAJOR, RULE>), dim3(grid), dim3(kEnhThreads), enhance_lds_bytes(), stream, a);
  }
  SI_HIP(hipGetLastError());
  return SPECINV_OK;
}

template <typename T, bool CPLX, bool FRAME_MAJOR>
static int enhance_launch_r(const EnhArgs& a, int rule, hipStream_t stream) {
  return rule == kEnhWiener ? enhance_launch_k<T, CPLX, FRAME_MAJOR, kEnhWiener>(a, stream)
                            : enhance_launch_k<T, CPLX, FRAME_MAJOR, kEnhLsa>(a, stream);
}

template <typename T, bool CPLX>
static int enhance_launch_l(const EnhArgs& a, bool frame_major, int rule, hipStream_t stream) {
  return frame_major ? enhance_launch_r<T, CPLX, true>(a, rule, stream) : enhance_launch_r<T, CPLX, false>(a, rule, stream);
}

int enhance_launch(const EnhArgs& a, bool is_double, bool is_complex, bool frame_major, int rule, hipStream_t stream) {
  SI_CHECK(a.spec != nullptr && a.batch >= 1 && a.n_freq >= 1 && a.n_frames >= 1 && a.init_frames >= 1 &&
               (rule == kEnhWiener || rule == kEnhLsa) && (a.noise_mode == kEnhNoiseTracked) == (a.noise_in == nullptr),
           SPECINV_EINVAL, "enhance: bad arguments");
  if (is_double)
    return is_complex ? enhance_launch_l<double, true>(a, frame_major, rule, stream)
                      : enhance_launch_l<double, false>(a, frame_major, rule, stream);
  return is_complex ? enhance_launch_l<float, true>(a, frame_major, rule, stream)
                    : enhance_launch_l<float, false>(a, frame_major, rule, stream);
}

}  // namespace specinv
