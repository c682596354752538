// k_beamform (kernels_beamform.h) and its launch.
#include "kernels_beamform.h"

namespace specinv {

template <typename T, int NE>
static int beamform_launch_k(const BfArgs& a, hipStream_t stream) {
  const BfGeom g = bf_geom(a.channels, (int)sizeof(T));
  const size_t lds = sizeof(double) * (size_t)g.wave_doubles * kBfWaves;
  SI_CHECK(lds <= 160 * 1024, SPECINV_EUNSUPPORTED, "beamform: %d channels need %zu bytes of LDS", a.channels, lds);
  const int64_t groups = ceil_div(a.batch * a.n_freq, kBfWaves);
  const unsigned grid = (unsigned)(groups < kBfMaxGrid ? groups : kBfMaxGrid);
  if (lds > 64 * 1024)
    SI_HIP(hipFuncSetAttribute((const void*)k_beamform<T, NE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((k_beamform<T, NE>), dim3(grid), dim3(kBfThreads), lds, stream, a);
  SI_HIP(hipGetLastError());
  return SPECINV_OK;
}

int beamform_launch(const BfArgs& a, bool is_double, hipStream_t stream) {
  SI_CHECK(a.spec != nullptr && a.batch >= 1 && a.n_freq >= 1 && a.n_frames >= 1 && a.channels >= 1 && a.channels <= kBfMaxChannels &&
               a.ref >= 0 && a.ref < a.channels && (a.out != nullptr || a.w_out != nullptr || a.scm_t != nullptr || a.scm_n != nullptr),
           SPECINV_EINVAL, "beamform: bad arguments");
  const bool wide = a.channels > kBfNarrowChannels;
  if (is_double) return wide ? beamform_launch_k<double, 4>(a, stream) : beamform_launch_k<double, 1>(a, stream);
  return wide ? beamform_launch_k<float, 4>(a, stream) : beamform_launch_k<float, 1>(a, stream);
}

}  // namespace specinv
