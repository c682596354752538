// k_wpe (kernels_wpe.h) and its launch.
#include "kernels_wpe.h"

namespace specinv {

template <typename T, int NB>
static int wpe_launch_k(const WpeArgs& a, const WpeGeom& g, hipStream_t stream) {
  const size_t lds = sizeof(double) * (size_t)g.total;
  const int64_t probs = a.batch * a.n_freq;
  const unsigned grid = (unsigned)(probs < kWpeMaxGrid ? probs : kWpeMaxGrid);
  if (lds > 64 * 1024)
    SI_HIP(hipFuncSetAttribute((const void*)k_wpe<T, NB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((k_wpe<T, NB>), dim3(grid), dim3(kWpeThreads), lds, stream, a);
  SI_HIP(hipGetLastError());
  return SPECINV_OK;
}

int wpe_launch(const WpeArgs& a, bool is_double, hipStream_t stream) {
  SI_CHECK(a.spec != nullptr && a.out != nullptr && a.batch >= 1 && a.n_freq >= 1 && a.n_frames >= 1 && a.channels >= 1 && a.taps >= 1 &&
               a.channels * a.taps <= kWpeMaxD && a.delay >= 1 && a.ctx >= 0 && a.n_iter >= 0 &&
               (a.filt_in != nullptr || (a.lam != nullptr && (a.ctx == 0 || a.qbuf != nullptr))),
           SPECINV_EINVAL, "wpe: bad arguments");
  const WpeGeom g = wpe_geom(a.channels, a.taps);
  SI_CHECK(sizeof(double) * (size_t)g.total <= 160 * 1024, SPECINV_EUNSUPPORTED, "wpe: %d channels x %d taps need %zu bytes of LDS",
           a.channels, a.taps, sizeof(double) * (size_t)g.total);
  const bool two = g.nblocks > kWpeThreads;          // (only without slices: a thread then owns two blocks)
  if (is_double) return two ? wpe_launch_k<double, 2>(a, g, stream) : wpe_launch_k<double, 1>(a, g, stream);
  return two ? wpe_launch_k<float, 2>(a, g, stream) : wpe_launch_k<float, 1>(a, g, stream);
}

}  // namespace specinv
