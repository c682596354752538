// specinv_wpe: the entry point, and the launch of k_wpe (kernels_wpe.h).
#include "entry.h"
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

}  // namespace specinv

using namespace specinv;

extern "C" int specinv_wpe(const void* spec, const void* power, const void* filt_in, void* out, void* filt_out, void* lam, void* scratch,
                           int64_t batch, int32_t channels, int64_t n_freq, int64_t n_frames, int32_t taps, int64_t delay,
                           int32_t n_iter, int64_t psd_context, double eps, double diag_load, int32_t dtype, int32_t device,
                           void* hip_stream) {
  // (the argument errors before the device is touched, in the header's order)
  SI_CHECK(spec && out, SPECINV_EINVAL, "specinv_wpe: NULL spec or out");
  SI_CHECK(filt_in == nullptr || (power == nullptr && filt_out == nullptr && lam == nullptr), SPECINV_EINVAL,
           "specinv_wpe: with filt_in given nothing is estimated: power, filt_out and lam must be NULL");
  SI_CHECK(filt_in != nullptr || lam != nullptr, SPECINV_EINVAL, "specinv_wpe: lam is NULL (it is the estimate's work array as well)");
  SI_CHECK(filt_in != nullptr || psd_context <= 0 || scratch != nullptr, SPECINV_EINVAL,
           "specinv_wpe: psd_context > 0 needs the scratch array");
  {
    const void* p[7] = {spec, power, filt_in, out, filt_out, lam, scratch};
    static const char* const names[7] = {"spec", "power", "filt_in", "out", "filt_out", "lam", "scratch"};
    SI_TRY(no_alias("specinv_wpe", p, names, 7, 3));
  }
  SI_CHECK(batch >= 1 && channels >= 1 && n_freq >= 1 && n_frames >= 1, SPECINV_EINVAL,
           "specinv_wpe: batch, channels, n_freq and n_frames must be >= 1, got %lld, %d, %lld and %lld", (long long)batch, channels,
           (long long)n_freq, (long long)n_frames);
  SI_CHECK(batch <= (INT64_MAX >> 12) / n_freq / n_frames, SPECINV_EINVAL, "specinv_wpe: %lld x %lld x %lld elements a channel are too many",
           (long long)batch, (long long)n_freq, (long long)n_frames);
  SI_CHECK(taps >= 1, SPECINV_EINVAL, "specinv_wpe: taps must be >= 1, got %d", taps);
  SI_CHECK(delay >= 1, SPECINV_EINVAL, "specinv_wpe: delay must be >= 1 (at 0 the filter predicts a frame from itself), got %lld",
           (long long)delay);
  SI_CHECK(n_iter >= 0 && psd_context >= 0, SPECINV_EINVAL, "specinv_wpe: n_iter and psd_context must be >= 0, got %d and %lld", n_iter,
           (long long)psd_context);
  SI_CHECK(eps >= 0 && std::isfinite(eps) && diag_load >= 0 && std::isfinite(diag_load), SPECINV_EINVAL,
           "specinv_wpe: eps and diag_load must be finite and >= 0, got %g and %g", eps, diag_load);
  SI_CHECK_DTYPE(dtype);
  SI_CHECK(channels <= kWpeMaxD && taps <= kWpeMaxD && channels * taps <= kWpeMaxD, SPECINV_EUNSUPPORTED,
           "specinv_wpe: channels x taps must be <= %d, got %d x %d", kWpeMaxD, channels, taps);
  SI_CHECK(n_iter <= kWpeMaxIter && psd_context <= kWpeMaxContext, SPECINV_EUNSUPPORTED,
           "specinv_wpe: n_iter must be <= %d and psd_context <= %d, got %d and %lld", kWpeMaxIter, kWpeMaxContext, n_iter,
           (long long)psd_context);
  SI_ENTER_DEVICE(device, hip_stream);
  WpeArgs a;
  a.spec = spec;
  a.power = (const double*)power;
  a.filt_in = filt_in;
  a.out = out;
  a.filt_out = filt_out;
  a.lam = (double*)lam;
  a.qbuf = (double*)scratch;
  a.batch = batch;
  a.n_freq = n_freq;
  a.n_frames = n_frames;
  a.delay = delay;
  a.ctx = psd_context < n_frames ? psd_context : n_frames;     // (a wider context holds the same frames)
  a.channels = channels;
  a.taps = taps;
  a.n_iter = n_iter;
  a.eps = eps;
  a.diag_load = diag_load;
  const WpeGeom g = wpe_geom(channels, taps);
  SI_CHECK(sizeof(double) * (size_t)g.total <= 160 * 1024, SPECINV_EUNSUPPORTED, "wpe: %d channels x %d taps need %zu bytes of LDS",
           channels, taps, sizeof(double) * (size_t)g.total);
  const bool two = g.nblocks > kWpeThreads;          // (only without slices: a thread then owns two blocks)
  if (dtype == SPECINV_F64) return two ? wpe_launch_k<double, 2>(a, g, stream) : wpe_launch_k<double, 1>(a, g, stream);
  return two ? wpe_launch_k<float, 2>(a, g, stream) : wpe_launch_k<float, 1>(a, g, stream);
}
