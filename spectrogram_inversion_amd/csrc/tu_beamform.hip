// specinv_beamform: the entry point, and the launch of k_beamform (kernels_beamform.h).
#include "entry.h"
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

}  // namespace specinv

using namespace specinv;

extern "C" int specinv_beamform(const void* spec, const void* mask_target, const void* mask_noise, const void* weights_in, void* out,
                                void* weights_out, void* scm_target, void* scm_noise, int64_t batch, int32_t channels, int64_t n_freq,
                                int64_t n_frames, int32_t solution, int32_t ref_channel, int32_t n_power_iter, double diag_load,
                                double mu, int32_t dtype, int32_t device, void* hip_stream) {
  // (the argument errors before the device is touched, in the header's order)
  SI_CHECK(spec, SPECINV_EINVAL, "specinv_beamform: NULL spec");
  SI_CHECK(weights_in == nullptr || (mask_target == nullptr && mask_noise == nullptr && weights_out == nullptr && scm_target == nullptr &&
                                     scm_noise == nullptr && out != nullptr),
           SPECINV_EINVAL,
           "specinv_beamform: with weights_in given nothing is estimated: out is needed, the masks, weights_out and the covariances "
           "must be NULL");
  SI_CHECK(weights_in != nullptr || out != nullptr || weights_out != nullptr || scm_target != nullptr || scm_noise != nullptr, SPECINV_EINVAL,
           "specinv_beamform: no result is asked for");
  SI_CHECK(weights_in != nullptr || mask_target != nullptr || (out == nullptr && weights_out == nullptr), SPECINV_EINVAL,
           "specinv_beamform: weights need mask_target");
  {
    const void* p[8] = {spec, mask_target, mask_noise, weights_in, out, weights_out, scm_target, scm_noise};
    static const char* const names[8] = {"spec", "mask_target", "mask_noise", "weights_in", "out", "weights_out", "scm_target", "scm_noise"};
    SI_TRY(no_alias("specinv_beamform", p, names, 8, 4));
  }
  SI_CHECK(batch >= 1 && channels >= 1 && n_freq >= 1 && n_frames >= 1, SPECINV_EINVAL,
           "specinv_beamform: batch, channels, n_freq and n_frames must be >= 1, got %lld, %d, %lld and %lld", (long long)batch, channels,
           (long long)n_freq, (long long)n_frames);
  SI_CHECK(batch <= (INT64_MAX >> 12) / n_freq / n_frames, SPECINV_EINVAL,
           "specinv_beamform: %lld x %lld x %lld elements a channel are too many", (long long)batch, (long long)n_freq, (long long)n_frames);
  SI_CHECK(solution == SPECINV_BEAMFORM_SOUDEN || solution == SPECINV_BEAMFORM_RTF_POWER || solution == SPECINV_BEAMFORM_MWF, SPECINV_EINVAL,
           "specinv_beamform: unknown solution %d", solution);
  SI_CHECK(ref_channel >= 0 && ref_channel < channels, SPECINV_EINVAL, "specinv_beamform: ref_channel must be in [0, %d), got %d", channels,
           ref_channel);
  SI_CHECK(n_power_iter >= 1, SPECINV_EINVAL, "specinv_beamform: n_power_iter must be >= 1, got %d", n_power_iter);
  SI_CHECK(diag_load >= 0 && std::isfinite(diag_load) && mu >= 0 && std::isfinite(mu), SPECINV_EINVAL,
           "specinv_beamform: diag_load and mu must be finite and >= 0, got %g and %g", diag_load, mu);
  SI_CHECK_DTYPE(dtype);
  SI_CHECK(channels <= kBfMaxChannels, SPECINV_EUNSUPPORTED, "specinv_beamform: channels must be <= %d, got %d", kBfMaxChannels, channels);
  SI_CHECK(n_power_iter <= kBfMaxPowerIter, SPECINV_EUNSUPPORTED, "specinv_beamform: n_power_iter must be <= %d, got %d", kBfMaxPowerIter,
           n_power_iter);
  SI_ENTER_DEVICE(device, hip_stream);
  BfArgs a;
  a.spec = spec;
  a.mask_t = (const double*)mask_target;
  a.mask_n = (const double*)mask_noise;
  a.w_in = weights_in;
  a.out = out;
  a.w_out = weights_out;
  a.scm_t = scm_target;
  a.scm_n = scm_noise;
  a.batch = batch;
  a.n_freq = n_freq;
  a.n_frames = n_frames;
  a.channels = channels;
  a.solution = solution;
  a.ref = ref_channel;
  a.n_power_iter = n_power_iter;
  a.diag_load = diag_load;
  a.mu = mu;
  const bool wide = channels > kBfNarrowChannels;
  if (dtype == SPECINV_F64) return wide ? beamform_launch_k<double, 4>(a, stream) : beamform_launch_k<double, 1>(a, stream);
  return wide ? beamform_launch_k<float, 4>(a, stream) : beamform_launch_k<float, 1>(a, stream);
}
