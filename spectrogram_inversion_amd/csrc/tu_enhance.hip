// specinv_enhance: the entry point, and the launch of k_enhance (kernels_enhance.h).
#include "entry.h"
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

static_assert(kEnhWiener == SPECINV_ENHANCE_WIENER && kEnhLsa == SPECINV_ENHANCE_LSA && kEnhNoiseTracked == SPECINV_ENHANCE_TRACK &&
                  kEnhNoiseFull == SPECINV_ENHANCE_NOISE_FULL && kEnhNoiseProfile == SPECINV_ENHANCE_NOISE_PROFILE,
              "the kernel reads the header's codes");

}  // namespace specinv

using namespace specinv;

extern "C" int specinv_enhance(const void* spec, const void* noise, const void* state_in, void* noise_out, void* spp_out, void* gain_out,
                               void* snr_out, void* enhanced_out, void* state_out, int64_t batch, int64_t n_freq, int64_t n_frames,
                               int32_t init_frames, int32_t noise_mode, int32_t rule, double alpha_pow, double alpha_spp,
                               double prior_snr, double alpha, double xi_min, double gain_min, int32_t is_complex, int32_t frame_major,
                               int32_t dtype, int32_t device, void* hip_stream) {
  // (the argument errors before the device is touched, in the header's order)
  SI_CHECK(spec, SPECINV_EINVAL, "specinv_enhance: NULL spec");
  SI_CHECK(noise_out || spp_out || gain_out || snr_out || enhanced_out || state_out, SPECINV_EINVAL,
           "specinv_enhance: every output is NULL");
  SI_CHECK(noise_mode == SPECINV_ENHANCE_TRACK || noise_mode == SPECINV_ENHANCE_NOISE_FULL || noise_mode == SPECINV_ENHANCE_NOISE_PROFILE,
           SPECINV_EINVAL, "specinv_enhance: noise_mode must be SPECINV_ENHANCE_TRACK, _NOISE_FULL or _NOISE_PROFILE, got %d", noise_mode);
  SI_CHECK((noise_mode == SPECINV_ENHANCE_TRACK) == (noise == nullptr), SPECINV_EINVAL,
           "specinv_enhance: noise must be NULL with SPECINV_ENHANCE_TRACK and given otherwise");
  SI_CHECK(noise == nullptr || (noise_out == nullptr && spp_out == nullptr), SPECINV_EINVAL,
           "specinv_enhance: with noise given the tracker does not run: noise_out and spp_out must be NULL");
  {
    const void* p[9] = {spec, noise, state_in, noise_out, spp_out, gain_out, snr_out, enhanced_out, state_out};
    static const char* const names[9] = {"spec",     "noise",   "state_in",     "noise_out", "spp_out",
                                         "gain_out", "snr_out", "enhanced_out", "state_out"};
    SI_TRY(no_alias("specinv_enhance", p, names, 9, 1));
  }
  SI_CHECK(batch >= 1 && n_freq >= 1 && n_frames >= 1, SPECINV_EINVAL,
           "specinv_enhance: batch, n_freq and n_frames must be >= 1, got %lld, %lld and %lld", (long long)batch, (long long)n_freq,
           (long long)n_frames);
  SI_CHECK(batch <= (INT64_MAX >> 5) / n_freq / n_frames, SPECINV_EINVAL, "specinv_enhance: %lld x %lld x %lld elements are too many",
           (long long)batch, (long long)n_freq, (long long)n_frames);
  SI_CHECK(init_frames >= 1, SPECINV_EINVAL, "specinv_enhance: init_frames must be >= 1, got %d", init_frames);
  SI_CHECK_DTYPE(dtype);
  SI_CHECK(rule == SPECINV_ENHANCE_WIENER || rule == SPECINV_ENHANCE_LSA, SPECINV_EINVAL,
           "specinv_enhance: rule must be SPECINV_ENHANCE_WIENER or SPECINV_ENHANCE_LSA, got %d", rule);
  SI_CHECK(alpha_pow >= 0 && alpha_pow <= 1 && alpha_spp >= 0 && alpha_spp <= 1 && alpha >= 0 && alpha <= 1, SPECINV_EINVAL,
           "specinv_enhance: alpha_pow, alpha_spp and alpha must be in 0 ... 1, got %g, %g and %g", alpha_pow, alpha_spp, alpha);
  SI_CHECK(std::isfinite(prior_snr) && prior_snr > 0 && std::isfinite(xi_min) && xi_min > 0, SPECINV_EINVAL,
           "specinv_enhance: prior_snr and xi_min must be finite and > 0, got %g and %g", prior_snr, xi_min);
  SI_CHECK(gain_min > 0 && gain_min <= 1, SPECINV_EINVAL, "specinv_enhance: gain_min must be in (0, 1], got %g", gain_min);
  SI_ENTER_DEVICE(device, hip_stream);
  EnhArgs a;
  a.spec = spec;
  a.noise_in = noise;
  a.state_in = (const double*)state_in;
  a.noise_out = noise_out;
  a.spp_out = spp_out;
  a.gain_out = gain_out;
  a.snr_out = snr_out;
  a.enh_out = enhanced_out;
  a.state_out = (double*)state_out;
  a.batch = batch;
  a.n_freq = n_freq;
  a.n_frames = n_frames;
  a.init_frames = init_frames;
  a.noise_mode = noise_mode;
  a.a_pow = alpha_pow;
  a.a_spp = alpha_spp;
  a.xi1p = 1.0 + prior_snr;
  a.c = prior_snr / (1.0 + prior_snr);
  a.alpha = alpha;
  a.xi_min = xi_min;
  a.g_min = gain_min;
  if (dtype == SPECINV_F64)
    return is_complex ? enhance_launch_l<double, true>(a, frame_major != 0, rule, stream)
                      : enhance_launch_l<double, false>(a, frame_major != 0, rule, stream);
  return is_complex ? enhance_launch_l<float, true>(a, frame_major != 0, rule, stream)
                    : enhance_launch_l<float, false>(a, frame_major != 0, rule, stream);
}
