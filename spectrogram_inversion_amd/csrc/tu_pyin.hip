// specinv_pyin_obs, specinv_pyin_viterbi: the entry points, and the launches of k_pyin_obs and k_pyin_viterbi (kernels_pyin.h).
#include <cmath>

#include "entry.h"
#include "kernels_pyin.h"

namespace specinv {

template <int C>
static int pyin_obs_launch_c(const PyinObsArgs& a, hipStream_t stream) {
  const size_t lds = pyin_obs_lds_bytes(64 * C, a.n_bins);
  const int64_t blocks = ceil_div(a.frames, kPyinWaves);
  const int64_t per_launch = (int64_t)1 << 22;
  for (int64_t b0 = 0; b0 < blocks; b0 += per_launch) {
    const int64_t nb = blocks - b0 < per_launch ? blocks - b0 : per_launch;
    hipLaunchKernelGGL((k_pyin_obs<C>), dim3((unsigned)nb), dim3(kPyinThreads), lds, stream, a, b0);
    SI_HIP(hipGetLastError());
  }
  return SPECINV_OK;
}

}  // namespace specinv

using namespace specinv;

extern "C" {

int specinv_pyin_obs(const void* cmnd, const void* tables, void* obs_out, void* vprob_out, int64_t frames, int32_t frame,
                     int32_t tau_min, int32_t tau_max, int32_t n_thresholds, int32_t n_ranks, int32_t n_bins, int32_t bins_per_semitone,
                     double sample_rate, double fmin, double no_trough_prob, int32_t dtype, int32_t device, void* hip_stream) {
  // (the argument errors before the device is touched, in the header's order)
  SI_CHECK(cmnd && tables && obs_out && vprob_out, SPECINV_EINVAL, "specinv_pyin_obs: NULL %s",
           !cmnd ? "cmnd" : !tables ? "tables" : !obs_out ? "obs_out" : "vprob_out");
  SI_CHECK(obs_out != cmnd && vprob_out != cmnd && obs_out != tables && vprob_out != tables && obs_out != vprob_out, SPECINV_EINVAL,
           "specinv_pyin_obs: an output must not alias an input or the other output");
  SI_CHECK(frames >= 1, SPECINV_EINVAL, "specinv_pyin_obs: frames must be >= 1, got %lld", (long long)frames);
  SI_CHECK_DTYPE(dtype);
  SI_CHECK(dtype == SPECINV_F32, SPECINV_EUNSUPPORTED, "specinv_pyin_obs: float32 only");
  SI_CHECK(frame == 256 || frame == 512 || frame == 1024 || frame == 2048, SPECINV_EUNSUPPORTED,
           "specinv_pyin_obs: frame must be 256, 512, 1024 or 2048, got %d", frame);
  SI_CHECK(n_bins >= 1 && n_bins <= kPyinMaxBins, SPECINV_EUNSUPPORTED, "specinv_pyin_obs: n_bins must be in 1 ... %d, got %d",
           kPyinMaxBins, n_bins);
  SI_CHECK(n_thresholds >= 1 && n_thresholds <= kPyinMaxThresholds, SPECINV_EUNSUPPORTED,
           "specinv_pyin_obs: n_thresholds must be in 1 ... %d, got %d", kPyinMaxThresholds, n_thresholds);
  SI_CHECK(tau_min >= 1 && tau_max <= frame / 2 - 1 && tau_min < tau_max, SPECINV_EINVAL,
           "specinv_pyin_obs: tau_min, tau_max must satisfy 1 <= tau_min < tau_max <= %d, got %d, %d", frame / 2 - 1, tau_min, tau_max);
  SI_CHECK(n_ranks >= (tau_max - tau_min) / 2 + 1, SPECINV_EINVAL,
           "specinv_pyin_obs: n_ranks must cover the %d troughs the range can hold, got %d", (tau_max - tau_min) / 2 + 1, n_ranks);
  SI_CHECK(bins_per_semitone >= 1, SPECINV_EINVAL, "specinv_pyin_obs: bins_per_semitone must be >= 1, got %d", bins_per_semitone);
  SI_CHECK(std::isfinite(sample_rate) && sample_rate > 0 && std::isfinite(fmin) && fmin > 0, SPECINV_EINVAL,
           "specinv_pyin_obs: sample_rate and fmin must be finite and > 0, got %g and %g", sample_rate, fmin);
  SI_CHECK(no_trough_prob >= 0 && no_trough_prob <= 1, SPECINV_EINVAL, "specinv_pyin_obs: no_trough_prob must be in 0 ... 1, got %g",
           no_trough_prob);
  SI_ENTER_DEVICE(device, hip_stream);
  static_assert(pyin_obs_lds_bytes(1024, kPyinMaxBins) <= 64 * 1024, "the rows must fit the LDS a launch gets without asking");
  PyinObsArgs a;
  a.cmnd = (const float*)cmnd;
  a.thr = (const double*)tables;
  a.wk = a.thr + n_thresholds;
  a.cum = a.wk + n_thresholds;
  a.boltz = a.cum + n_thresholds + 1;
  a.inv = a.boltz + n_ranks;
  a.obs = (float*)obs_out;
  a.vprob = (float*)vprob_out;
  a.frames = frames;
  a.n_thr = n_thresholds;
  a.tau_min = tau_min;
  a.tau_max = tau_max;
  a.n_bins = n_bins;
  a.sample_rate = sample_rate;
  a.fmin = fmin;
  a.scale = 12.0 * (double)bins_per_semitone;
  a.no_trough = no_trough_prob;
  switch (frame / 128) {
    case 2:
      return pyin_obs_launch_c<2>(a, stream);
    case 4:
      return pyin_obs_launch_c<4>(a, stream);
    case 8:
      return pyin_obs_launch_c<8>(a, stream);
    default:
      return pyin_obs_launch_c<16>(a, stream);
  }
}

int specinv_pyin_viterbi(const void* obs, const void* vprob, const void* tables, void* backptr, void* states_out, void* ticks_out,
                         int64_t batch, int64_t n_frames, int32_t n_bins, int32_t half_width, double switch_prob, int32_t dtype,
                         int32_t device, void* hip_stream) {
  // (the argument errors before the device is touched, in the header's order)
  SI_CHECK(obs && vprob && tables && backptr && states_out, SPECINV_EINVAL, "specinv_pyin_viterbi: NULL %s",
           !obs ? "obs" : !vprob ? "vprob" : !tables ? "tables" : !backptr ? "backptr" : "states_out");
  {
    const void* p[6] = {obs, vprob, tables, backptr, states_out, ticks_out};
    static const char* const names[6] = {"obs", "vprob", "tables", "backptr", "states_out", "ticks_out"};
    SI_TRY(no_alias("specinv_pyin_viterbi", p, names, 6, 3));
  }
  SI_CHECK(batch >= 1 && n_frames >= 1, SPECINV_EINVAL, "specinv_pyin_viterbi: batch and n_frames must be >= 1, got %lld and %lld",
           (long long)batch, (long long)n_frames);
  SI_CHECK_DTYPE(dtype);
  SI_CHECK(dtype == SPECINV_F32, SPECINV_EUNSUPPORTED, "specinv_pyin_viterbi: float32 observations only");
  SI_CHECK(n_bins >= 1 && n_bins <= kPyinMaxBins, SPECINV_EUNSUPPORTED, "specinv_pyin_viterbi: n_bins must be in 1 ... %d, got %d",
           kPyinMaxBins, n_bins);
  SI_CHECK(half_width >= 0 && half_width <= kPyinMaxHalf, SPECINV_EUNSUPPORTED,
           "specinv_pyin_viterbi: half_width must be in 0 ... %d (a band of at most %d bins), got %d", kPyinMaxHalf,
           2 * kPyinMaxHalf + 1, half_width);
  SI_CHECK(switch_prob > 0 && switch_prob < 1, SPECINV_EINVAL, "specinv_pyin_viterbi: switch_prob must be in (0, 1), got %g",
           switch_prob);
  SI_ENTER_DEVICE(device, hip_stream);
  PyinVitArgs a;
  a.obs = (const float*)obs;
  a.vprob = (const float*)vprob;
  a.ltri = (const double*)tables;
  a.nlz = a.ltri + half_width + 1;
  a.backptr = (int16_t*)backptr;
  a.states = (int32_t*)states_out;
  a.ticks = (int64_t*)ticks_out;
  a.batch = batch;
  a.n_frames = n_frames;
  a.n_bins = n_bins;
  a.half = half_width;
  a.l_stay = std::log(1.0 - switch_prob + kPyinTiny);
  a.l_switch = std::log(switch_prob + kPyinTiny);
  a.l_tiny = std::log(kPyinTiny);
  const size_t lds = pyin_vit_lds_bytes(n_bins, half_width);
  static_assert(pyin_vit_lds_bytes(kPyinMaxBins, kPyinMaxHalf) <= 160 * 1024, "the state must fit a CU's LDS");
  const void* fn = ticks_out != nullptr ? (const void*)k_pyin_viterbi<true> : (const void*)k_pyin_viterbi<false>;
  SI_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)pyin_vit_lds_bytes(kPyinMaxBins, kPyinMaxHalf)));
  const unsigned threads = 64u * (unsigned)ceil_div(n_bins, 64);
  const unsigned grid = (unsigned)(batch < 65536 ? batch : 65536);
  if (ticks_out != nullptr)
    hipLaunchKernelGGL((k_pyin_viterbi<true>), dim3(grid), dim3(threads), lds, stream, a);
  else
    hipLaunchKernelGGL((k_pyin_viterbi<false>), dim3(grid), dim3(threads), lds, stream, a);
  SI_HIP(hipGetLastError());
  return SPECINV_OK;
}

}  // extern "C"
