// k_pyin_obs and k_pyin_viterbi (kernels_pyin.h) and their launches.
#include <cmath>

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

int pyin_obs_launch(const float* cmnd, const double* tables, float* obs, float* vprob, int64_t frames, int frame, int tau_min,
                    int tau_max, int n_thr, int n_ranks, int n_bins, int bins_per_semitone, double sample_rate, double fmin,
                    double no_trough, hipStream_t stream) {
  const int C = frame / 128;
  SI_CHECK(cmnd != nullptr && tables != nullptr && obs != nullptr && vprob != nullptr && frames >= 1 && frame == 128 * C &&
               (C == 2 || C == 4 || C == 8 || C == 16) && tau_min >= 1 && tau_min < tau_max && tau_max <= frame / 2 - 1 &&
               n_thr >= 1 && n_thr <= kPyinMaxThresholds && n_ranks >= (tau_max - tau_min) / 2 + 1 && n_bins >= 1 &&
               n_bins <= kPyinMaxBins && bins_per_semitone >= 1,
           SPECINV_EINVAL, "pyin_obs: bad arguments");
  static_assert(pyin_obs_lds_bytes(1024, kPyinMaxBins) <= 64 * 1024, "the rows must fit the LDS a launch gets without asking");
  PyinObsArgs a;
  a.cmnd = cmnd;
  a.thr = tables;
  a.wk = a.thr + n_thr;
  a.cum = a.wk + n_thr;
  a.boltz = a.cum + n_thr + 1;
  a.inv = a.boltz + n_ranks;
  a.obs = obs;
  a.vprob = vprob;
  a.frames = frames;
  a.n_thr = n_thr;
  a.tau_min = tau_min;
  a.tau_max = tau_max;
  a.n_bins = n_bins;
  a.sample_rate = sample_rate;
  a.fmin = fmin;
  a.scale = 12.0 * (double)bins_per_semitone;
  a.no_trough = no_trough;
  switch (C) {
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

int pyin_viterbi_launch(const float* obs, const float* vprob, const double* tables, int16_t* backptr, int32_t* states, int64_t* ticks,
                        int64_t batch, int64_t n_frames, int n_bins, int half, double switch_prob, hipStream_t stream) {
  SI_CHECK(obs != nullptr && vprob != nullptr && tables != nullptr && backptr != nullptr && states != nullptr && batch >= 1 &&
               n_frames >= 1 && n_bins >= 1 && n_bins <= kPyinMaxBins && half >= 0 && half <= kPyinMaxHalf && switch_prob > 0 &&
               switch_prob < 1,
           SPECINV_EINVAL, "pyin_viterbi: bad arguments");
  PyinVitArgs a;
  a.obs = obs;
  a.vprob = vprob;
  a.ltri = tables;
  a.nlz = tables + half + 1;
  a.backptr = backptr;
  a.states = states;
  a.ticks = ticks;
  a.batch = batch;
  a.n_frames = n_frames;
  a.n_bins = n_bins;
  a.half = half;
  a.l_stay = std::log(1.0 - switch_prob + kPyinTiny);
  a.l_switch = std::log(switch_prob + kPyinTiny);
  a.l_tiny = std::log(kPyinTiny);
  const size_t lds = pyin_vit_lds_bytes(n_bins, half);
  static_assert(pyin_vit_lds_bytes(kPyinMaxBins, kPyinMaxHalf) <= 160 * 1024, "the state must fit a CU's LDS");
  const void* fn = ticks != nullptr ? (const void*)k_pyin_viterbi<true> : (const void*)k_pyin_viterbi<false>;
  SI_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)pyin_vit_lds_bytes(kPyinMaxBins, kPyinMaxHalf)));
  const unsigned threads = 64u * (unsigned)ceil_div(n_bins, 64);
  const unsigned grid = (unsigned)(batch < 65536 ? batch : 65536);
  if (ticks != nullptr)
    hipLaunchKernelGGL((k_pyin_viterbi<true>), dim3(grid), dim3(threads), lds, stream, a);
  else
    hipLaunchKernelGGL((k_pyin_viterbi<false>), dim3(grid), dim3(threads), lds, stream, a);
  SI_HIP(hipGetLastError());
  return SPECINV_OK;
}

}  // namespace specinv
