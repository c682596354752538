// k_yin (kernels_yin.h) and its launch.
#include "kernels_yin.h"

namespace specinv {

template <int R>
static int yin_launch_r(const YinArgs& a, int64_t blocks, hipStream_t stream) {
  const void* fn = (const void*)k_yin<R>;
  const size_t lds = YinGeo<R>::lds_bytes();
  static_assert(YinGeo<R>::lds_bytes() <= 160 * 1024, "the tables must fit a CU's LDS");
  SI_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int64_t per_launch = (int64_t)1 << 22;
  for (int64_t b0 = 0; b0 < blocks; b0 += per_launch) {
    const int64_t nb = blocks - b0 < per_launch ? blocks - b0 : per_launch;
    hipLaunchKernelGGL((k_yin<R>), dim3((unsigned)nb), dim3(kYinThreads), lds, stream, a, b0);
    SI_HIP(hipGetLastError());
  }
  return SPECINV_OK;
}

int yin_launch(const float* x, float* period, float* aper, int32_t* tau, float* cmnd, int64_t batch, int64_t length, int frame,
               int hop, bool center, int tau_min, int tau_max, double threshold, hipStream_t stream) {
  const int R = frame / 64;
  SI_CHECK(x != nullptr && period != nullptr && aper != nullptr && batch >= 1 && frame == 64 * R &&
               (R == 4 || R == 8 || R == 16 || R == 32) && hop >= 1 && hop <= frame && length >= (center ? 1 : frame) &&
               tau_min >= 1 && tau_min < tau_max && tau_max <= frame / 2 - 1,
           SPECINV_EINVAL, "yin: bad arguments");
  YinArgs a;
  a.x = x;
  a.period = period;
  a.aper = aper;
  a.tau = tau;
  a.cmnd = cmnd;
  a.length = length;
  a.n_frames = center ? 1 + length / hop : 1 + (length - frame) / hop;
  a.hop = hop;
  a.center = center ? 1 : 0;
  a.tau_min = tau_min;
  a.tau_max = tau_max;
  a.threshold = threshold;
  a.groups_t = ceil_div(a.n_frames, kYinWaves);
  const __int128 blocks = (__int128)batch * a.groups_t;
  SI_CHECK(blocks < ((__int128)1 << 62), SPECINV_EINVAL, "yin: %lld items of %lld frames exceed the launch grid", (long long)batch,
           (long long)a.n_frames);
  switch (R) {
    case 4:
      return yin_launch_r<4>(a, (int64_t)blocks, stream);
    case 8:
      return yin_launch_r<8>(a, (int64_t)blocks, stream);
    case 16:
      return yin_launch_r<16>(a, (int64_t)blocks, stream);
    default:
      return yin_launch_r<32>(a, (int64_t)blocks, stream);
  }
}

}  // namespace specinv
