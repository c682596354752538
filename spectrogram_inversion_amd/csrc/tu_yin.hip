// specinv_yin: the entry point, and the launch of k_yin (kernels_yin.h).
#include "entry.h"
#include "kernels_yin.h"

namespace specinv {

// Items and their groups of four frames are one flattened grid, in as many launches as 2^22 workgroups each take.
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

}  // namespace specinv

using namespace specinv;

extern "C" int specinv_yin(const void* x, void* period_out, void* aper_out, void* tau_out, void* cmnd_out, int64_t batch, int64_t length,
                           int32_t frame, int32_t hop, int32_t center, int32_t tau_min, int32_t tau_max, double threshold,
                           int32_t dtype, int32_t device, void* hip_stream) {
  // (the argument errors before the device is touched, in the header's order)
  SI_CHECK(x && period_out && aper_out, SPECINV_EINVAL, "specinv_yin: NULL %s", !x ? "x" : !period_out ? "period_out" : "aper_out");
  {
    const void* p[5] = {x, period_out, aper_out, tau_out, cmnd_out};
    static const char* const names[5] = {"x", "period_out", "aper_out", "tau_out", "cmnd_out"};
    SI_TRY(no_alias("specinv_yin", p, names, 5, 1));
  }
  SI_CHECK(batch >= 1, SPECINV_EINVAL, "specinv_yin: batch must be >= 1, got %lld", (long long)batch);
  SI_CHECK_DTYPE(dtype);
  SI_CHECK(dtype == SPECINV_F32, SPECINV_EUNSUPPORTED, "specinv_yin: float32 only");
  SI_CHECK(frame == 256 || frame == 512 || frame == 1024 || frame == 2048, SPECINV_EUNSUPPORTED,
           "specinv_yin: frame must be 256, 512, 1024 or 2048, got %d", frame);
  SI_CHECK(hop >= 1 && hop <= frame, SPECINV_EINVAL, "specinv_yin: hop must be in 1 ... %d, got %d", frame, hop);
  SI_CHECK(length >= (center ? 1 : frame), SPECINV_EINVAL, "specinv_yin: a length of %lld gives no frame (center %d, frame %d)",
           (long long)length, center, frame);
  SI_CHECK(tau_min >= 1 && tau_max <= frame / 2 - 1 && tau_min < tau_max, SPECINV_EINVAL,
           "specinv_yin: tau_min, tau_max must satisfy 1 <= tau_min < tau_max <= %d, got %d, %d", frame / 2 - 1, tau_min, tau_max);
  SI_CHECK(std::isfinite(threshold) && threshold > 0, SPECINV_EINVAL, "specinv_yin: threshold must be finite and > 0, got %g", threshold);
  SI_ENTER_DEVICE(device, hip_stream);
  YinArgs a;
  a.x = (const float*)x;
  a.period = (float*)period_out;
  a.aper = (float*)aper_out;
  a.tau = (int32_t*)tau_out;
  a.cmnd = (float*)cmnd_out;
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
  switch (frame / 64) {
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
