// specinv_spectral_envelope: the entry point, and the launch of k_spectral_envelope (kernels_envelope.h).
#include "entry.h"
#include "kernels_envelope.h"

namespace specinv {

// Items and tiles are one flattened grid, in as many launches as 2^22 workgroups each take.
template <int R, bool CPLX>
static int envelope_launch_r(const EnvArgs& a, int64_t blocks, hipStream_t stream) {
  using E = EnvGeo<R>;
  const void* fn = (const void*)k_spectral_envelope<R, CPLX>;
  const size_t lds = E::lds_bytes();
  static_assert(E::lds_bytes() <= 160 * 1024, "the tile and the tables must fit a CU's LDS");
  SI_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int64_t per_launch = (int64_t)1 << 22;
  for (int64_t b0 = 0; b0 < blocks; b0 += per_launch) {
    const int64_t nb = blocks - b0 < per_launch ? blocks - b0 : per_launch;
    hipLaunchKernelGGL((k_spectral_envelope<R, CPLX>), dim3((unsigned)nb), dim3(kEnvThreads), lds, stream, a, b0);
    SI_HIP(hipGetLastError());
  }
  return SPECINV_OK;
}

}  // namespace specinv

using namespace specinv;

extern "C" int specinv_spectral_envelope(const void* spec, void* out, const void* amin, int64_t batch, int32_t n_freq, int32_t n_frames,
                                         int32_t order, int32_t n_iter, int32_t out_log, int32_t is_complex, int32_t frame_major,
                                         int32_t dtype, int32_t device, void* hip_stream) {
  // (the argument errors before the device is touched, in the header's order)
  SI_CHECK(spec && out && amin, SPECINV_EINVAL, "specinv_spectral_envelope: NULL %s", !spec ? "spec" : !out ? "out" : "amin");
  SI_CHECK(out != spec, SPECINV_EINVAL, "specinv_spectral_envelope: out must not alias spec");
  SI_CHECK(batch >= 1 && n_frames >= 1, SPECINV_EINVAL, "specinv_spectral_envelope: batch and n_frames must be >= 1, got %lld and %d",
           (long long)batch, n_frames);
  SI_CHECK(n_iter >= 0 && n_iter <= kEnvMaxIter, SPECINV_EINVAL, "specinv_spectral_envelope: n_iter must be in 0 ... %d, got %d",
           kEnvMaxIter, n_iter);
  SI_CHECK_DTYPE(dtype);
  SI_CHECK(dtype == SPECINV_F32, SPECINV_EUNSUPPORTED, "specinv_spectral_envelope: float32 only");
  SI_CHECK(n_freq == 129 || n_freq == 257 || n_freq == 513 || n_freq == 1025, SPECINV_EUNSUPPORTED,
           "specinv_spectral_envelope: n_freq must be 129, 257, 513 or 1025 (n_fft 256, 512, 1024 or 2048), got %d", n_freq);
  SI_CHECK(order >= 0 && order <= n_freq - 1, SPECINV_EINVAL, "specinv_spectral_envelope: order must be in 0 ... %d, got %d",
           n_freq - 1, order);
  SI_ENTER_DEVICE(device, hip_stream);
  const int R = (n_freq - 1) / 32;           // n_fft / 64
  EnvArgs a;
  a.spec = (const float*)spec;
  a.out = (float*)out;
  a.amin = (const float*)amin;
  a.n_frames = n_frames;
  a.order = order;
  a.n_iter = n_iter;
  a.out_log = out_log ? 1 : 0;
  a.frame_major = frame_major ? 1 : 0;
  const int tt = R <= 8 ? EnvGeo<4>::TT : R == 16 ? EnvGeo<16>::TT : EnvGeo<32>::TT;
  a.tiles_t = ceil_div(n_frames, tt);
  const __int128 blocks = (__int128)batch * a.tiles_t;
  SI_CHECK(blocks < ((__int128)1 << 62), SPECINV_EINVAL, "spectral_envelope: %lld items of %d frames exceed the launch grid",
           (long long)batch, n_frames);
#define SPECINV_ENV_CASE(RR)                                                                  \
  case RR:                                                                                    \
    return is_complex ? envelope_launch_r<RR, true>(a, (int64_t)blocks, stream) : envelope_launch_r<RR, false>(a, (int64_t)blocks, stream)
  switch (R) {
    SPECINV_ENV_CASE(4);
    SPECINV_ENV_CASE(8);
    SPECINV_ENV_CASE(16);
    default:
      SPECINV_ENV_CASE(32);
  }
#undef SPECINV_ENV_CASE
}
