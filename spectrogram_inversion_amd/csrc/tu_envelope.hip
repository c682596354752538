// k_spectral_envelope (kernels_envelope.h) and its launch.
#include "kernels_envelope.h"

namespace specinv {

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

int envelope_launch(const float* spec, float* out, const float* amin, int64_t batch, int n_freq, int n_frames, int order, int n_iter,
                    bool out_log, bool is_complex, bool frame_major, hipStream_t stream) {
  const int n_fft = 2 * (n_freq - 1), R = n_fft / 64;
  SI_CHECK(spec != nullptr && out != nullptr && amin != nullptr && batch >= 1 && n_frames >= 1 && n_freq == 32 * R + 1 &&
               (R == 4 || R == 8 || R == 16 || R == 32) && order >= 0 && order <= n_fft / 2 && n_iter >= 0 && n_iter <= kEnvMaxIter,
           SPECINV_EINVAL, "spectral_envelope: bad arguments");
  EnvArgs a;
  a.spec = spec;
  a.out = out;
  a.amin = amin;
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

}  // namespace specinv
