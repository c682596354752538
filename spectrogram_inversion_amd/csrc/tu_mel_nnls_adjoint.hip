// k_mel_nnls_adjoint (kernels_mel_nnls_adjoint.h) and its launch, on the plan state of specinv_mel_nnls_setup.
#include "kernels_mel_nnls_adjoint.h"
#include "mel_nnls_state.h"

namespace specinv {

namespace fast {
template __global__ void k_mel_nnls_adjoint<float, false>(MelNnlsAdjointArgs<float>);
template __global__ void k_mel_nnls_adjoint<float, true>(MelNnlsAdjointArgs<float>);
template __global__ void k_mel_nnls_adjoint<double, false>(MelNnlsAdjointArgs<double>);
template __global__ void k_mel_nnls_adjoint<double, true>(MelNnlsAdjointArgs<double>);
}  // namespace fast

using namespace mel_nnls;

namespace {

// the largest n_iter whose mask words fit behind one wave's slice with the band form read from global memory (the roomiest
// layout); negative when the slice alone does not fit
template <typename T>
long long max_iter_t(const MelNnlsState& st, int F) {
  const long long slice = ((long long)(2 * F + 2 * st.n_mels + st.nseg) * sizeof(T) + 7) & ~7LL;
  if (slice > kLdsBytes) return -1;
  return std::min<long long>((kLdsBytes - slice) / (8LL * ((F + 63) / 64)), 1 << 24);
}

template <typename T>
int run_t(PlanBase& pl, const T* mel, int n_iter, double power, const T* gmag, T* gmel) {
  MelNnlsState& st = *pl.mel_nnls;
  const int F = pl.n_freq, nwords = (F + 63) / 64;
  const Pick pk = pick_layout<T>(st, F, 8LL * nwords * n_iter);
  SI_CHECK(pk.waves > 0, SPECINV_EUNSUPPORTED,
           "mel_nnls_adjoint: %d iterations of a frame of %d bins and %d mel bands (%s) do not fit a CU's LDS: this shape admits "
           "n_iter <= %lld", n_iter, F, st.n_mels, sizeof(T) == 4 ? "float32" : "float64", max_iter_t<T>(st, F));
  SI_TRY(ensure_beta(pl, st, n_iter));
  fast::MelNnlsAdjointArgs<T> a{};
  a.f.y = mel;
  fill_args<T>(a.f, st, pl, pk, n_iter, power);
  a.g = gmag;
  a.gy = gmel;
  a.nwords = nwords;
  a.slice_bytes = pk.slice_bytes;
  a.mask_off = pk.slice_bytes - 8 * nwords * n_iter;
  const void* fn = pk.staged ? (const void*)fast::k_mel_nnls_adjoint<T, true> : (const void*)fast::k_mel_nnls_adjoint<T, false>;
  SI_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, pk.lds));
  const int grid = grid_size(pk, a.f.n_groups);
  if (a.f.n_groups == 0) return SPECINV_OK;
  if (pk.staged)
    hipLaunchKernelGGL((fast::k_mel_nnls_adjoint<T, true>), dim3(grid), dim3(64 * pk.waves), pk.lds, pl.stream, a);
  else
    hipLaunchKernelGGL((fast::k_mel_nnls_adjoint<T, false>), dim3(grid), dim3(64 * pk.waves), pk.lds, pl.stream, a);
  SI_HIP(hipGetLastError());
  return SPECINV_OK;
}

}  // namespace

int mel_nnls_adjoint_run(PlanBase& pl, const void* mel, int n_iter, double power, const void* gmag, void* gmel_out) {
  if (pl.cfg.dtype == SPECINV_F32)
    return run_t(pl, static_cast<const float*>(mel), n_iter, power, static_cast<const float*>(gmag), static_cast<float*>(gmel_out));
  return run_t(pl, static_cast<const double*>(mel), n_iter, power, static_cast<const double*>(gmag), static_cast<double*>(gmel_out));
}

int mel_nnls_adjoint_max_iter(PlanBase& pl, int* out) {
  const MelNnlsState& st = *pl.mel_nnls;
  const long long n = pl.cfg.dtype == SPECINV_F32 ? max_iter_t<float>(st, pl.n_freq) : max_iter_t<double>(st, pl.n_freq);
  SI_CHECK(n >= 0, SPECINV_EUNSUPPORTED, "mel_nnls_adjoint: a frame of %d bins and %d mel bands does not fit a CU's LDS", pl.n_freq,
           st.n_mels);
  *out = (int)n;
  return SPECINV_OK;
}

}  // namespace specinv
