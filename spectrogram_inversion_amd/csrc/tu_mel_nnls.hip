// k_mel_nnls (kernels_mel_nnls.h) and the plan state behind specinv_mel_nnls_setup / specinv_mel_nnls.
#include "kernels_mel_nnls.h"
#include "mel_nnls_state.h"

namespace specinv {

namespace fast {
template __global__ void k_mel_nnls<float, false>(MelNnlsArgs<float>);
template __global__ void k_mel_nnls<float, true>(MelNnlsArgs<float>);
template __global__ void k_mel_nnls<double, false>(MelNnlsArgs<double>);
template __global__ void k_mel_nnls<double, true>(MelNnlsArgs<double>);
}  // namespace fast

using namespace mel_nnls;

void MelNnlsFree::operator()(MelNnlsState* st) const { delete st; }

namespace {

template <typename T>
int setup_t(PlanBase& pl, const T* mel_fb, int n_mels, double lipschitz) {
  const int F = pl.n_freq;
  SI_CHECK(n_mels <= 32767, SPECINV_EUNSUPPORTED, "mel_nnls: %d mel bands (at most 32767)", n_mels);
  std::vector<T> host((size_t)n_mels * F);
  SI_HIP(hipMemcpyAsync(host.data(), mel_fb, host.size() * sizeof(T), hipMemcpyDeviceToHost, pl.stream));
  SI_HIP(hipStreamSynchronize(pl.stream));
  std::vector<double> M(host.begin(), host.end());
  for (double v : M) SI_CHECK(std::isfinite(v), SPECINV_EINVAL, "mel_nnls: the filterbank holds a non-finite entry");
  fast::MelNnlsBands bd;
  fast::mel_nnls_build(M, n_mels, F, bd);
  std::unique_ptr<MelNnlsState, MelNnlsFree> st(new MelNnlsState());
  st->n_mels = n_mels;
  st->nseg = bd.nseg;
  st->nwr = (int)bd.wr.size();
  st->nwc = (int)bd.wc.size();
  st->piece = bd.piece;
  st->lipschitz = lipschitz;
  // (the kernel's stage: wr | wc | seg | col | rowseg, each 16-byte aligned)
  auto a16 = [](long long bytes) { return (bytes + 15) & ~15LL; };
  st->stage_bytes = a16((long long)st->nwr * sizeof(T)) + a16((long long)st->nwc * sizeof(T)) + 16LL * st->nseg + a16(8LL * F) +
                    a16(4LL * (n_mels + 1));
  std::vector<T> wr(bd.wr.begin(), bd.wr.end()), wc(bd.wc.begin(), bd.wc.end());
  SI_TRY(upload(st->wr, wr.data(), wr.size() * sizeof(T), pl.stream));
  SI_TRY(upload(st->wc, wc.data(), wc.size() * sizeof(T), pl.stream));
  SI_TRY(upload(st->seg, bd.seg.data(), bd.seg.size() * sizeof(int), pl.stream));
  SI_TRY(upload(st->rowseg, bd.rowseg.data(), bd.rowseg.size() * sizeof(int), pl.stream));
  SI_TRY(upload(st->col, bd.col.data(), bd.col.size() * sizeof(int), pl.stream));
  SI_HIP(hipStreamSynchronize(pl.stream));       // (the host vectors go out of scope)
  pl.mel_nnls = std::move(st);
  return SPECINV_OK;
}

template <typename T>
int run_t(PlanBase& pl, const T* mel, int n_iter, double power, T* out) {
  MelNnlsState& st = *pl.mel_nnls;
  const int F = pl.n_freq;
  Pick pk = pick_layout<T>(st, F);
  SI_CHECK(pk.waves > 0, SPECINV_EUNSUPPORTED,
           "mel_nnls: a frame of %d bins and %d mel bands needs %lld bytes of LDS (%s), more than a CU has: use a smaller n_fft "
           "(up to 8192 is supported in both dtypes)", F, st.n_mels, (long long)(2 * F + 2 * st.n_mels + st.nseg) * (long long)sizeof(T),
           sizeof(T) == 4 ? "float32" : "float64");
  SI_TRY(ensure_beta(pl, st, n_iter));
  fast::MelNnlsArgs<T> a{};
  a.y = mel;
  a.out = out;
  fill_args<T>(a, st, pl, pk, n_iter, power);
  const void* fn = pk.staged ? (const void*)fast::k_mel_nnls<T, true> : (const void*)fast::k_mel_nnls<T, false>;
  SI_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, pk.lds));
  const int grid = grid_size(pk, a.n_groups);
  if (a.n_groups == 0) return SPECINV_OK;
  if (pk.staged)
    hipLaunchKernelGGL((fast::k_mel_nnls<T, true>), dim3(grid), dim3(64 * pk.waves), pk.lds, pl.stream, a);
  else
    hipLaunchKernelGGL((fast::k_mel_nnls<T, false>), dim3(grid), dim3(64 * pk.waves), pk.lds, pl.stream, a);
  SI_HIP(hipGetLastError());
  return SPECINV_OK;
}

}  // namespace

int mel_nnls_setup(PlanBase& pl, const void* mel_fb, int n_mels, double lipschitz) {
  pl.mel_nnls.reset();
  if (pl.cfg.dtype == SPECINV_F32) return setup_t(pl, static_cast<const float*>(mel_fb), n_mels, lipschitz);
  return setup_t(pl, static_cast<const double*>(mel_fb), n_mels, lipschitz);
}

int mel_nnls_run(PlanBase& pl, const void* mel, int n_iter, double power, void* mag_out) {
  if (pl.cfg.dtype == SPECINV_F32)
    return run_t(pl, static_cast<const float*>(mel), n_iter, power, static_cast<float*>(mag_out));
  return run_t(pl, static_cast<const double*>(mel), n_iter, power, static_cast<double*>(mag_out));
}

}  // namespace specinv
