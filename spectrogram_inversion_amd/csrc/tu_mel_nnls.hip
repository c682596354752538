// k_mel_nnls (kernels_mel_nnls.h) and the plan state behind specinv_mel_nnls_setup / specinv_mel_nnls.
#include <mutex>

#include "dev_buf.h"
#include "kernels_mel_nnls.h"
#include "plan.h"

namespace specinv {

namespace fast {
template __global__ void k_mel_nnls<float, false>(MelNnlsArgs<float>);
template __global__ void k_mel_nnls<float, true>(MelNnlsArgs<float>);
template __global__ void k_mel_nnls<double, false>(MelNnlsArgs<double>);
template __global__ void k_mel_nnls<double, true>(MelNnlsArgs<double>);
}  // namespace fast

namespace {

constexpr int kLdsBytes = 160 * 1024;

int upload(DevBuf& d, const void* src, size_t n, hipStream_t stream) {
  SI_TRY(d.reserve(n));
  if (n) SI_HIP(hipMemcpyAsync(d.p, src, n, hipMemcpyHostToDevice, stream));
  return SPECINV_OK;
}

}  // namespace

struct MelNnlsState {
  int n_mels = 0, nseg = 0, nwr = 0, nwc = 0, piece = 0;
  double lipschitz = 0;
  DevBuf wr, wc, seg, rowseg, col, beta;
  int n_beta = 0;
  long long stage_bytes = 0;   // the band form's bytes in LDS
};

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

// momentum table: beta_k = (t_k - 1) / t_{k+1}, t_0 = 1, t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2 - grown, never recomputed: a run of
// n iterations reads the first n entries whatever the longest run so far
int ensure_beta(PlanBase& pl, MelNnlsState& st, int n_iter) {
  if (n_iter <= st.n_beta) return SPECINV_OK;
  const int n = std::max(n_iter, 128);
  std::vector<double> beta(n);
  double t = 1.0;
  for (int k = 0; k < n; ++k) {
    const double tn = (1.0 + std::sqrt(1.0 + 4.0 * t * t)) / 2.0;
    beta[k] = (t - 1.0) / tn;
    t = tn;
  }
  DevBuf fresh;
  SI_TRY(upload(fresh, beta.data(), beta.size() * sizeof(double), pl.stream));
  SI_HIP(hipStreamSynchronize(pl.stream));
  std::swap(st.beta.p, fresh.p);
  std::swap(st.beta.bytes, fresh.bytes);
  st.n_beta = n;
  return SPECINV_OK;
}

struct Pick {
  bool staged = false;
  int waves = 0, per_wave = 0, lds = 0;
};

// the layout that puts the most waves on a CU by LDS (at most 32): the band form staged beside the slices or read from global
// memory (L1 / L2), one to eight waves per workgroup; on a tie the staged form, then four waves (the finer grain of the two that
// fill a CU)
template <typename T>
Pick pick_layout(const MelNnlsState& st, int F) {
  Pick p;
  p.per_wave = 2 * F + 2 * st.n_mels + st.nseg;
  const long long slice = (long long)p.per_wave * sizeof(T);
  int best = 0;
  for (bool staged : {true, false})
    for (int w : {4, 8, 2, 1}) {
      const long long lds = (staged ? st.stage_bytes : 0) + w * slice;
      if (lds > kLdsBytes) continue;
      const int waves_cu = (int)std::min<long long>(32, w * (kLdsBytes / lds));
      if (waves_cu > best) {
        best = waves_cu;
        p.staged = staged;
        p.waves = w;
        p.lds = (int)lds;
      }
    }
  return p;
}

template <typename T>
int run_t(PlanBase& pl, const T* mel, int n_iter, double power, T* out) {
  MelNnlsState& st = *pl.mel_nnls;
  const int F = pl.n_freq, B = pl.cfg.batch, TT = pl.cfg.n_frames;
  Pick pk = pick_layout<T>(st, F);
  SI_CHECK(pk.waves > 0, SPECINV_EUNSUPPORTED,
           "mel_nnls: a frame of %d bins and %d mel bands needs %lld bytes of LDS (%s), more than a CU has: use a smaller n_fft "
           "(up to 8192 is supported in both dtypes)", F, st.n_mels, (long long)(2 * F + 2 * st.n_mels + st.nseg) * (long long)sizeof(T),
           sizeof(T) == 4 ? "float32" : "float64");
  SI_TRY(ensure_beta(pl, st, n_iter));
  fast::MelNnlsArgs<T> a{};
  a.y = mel;
  a.out = out;
  a.beta = static_cast<const double*>(st.beta.p);
  a.wr = static_cast<const T*>(st.wr.p);
  a.wc = static_cast<const T*>(st.wc.p);
  a.seg = static_cast<const int4*>(st.seg.p);
  a.rowseg = static_cast<const int*>(st.rowseg.p);
  a.col = static_cast<const int2*>(st.col.p);
  a.F = F;
  a.n_mels = st.n_mels;
  a.nseg = st.nseg;
  a.nwr = st.nwr;
  a.nwc = st.nwc;
  a.frames = TT;
  a.tgroups = (TT + pk.waves - 1) / pk.waves;
  a.n_groups = a.tgroups * B;
  a.n_iter = n_iter;
  a.per_wave = pk.per_wave;
  a.stage_bytes = pk.staged ? (int)st.stage_bytes : 0;
  a.step = (T)(1.0 / st.lipschitz);
  a.root = power == 1.0 ? 1 : power == 2.0 ? 2 : 0;
  a.inv_power = (T)(1.0 / power);
  static int n_cu = 0;
  static std::once_flag once;
  std::call_once(once, [] {
    int dev = 0;
    hipDeviceProp_t prop{};
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n_cu = prop.multiProcessorCount;
    if (n_cu <= 0) n_cu = 256;
  });
  const void* fn = pk.staged ? (const void*)fast::k_mel_nnls<T, true> : (const void*)fast::k_mel_nnls<T, false>;
  SI_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, pk.lds));
  // one workgroup per group of frames while the chip has room; past that every workgroup walks groups (the band form staged once)
  const int per_cu = std::max(1, std::min(kLdsBytes / pk.lds, 32 / pk.waves));
  const int grid = std::max(1, std::min(a.n_groups, n_cu * per_cu));
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
