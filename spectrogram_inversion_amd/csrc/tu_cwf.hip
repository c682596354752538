// Consistent Wiener filtering: the kernels of kernels_cwf.h, their launches and the host loop of specinv_cwf_run.
#include <vector>

#include "dev_buf.h"
#include "kernels_cwf.h"
#include "plan.h"

namespace specinv {

// what a call needs beyond its outputs: three spectra, Lam, one signal and the sums
struct CwfState {
  DevBuf r, p, u, lam, wave, part, scal, res;
};
void CwfFree::operator()(CwfState* st) const { delete st; }

template <typename T>
int cwf_launch(int which, const CwfArgs<T>& a, int k, hipStream_t stream) {
  const dim3 grid((unsigned)a.nblk, (unsigned)a.batch), blk(kCwfThreads);
  switch (which) {
    case kCwfMax: hipLaunchKernelGGL((k_cwf_max<T>), grid, blk, 0, stream, a); break;
    case kCwfInit: hipLaunchKernelGGL((k_cwf_init<T>), grid, blk, 0, stream, a); break;
    case kCwfU0: hipLaunchKernelGGL((k_cwf_u<T>), grid, blk, 0, stream, a, (const T*)a.S); break;
    case kCwfQ0: hipLaunchKernelGGL((k_cwf_q<T, true>), grid, blk, 0, stream, a); break;
    case kCwfU: hipLaunchKernelGGL((k_cwf_u<T>), grid, blk, 0, stream, a, (const T*)a.P); break;
    case kCwfQ: hipLaunchKernelGGL((k_cwf_q<T, false>), grid, blk, 0, stream, a); break;
    case kCwfUpdate: hipLaunchKernelGGL((k_cwf_update<T>), grid, blk, 0, stream, a, k); break;
    case kCwfDir: hipLaunchKernelGGL((k_cwf_dir<T>), grid, blk, 0, stream, a, k); break;
    case kCwfNoise: hipLaunchKernelGGL((k_cwf_noise<T>), grid, blk, 0, stream, a); break;
    default: return fail(SPECINV_EINVAL, "cwf_launch: unknown kernel %d", which);
  }
  SI_HIP(hipGetLastError());
  return SPECINV_OK;
}
template int cwf_launch<float>(int, const CwfArgs<float>&, int, hipStream_t);
template int cwf_launch<double>(int, const CwfArgs<double>&, int, hipStream_t);

int cwf_residual_launch(const double* part, const double* scal, int batch, int nblk, int k, double* res, hipStream_t stream) {
  hipLaunchKernelGGL(k_cwf_residual, dim3(1, (unsigned)batch), dim3(kCwfThreads), 0, stream, part, scal, batch, nblk, k, res);
  SI_HIP(hipGetLastError());
  return SPECINV_OK;
}

namespace {

template <typename T>
int cwf_run_t(PlanBase& plan, const void* mix, const void* var_s, const void* var_n, double gamma, bool relative, double floor,
              int n_iter, int eva_iter, double tol, void* S_out, void* N_out, double* residual_out_host, int* iters_out) {
  const int batch = plan.cfg.batch;
  const int64_t ft = (int64_t)plan.n_freq * plan.cfg.n_frames, ns = ft * batch;
  if (!plan.cwf) plan.cwf.reset(new CwfState());
  CwfState& st = *plan.cwf;
  const int nblk = cwf_blocks(ft);
  SI_TRY(st.r.reserve((size_t)ns * 2 * sizeof(T)));
  SI_TRY(st.p.reserve((size_t)ns * 2 * sizeof(T)));
  SI_TRY(st.u.reserve((size_t)ns * 2 * sizeof(T)));
  SI_TRY(st.lam.reserve((size_t)ns * sizeof(T)));
  SI_TRY(st.wave.reserve((size_t)batch * plan.length * sizeof(T)));
  SI_TRY(st.part.reserve((size_t)kCwfPartSets * batch * nblk * sizeof(double)));
  SI_TRY(st.scal.reserve((size_t)kCwfScalStride * batch * sizeof(double)));
  SI_TRY(st.res.reserve((size_t)batch * sizeof(double)));
  const hipStream_t stream = plan.stream;

  CwfArgs<T> a{};
  a.mix = static_cast<const T*>(mix);
  a.vs = static_cast<const T*>(var_s);
  a.vn = static_cast<const T*>(var_n);
  a.S = static_cast<T*>(S_out);
  a.Q = static_cast<T*>(N_out);
  a.R = st.r.as<T>();
  a.P = st.p.as<T>();
  a.U = st.u.as<T>();
  a.lam = st.lam.as<T>();
  a.part = st.part.as<double>();
  a.scal = st.scal.as<double>();
  a.ft = ft;
  a.nblk = nblk;
  a.batch = batch;
  a.gamma = gamma;
  a.floor = floor;
  a.shrink = 1.0 - (double)plan.cfg.hop_length / (double)plan.cfg.n_fft;
  a.relative = relative ? 1 : 0;

  // Q <- G src ;  U <- src - Q ;  Q <- G' U: the four transforms around k_cwf_u
  auto consistency = [&](const T* src, int u_kernel) -> int {
    SI_TRY(plan.istft(src, st.wave.p));
    SI_TRY(plan.stft(st.wave.p, plan.length, a.Q));
    SI_TRY(cwf_launch<T>(u_kernel, a, 0, stream));
    SI_TRY(plan.stft_adjoint(a.U, plan.length, st.wave.p));
    return plan.istft_adjoint(st.wave.p, a.Q);
  };
  auto residuals = [&](int k, double* out_host) -> int {
    SI_TRY(cwf_residual_launch(a.part, a.scal, batch, nblk, k, st.res.as<double>(), stream));
    SI_HIP(hipMemcpyAsync(out_host, st.res.p, (size_t)batch * sizeof(double), hipMemcpyDeviceToHost, stream));
    SI_HIP(hipStreamSynchronize(stream));
    return SPECINV_OK;
  };

  SI_TRY(cwf_launch<T>(kCwfMax, a, 0, stream));
  SI_TRY(cwf_launch<T>(kCwfInit, a, 0, stream));
  SI_TRY(consistency(a.S, kCwfU0));
  SI_TRY(cwf_launch<T>(kCwfQ0, a, 0, stream));
  std::vector<double> res_host((size_t)batch);
  int k = 0;
  while (k < n_iter) {
    SI_TRY(consistency(a.P, kCwfU));
    SI_TRY(cwf_launch<T>(kCwfQ, a, 0, stream));
    ++k;
    SI_TRY(cwf_launch<T>(kCwfUpdate, a, k, stream));
    if (tol > 0 && k % eva_iter == 0 && k < n_iter) {
      SI_TRY(residuals(k, res_host.data()));
      bool all = true;
      for (int b = 0; b < batch; ++b) all = all && res_host[b] <= tol;
      if (all) break;
    }
    if (k < n_iter) SI_TRY(cwf_launch<T>(kCwfDir, a, k, stream));
  }
  SI_TRY(cwf_launch<T>(kCwfNoise, a, 0, stream));
  if (iters_out) *iters_out = k;
  return residual_out_host ? residuals(k, residual_out_host) : SPECINV_OK;
}

}  // namespace

int cwf_run(PlanBase& plan, const void* mix, const void* var_s, const void* var_n, double gamma, bool relative, double floor,
            int n_iter, int eva_iter, double tol, void* S_out, void* N_out, double* residual_out_host, int* iters_out) {
  if (plan.cfg.dtype == SPECINV_F32)
    return cwf_run_t<float>(plan, mix, var_s, var_n, gamma, relative, floor, n_iter, eva_iter, tol, S_out, N_out, residual_out_host,
                            iters_out);
  return cwf_run_t<double>(plan, mix, var_s, var_n, gamma, relative, floor, n_iter, eva_iter, tol, S_out, N_out, residual_out_host,
                           iters_out);
}

}  // namespace specinv
