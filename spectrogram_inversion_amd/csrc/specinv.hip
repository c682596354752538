// libspecinv.so - the plan and its C ABI entry points (include/specinv.h); the plan-free ops have theirs in their tu_*.hip.
// gfx950 only.
#include <cstdarg>
#include <cstdio>
#include <new>
#include <vector>

#include "entry.h"
#include "kernels_mel_nnls.h"
#include "kernels_mel_nnls_adjoint.h"
#include "plan_impl.h"

namespace specinv {

std::string& last_error() {
  static thread_local std::string msg;
  return msg;
}

int fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  last_error() = buf;
  return code;
}

std::unique_ptr<PlanBase> make_plan_f32() { return std::unique_ptr<PlanBase>(new PlanT<float>()); }
std::unique_ptr<PlanBase> make_plan_f64() { return std::unique_ptr<PlanBase>(new PlanT<double>()); }

// metrics.py:14 (sc, dB), :28-29 (snr), :43 (ser) from the whole-tensor sums
// sums = { sum((out-target)^2), sum(out^2), sum(target^2), count }
double metric_from_sums(int metric, const double s[4]) {
  switch (metric) {
    case SPECINV_METRIC_SC:
      return 20.0 * (std::log10(std::sqrt(s[0])) - std::log10(std::sqrt(s[2])));
    case SPECINV_METRIC_SNR:
      return -10.0 * std::log10(s[0] / s[2]);
    default:
      return 10.0 * (std::log10(s[1]) - std::log10(s[0]));
  }
}

// _training_loop, methods.py:153-190.  Iterations between evaluations are enqueued back to
// back; the host only synchronises at an evaluation.
int PlanBase::run_loop(int max_iter, int eva_iter, double tol, int metric, specinv_eval* evals, int* n_evals,
                       int* iters_done, specinv_eval_cb cb, void* user) {
  SI_CHECK(eva_iter > 0, SPECINV_EINVAL, "eva_iter must be > 0");    // :163
  SI_CHECK(max_iter > 0, SPECINV_EINVAL, "max_iter must be > 0");    // :164
  SI_CHECK(tol >= 0, SPECINV_EINVAL, "tol must be >= 0");            // :165
  SI_CHECK(metric >= 0 && metric <= 2, SPECINV_EINVAL, "unknown metric");  // :168
  double init_loss = 0, prev = 0;
  bool have_init = false;
  int done = 0, ne = 0;
  if (tol == 0.0 && cb == nullptr) {
    // The stop rule `(prev - loss)/init < 0 and prev > loss` (:188) can never fire with tol == 0, and
    // nobody watches the evaluations: enqueue everything, read all sums back once.
    const int n_slots = max_iter / eva_iter;
    SI_TRY(begin_deferred(n_slots));
    int rc = SPECINV_OK;
    while (done < max_iter && rc == SPECINV_OK) {
      const int until_eval = eva_iter - (done % eva_iter);
      if (done + until_eval > max_iter) {
        rc = iterate(max_iter - done, false, nullptr);
        done = max_iter;
        break;
      }
      deferred_slot = ne;
      rc = iterate(until_eval, true, nullptr);
      deferred_slot = -1;
      done += until_eval;
      ++ne;
    }
    deferred_slot = -1;
    SI_TRY(rc);
    std::vector<double> all((size_t)std::max(1, ne) * 4);
    SI_TRY(read_deferred(ne, all.data()));
    for (int i = 0; i < ne && evals; ++i) {
      evals[i].iteration = (i + 1) * eva_iter - 1;
      evals[i].metric = metric_from_sums(metric, &all[4 * i]);
      evals[i].loss = all[4 * i] / all[4 * i + 3];
    }
    if (n_evals) *n_evals = ne;
    if (iters_done) *iters_done = done;
    return SPECINV_OK;
  }
  while (done < max_iter) {
    const int until_eval = eva_iter - (done % eva_iter);             // next i with i % eva == eva-1
    if (done + until_eval > max_iter) {
      SI_TRY(iterate(max_iter - done, false, nullptr));
      done = max_iter;
      break;
    }
    double s[4];
    SI_TRY(iterate(until_eval, true, s));
    done += until_eval;
    specinv_eval ev;
    ev.iteration = done - 1;
    ev.metric = metric_from_sums(metric, s);
    ev.loss = s[0] / s[3];                                            // F.mse_loss, :182
    if (evals) evals[ne] = ev;
    ++ne;
    if (cb && cb(&ev, user) != 0) break;
    if (!have_init || init_loss == 0.0) {                             // `if not init_loss`, :186
      init_loss = ev.loss;
      have_init = true;
    } else if ((prev - ev.loss) / init_loss < tol && prev > ev.loss) {  // :188
      break;
    }
    prev = ev.loss;
  }
  if (n_evals) *n_evals = ne;
  if (iters_done) *iters_done = done;
  return SPECINV_OK;
}

}  // namespace specinv

using namespace specinv;

#define PLAN_OR_FAIL(p) SI_CHECK((p) != nullptr && (p)->impl, SPECINV_EINVAL, "plan is NULL")

extern "C" {

const char* specinv_last_error(void) { return last_error().c_str(); }
int specinv_abi_version(void) { return SPECINV_ABI_VERSION; }
int specinv_has_approx(void) { return 0; }   // (kept for compatibility: there are no approximate-projection kernels)

int specinv_plan_create(const specinv_stft_cfg* cfg, specinv_plan** out) {
  SI_CHECK(cfg && out, SPECINV_EINVAL, "null argument");
  SI_CHECK(cfg->dtype == SPECINV_F32 || cfg->dtype == SPECINV_F64, SPECINV_EINVAL, "bad dtype %d", cfg->dtype);
  specinv_plan* p = new (std::nothrow) specinv_plan();
  SI_CHECK(p, SPECINV_ENOMEM, "out of host memory");
  p->impl = cfg->dtype == SPECINV_F32 ? make_plan_f32() : make_plan_f64();
  p->impl->cfg = *cfg;
  DeviceGuard guard_;                     // setup() selects the plan's device
  (void)guard_.enter(cfg->device, &p->impl->dev_bytes);
  const int rc = p->impl->setup();
  bytes_sink() = nullptr;                 // (p may be deleted below)
  if (rc != SPECINV_OK) {
    delete p;
    return rc;
  }
  *out = p;
  return SPECINV_OK;
}

int specinv_plan_destroy(specinv_plan* plan) {
  if (plan) {
    DeviceGuard guard_;
    if (plan->impl) (void)guard_.enter(plan->impl->cfg.device);
    delete plan;
  }
  return SPECINV_OK;
}

int specinv_plan_set_stream(specinv_plan* plan, void* hip_stream) {
  PLAN_OR_FAIL(plan);
  plan->impl->stream = static_cast<hipStream_t>(hip_stream);
  return SPECINV_OK;
}

int specinv_plan_n_freq(const specinv_plan* plan) { return plan && plan->impl ? plan->impl->n_freq : SPECINV_EINVAL; }
int64_t specinv_plan_length(const specinv_plan* plan) { return plan && plan->impl ? plan->impl->length : SPECINV_EINVAL; }
int specinv_plan_fast_path(const specinv_plan* plan) { return plan && plan->impl ? plan->impl->path_kind() : SPECINV_EINVAL; }
int specinv_transform_objective_kind(const specinv_plan* plan) { return plan && plan->impl ? plan->impl->objective_kind : SPECINV_EINVAL; }
int64_t specinv_plan_device_bytes(const specinv_plan* plan) { return plan && plan->impl ? plan->impl->dev_bytes : SPECINV_EINVAL; }
int specinv_plan_launch_geometry(const specinv_plan* plan, int32_t out[4]) {
  SI_CHECK(plan != nullptr && plan->impl && out, SPECINV_EINVAL, "null argument");
  int g[4] = {0, 0, 0, 0};
  plan->impl->launch_geometry(g);
  for (int i = 0; i < 4; ++i) out[i] = g[i];
  return SPECINV_OK;
}
int specinv_plan_keep_state(specinv_plan* plan, int on) {
  PLAN_OR_FAIL(plan);
  // one-sided plans re-read the flag on every iterate(); a two-sided float32 plan picks its KERNELS by it (the frame kernel carries
  // Y = X + U alone, keep_state takes the coverage kernels and their buffers, reserved by *_init) and latches it there: it is read
  // by the next specinv_gla_init / specinv_admm_init, a running method keeps its kernels
  plan->impl->keep_state = on != 0;
  return SPECINV_OK;
}
int specinv_plan_set_exact(specinv_plan* plan, int) {
  PLAN_OR_FAIL(plan);                   // (kept for compatibility: the reference's operation order is the only arithmetic)
  return SPECINV_OK;
}
int specinv_plan_force_generic(specinv_plan* plan, int on) {
  PLAN_OR_FAIL(plan);
  SI_CHECK(plan->impl->method == Method::None, SPECINV_ESTATE, "cannot switch paths while a method is running");
  plan->impl->force_generic = on != 0;
  return SPECINV_OK;
}

// a plan in the MISI state must not be stepped by another method's entry point: the coupling step would silently be dropped
#define NOT_MISI(plan, name)                                                                                           \
  SI_CHECK((plan)->impl->method != Method::Misi, SPECINV_ESTATE,                                                      \
           name " on a plan in the MISI state would drop the coupling step: use specinv_misi_iterate / specinv_misi_run")

// ... nor one in the AGLA state: the extrapolation would be dropped, and specinv_get_wave would return a stale t
#define NOT_AGLA(plan, name)                                                                                           \
  SI_CHECK((plan)->impl->method != Method::Agla, SPECINV_ESTATE,                                                      \
           name " on a plan in the AGLA state would drop the extrapolation step: use specinv_agla_iterate / specinv_agla_run")

#define ENTER(plan)                                 \
  PLAN_OR_FAIL(plan);                               \
  DeviceGuard guard_;                               \
  SI_HIP(guard_.enter((plan)->impl->cfg.device, &(plan)->impl->dev_bytes))

int specinv_stft(specinv_plan* plan, const void* x, int64_t length, void* spec_out) {
  ENTER(plan);
  return plan->impl->stft(x, length, spec_out);
}
int specinv_istft(specinv_plan* plan, const void* spec, void* x_out) {
  ENTER(plan);
  return plan->impl->istft(spec, x_out);
}
int specinv_envelope(specinv_plan* plan, void* env_out) {
  ENTER(plan);
  return plan->impl->envelope(env_out);
}
int specinv_phase_init(specinv_plan* plan, const void* mag, void* spec_out) {
  ENTER(plan);
  return plan->impl->phase_init(mag, spec_out);
}
int specinv_phase_vocoder(specinv_plan* plan, const void* spec_in, int32_t n_frames_in, double rate, void* spec_out) {
  // (the argument errors before the device is touched)
  SI_CHECK(spec_in && spec_out, SPECINV_EINVAL, "specinv_phase_vocoder: NULL %s", spec_in ? "spec_out" : "spec_in");
  SI_CHECK(spec_in != spec_out, SPECINV_EINVAL, "specinv_phase_vocoder: spec_out must not alias spec_in");
  SI_CHECK(n_frames_in >= 1, SPECINV_EINVAL, "n_frames_in must be >= 1, got %d", n_frames_in);
  SI_CHECK(rate > 0 && std::isfinite(rate), SPECINV_EINVAL, "rate must be finite and > 0, got %g", rate);
  PLAN_OR_FAIL(plan);
  const int64_t want = pvoc_stretched_frames(n_frames_in, rate);
  SI_CHECK(want == (int64_t)plan->impl->cfg.n_frames, SPECINV_EINVAL,
           "the plan holds %d frames, %d frames at rate %g stretch to %lld (make the plan for the output frame count)",
           plan->impl->cfg.n_frames, n_frames_in, rate, (long long)want);
  ENTER(plan);
  return plan->impl->phase_vocoder(spec_in, n_frames_in, rate, spec_out);
}
int specinv_phase_vocoder_locked(specinv_plan* plan, const void* spec_in, int32_t n_frames_in, double rate, int32_t mode,
                                 void* spec_out) {
  // (specinv_phase_vocoder's argument errors in its order, then the mode)
  SI_CHECK(spec_in && spec_out, SPECINV_EINVAL, "specinv_phase_vocoder_locked: NULL %s", spec_in ? "spec_out" : "spec_in");
  SI_CHECK(spec_in != spec_out, SPECINV_EINVAL, "specinv_phase_vocoder_locked: spec_out must not alias spec_in");
  SI_CHECK(n_frames_in >= 1, SPECINV_EINVAL, "n_frames_in must be >= 1, got %d", n_frames_in);
  SI_CHECK(rate > 0 && std::isfinite(rate), SPECINV_EINVAL, "rate must be finite and > 0, got %g", rate);
  SI_CHECK(mode == SPECINV_PVOC_LOCK_NONE || mode == SPECINV_PVOC_LOCK_IDENTITY, SPECINV_EINVAL,
           "mode must be SPECINV_PVOC_LOCK_NONE or SPECINV_PVOC_LOCK_IDENTITY, got %d", mode);
  if (mode == SPECINV_PVOC_LOCK_NONE) return specinv_phase_vocoder(plan, spec_in, n_frames_in, rate, spec_out);
  PLAN_OR_FAIL(plan);
  const int64_t want = pvoc_stretched_frames(n_frames_in, rate);
  SI_CHECK(want == (int64_t)plan->impl->cfg.n_frames, SPECINV_EINVAL,
           "the plan holds %d frames, %d frames at rate %g stretch to %lld (make the plan for the output frame count)",
           plan->impl->cfg.n_frames, n_frames_in, rate, (long long)want);
  ENTER(plan);
  return plan->impl->phase_vocoder_locked(spec_in, n_frames_in, rate, spec_out);
}
int specinv_cwf_run(specinv_plan* plan, const void* mix, const void* var_s, const void* var_n, double gamma, int relative, double floor,
                    int n_iter, int eva_iter, double tol, void* S_out, void* N_out, double* residual_out_host, int* iters_out) {
  // (the argument errors before the device is touched, in the header's order)
  SI_CHECK(mix && var_s && var_n && S_out && N_out, SPECINV_EINVAL, "specinv_cwf_run: NULL %s",
           !mix ? "mix" : !var_s ? "var_s" : !var_n ? "var_n" : !S_out ? "S_out" : "N_out");
  SI_CHECK(S_out != N_out && S_out != mix && N_out != mix && S_out != var_s && S_out != var_n && N_out != var_s && N_out != var_n,
           SPECINV_EINVAL, "specinv_cwf_run: %s", S_out == N_out ? "N_out must not alias S_out" : "an output must not alias an input");
  SI_CHECK(!(((uintptr_t)mix | (uintptr_t)var_s | (uintptr_t)var_n | (uintptr_t)S_out | (uintptr_t)N_out) & 15), SPECINV_EINVAL,
           "specinv_cwf_run: the arrays must be 16-byte aligned");
  SI_CHECK(gamma > 0 && std::isfinite(gamma), SPECINV_EINVAL, "specinv_cwf_run: gamma must be finite and > 0, got %g", gamma);
  SI_CHECK(floor > 0 && floor < 1, SPECINV_EINVAL, "specinv_cwf_run: floor must be in (0, 1), got %g", floor);
  SI_CHECK(n_iter >= 0, SPECINV_EINVAL, "specinv_cwf_run: n_iter must be >= 0, got %d", n_iter);
  SI_CHECK(eva_iter >= 1, SPECINV_EINVAL, "specinv_cwf_run: eva_iter must be >= 1, got %d", eva_iter);
  SI_CHECK(tol >= 0, SPECINV_EINVAL, "specinv_cwf_run: tol must be >= 0, got %g", tol);
  PLAN_OR_FAIL(plan);
  SI_CHECK(plan->impl->cfg.onesided, SPECINV_EUNSUPPORTED, "specinv_cwf_run takes one-sided spectrograms only");
  ENTER(plan);
  return cwf_run(*plan->impl, mix, var_s, var_n, gamma, relative != 0, floor, n_iter, eva_iter, tol, S_out, N_out, residual_out_host,
                 iters_out);
}
int specinv_metric_sums(specinv_plan* plan, const void* a, const void* b, int64_t n, double sums_host[4]) {
  ENTER(plan);
  SI_CHECK(sums_host, SPECINV_EINVAL, "sums_host is NULL");
  return plan->impl->metric_sums(a, b, n, sums_host);
}

int specinv_gla_init(specinv_plan* plan, const void* init_spec, const void* mag, double alpha) {
  ENTER(plan);
  return plan->impl->gla_init(init_spec, mag, alpha);
}
int specinv_gla_iterate(specinv_plan* plan, int n_iter, int eval_last, double sums_host[4]) {
  ENTER(plan);
  NOT_MISI(plan, "specinv_gla_iterate");
  NOT_AGLA(plan, "specinv_gla_iterate");
  SI_CHECK(plan->impl->method == Method::Gla, SPECINV_ESTATE, "specinv_gla_init has not been called");
  return plan->impl->iterate(n_iter, eval_last != 0, sums_host);
}
int specinv_gla_run(specinv_plan* plan, int max_iter, int eva_iter, double tol, int metric, specinv_eval* evals_out,
                    int* n_evals_out, int* iters_done_out, specinv_eval_cb cb, void* user) {
  ENTER(plan);
  NOT_MISI(plan, "specinv_gla_run");
  NOT_AGLA(plan, "specinv_gla_run");
  SI_CHECK(plan->impl->method == Method::Gla, SPECINV_ESTATE, "specinv_gla_init has not been called");
  return plan->impl->run_loop(max_iter, eva_iter, tol, metric, evals_out, n_evals_out, iters_done_out, cb, user);
}

int specinv_admm_init(specinv_plan* plan, const void* init_spec, const void* mag, double rho) {
  ENTER(plan);
  return plan->impl->admm_init(init_spec, mag, rho);
}
int specinv_admm_iterate(specinv_plan* plan, int n_iter, int eval_last, double sums_host[4]) {
  ENTER(plan);
  NOT_MISI(plan, "specinv_admm_iterate");
  NOT_AGLA(plan, "specinv_admm_iterate");
  SI_CHECK(plan->impl->method == Method::Admm, SPECINV_ESTATE, "specinv_admm_init has not been called");
  return plan->impl->iterate(n_iter, eval_last != 0, sums_host);
}
int specinv_admm_run(specinv_plan* plan, int max_iter, int eva_iter, double tol, int metric, specinv_eval* evals_out,
                     int* n_evals_out, int* iters_done_out, specinv_eval_cb cb, void* user) {
  ENTER(plan);
  NOT_MISI(plan, "specinv_admm_run");
  NOT_AGLA(plan, "specinv_admm_run");
  SI_CHECK(plan->impl->method == Method::Admm, SPECINV_ESTATE, "specinv_admm_init has not been called");
  return plan->impl->run_loop(max_iter, eva_iter, tol, metric, evals_out, n_evals_out, iters_done_out, cb, user);
}

int specinv_misi_init(specinv_plan* plan, const void* init_spec, const void* mag, const void* mixture, int64_t mix_stride, int n_src) {
  // (the argument errors before the device is touched; PlanT::misi_init repeats them for its own callers)
  SI_CHECK(init_spec && mixture, SPECINV_EINVAL, "specinv_misi_init: NULL %s (init_spec is required: the host layer forms the mixture-phase start)",
           init_spec ? "mixture" : "init_spec");
  SI_CHECK(n_src >= 1, SPECINV_EINVAL, "n_src must be >= 1, got %d", n_src);
  PLAN_OR_FAIL(plan);
  SI_CHECK(plan->impl->cfg.batch % n_src == 0, SPECINV_EINVAL, "the plan's batch (%d) is not a multiple of n_src (%d)",
           plan->impl->cfg.batch, n_src);
  SI_CHECK(mix_stride >= plan->impl->length, SPECINV_EINVAL, "mix_stride (%lld) is smaller than the plan's signal length (%lld)",
           (long long)mix_stride, (long long)plan->impl->length);
  ENTER(plan);
  return plan->impl->misi_init(init_spec, mag, mixture, mix_stride, n_src);
}
int specinv_misi_iterate(specinv_plan* plan, int n_iter, int eval_last, double sums_host[4]) {
  PLAN_OR_FAIL(plan);
  NOT_AGLA(plan, "specinv_misi_iterate");
  SI_CHECK(plan->impl->method == Method::Misi, SPECINV_ESTATE, "specinv_misi_init has not been called");
  ENTER(plan);
  return plan->impl->iterate(n_iter, eval_last != 0, sums_host);
}
int specinv_misi_run(specinv_plan* plan, int max_iter, int eva_iter, double tol, int metric, specinv_eval* evals_out,
                     int* n_evals_out, int* iters_done_out, specinv_eval_cb cb, void* user) {
  PLAN_OR_FAIL(plan);
  NOT_AGLA(plan, "specinv_misi_run");
  SI_CHECK(plan->impl->method == Method::Misi, SPECINV_ESTATE, "specinv_misi_init has not been called");
  ENTER(plan);
  return plan->impl->run_loop(max_iter, eva_iter, tol, metric, evals_out, n_evals_out, iters_done_out, cb, user);
}

int specinv_agla_init_sched(specinv_plan* plan, const void* init_spec, const void* mag, int n_sched, const double* alpha,
                            const double* beta, const double* gamma) {
  // (the argument errors before the device is touched; PlanT::agla_init_sched repeats them for its own callers)
  SI_CHECK(n_sched >= 1, SPECINV_EINVAL, "n_sched must be >= 1, got %d", n_sched);
  SI_CHECK(alpha && beta && gamma, SPECINV_EINVAL, "specinv_agla_init_sched: NULL %s", !alpha ? "alpha" : !beta ? "beta" : "gamma");
  for (int i = 0; i < n_sched; ++i) {
    SI_CHECK(alpha[i] >= 0 && beta[i] >= 0, SPECINV_EINVAL, "alpha and beta must be >= 0, got %g and %g", alpha[i], beta[i]);
    SI_CHECK(gamma[i] > 0, SPECINV_EINVAL, "gamma must be > 0, got %g", gamma[i]);
  }
  ENTER(plan);
  return plan->impl->agla_init_sched(init_spec, mag, n_sched, alpha, beta, gamma);
}
int specinv_agla_init(specinv_plan* plan, const void* init_spec, const void* mag, double alpha, double beta, double gamma) {
  return specinv_agla_init_sched(plan, init_spec, mag, 1, &alpha, &beta, &gamma);
}
int specinv_agla_constrain(specinv_plan* plan, const void* offset, const void* fixed_mask) {
  PLAN_OR_FAIL(plan);
  SI_CHECK(plan->impl->method == Method::Agla, SPECINV_ESTATE, "specinv_agla_init has not been called");
  SI_CHECK(offset || !fixed_mask, SPECINV_EINVAL, "specinv_agla_constrain: a fixed_mask needs an offset");
  ENTER(plan);
  return plan->impl->agla_constrain(offset, fixed_mask);
}
int specinv_agla_iterate(specinv_plan* plan, int n_iter, int eval_last, double sums_host[4]) {
  PLAN_OR_FAIL(plan);
  SI_CHECK(plan->impl->method == Method::Agla, SPECINV_ESTATE, "specinv_agla_init has not been called");
  ENTER(plan);
  return plan->impl->iterate(n_iter, eval_last != 0, sums_host);
}
int specinv_agla_run(specinv_plan* plan, int max_iter, int eva_iter, double tol, int metric, specinv_eval* evals_out,
                     int* n_evals_out, int* iters_done_out, specinv_eval_cb cb, void* user) {
  PLAN_OR_FAIL(plan);
  SI_CHECK(plan->impl->method == Method::Agla, SPECINV_ESTATE, "specinv_agla_init has not been called");
  ENTER(plan);
  return plan->impl->run_loop(max_iter, eva_iter, tol, metric, evals_out, n_evals_out, iters_done_out, cb, user);
}

int specinv_iterate_eval_dev(specinv_plan* plan, int n_iter, void* sums_dev) {
  ENTER(plan);
  SI_CHECK(plan->impl->method != Method::None, SPECINV_ESTATE, "specinv_gla_init / specinv_admm_init has not been called");
  SI_CHECK(sums_dev != nullptr && n_iter >= 1, SPECINV_EINVAL, "bad arguments");
  plan->impl->eval_dev_out = static_cast<double*>(sums_dev);
  const int rc = plan->impl->iterate(n_iter, true, nullptr);
  plan->impl->eval_dev_out = nullptr;
  return rc;
}

int specinv_get_wave(specinv_plan* plan, void* x_out) {
  ENTER(plan);
  return plan->impl->get_wave(x_out);
}
int specinv_get_state_spec(specinv_plan* plan, int which, void* spec_out) {
  ENTER(plan);
  return plan->impl->get_state_spec(which, spec_out);
}

int specinv_gla_update(specinv_plan* plan, const void* R, const void* P, const void* mag, double lr, void* S_out,
                       void* Q_out) {
  ENTER(plan);
  return plan->impl->gla_update(R, P, mag, lr, S_out, Q_out);
}
int specinv_gla_update_adjoint(specinv_plan* plan, const void* gQ, const void* gP_next, const void* S, const void* mag,
                               double lr, void* gR_out, void* gP_out, void* gmag_accum) {
  ENTER(plan);
  return plan->impl->gla_update_adjoint(gQ, gP_next, S, mag, lr, gR_out, gP_out, gmag_accum);
}
int specinv_admm_update(specinv_plan* plan, const void* R, const void* X, const void* U, const void* mag, double rho,
                        void* Xn_out, void* Un_out, void* V_out, void* Yn_out) {
  ENTER(plan);
  return plan->impl->admm_update(R, X, U, mag, rho, Xn_out, Un_out, V_out, Yn_out);
}
int specinv_admm_update_adjoint(specinv_plan* plan, const void* gYn, const void* gXn, const void* gUn, const void* V,
                                const void* mag, double rho, void* gR_out, void* gX_out, void* gU_out, void* gmag_accum) {
  ENTER(plan);
  return plan->impl->admm_update_adjoint(gYn, gXn, gUn, V, mag, rho, gR_out, gX_out, gU_out, gmag_accum);
}
int specinv_istft_adjoint(specinv_plan* plan, const void* g_x, void* g_spec_out) {
  ENTER(plan);
  return plan->impl->istft_adjoint(g_x, g_spec_out);
}
int specinv_stft_adjoint(specinv_plan* plan, const void* g_spec, int64_t length, void* g_x_out) {
  ENTER(plan);
  return plan->impl->stft_adjoint(g_spec, length, g_x_out);
}
int specinv_misi_mix_adjoint(specinv_plan* plan, int n_src, void* g_inout, void* gmix_accum) {
  // (the argument errors before the device is touched; PlanT repeats them for its own callers)
  SI_CHECK(g_inout && gmix_accum, SPECINV_EINVAL, "specinv_misi_mix_adjoint: NULL %s", g_inout ? "gmix_accum" : "g_inout");
  SI_CHECK(n_src >= 1, SPECINV_EINVAL, "n_src must be >= 1, got %d", n_src);
  PLAN_OR_FAIL(plan);
  SI_CHECK(plan->impl->cfg.batch % n_src == 0, SPECINV_EINVAL, "the plan's batch (%d) is not a multiple of n_src (%d)",
           plan->impl->cfg.batch, n_src);
  ENTER(plan);
  return plan->impl->misi_mix_adjoint(n_src, g_inout, gmix_accum);
}
int specinv_misi_step_adjoint(specinv_plan* plan, int n_src, const void* x_prev, const void* mag_fm, void* g_inout,
                              void* gmix_accum, void* gmag_fm_accum) {
  SI_CHECK(x_prev && mag_fm && g_inout && gmix_accum && gmag_fm_accum, SPECINV_EINVAL, "specinv_misi_step_adjoint: NULL %s",
           !x_prev ? "x_prev" : !mag_fm ? "mag_fm" : !g_inout ? "g_inout" : !gmix_accum ? "gmix_accum" : "gmag_fm_accum");
  SI_CHECK(n_src >= 1, SPECINV_EINVAL, "n_src must be >= 1, got %d", n_src);
  PLAN_OR_FAIL(plan);
  SI_CHECK(plan->impl->cfg.batch % n_src == 0, SPECINV_EINVAL, "the plan's batch (%d) is not a multiple of n_src (%d)",
           plan->impl->cfg.batch, n_src);
  ENTER(plan);
  return plan->impl->misi_step_adjoint(n_src, x_prev, mag_fm, g_inout, gmix_accum, gmag_fm_accum);
}
// (the argument errors before the device is touched; PlanT repeats them for its own callers)
#define AGLA_ADJ_ARGS(name)                                                                                                     \
  SI_CHECK(t_n && t_nm1 && coef && a_inout && gc_inout && c_prev_out && dots_dev_out, SPECINV_EINVAL, name ": NULL %s",         \
           !t_n ? "t_n" : !t_nm1 ? "t_nm1" : !coef ? "coef" : !a_inout ? "a_inout" : !gc_inout ? "gc_inout" : !c_prev_out ? "c_prev_out" \
                                                                                                            : "dots_dev_out"); \
  SI_CHECK(coef[0] >= 0 && coef[1] >= 0 && coef[3] >= 0 && coef[4] >= 0, SPECINV_EINVAL, name ": alpha and beta must be >= 0"); \
  SI_CHECK(coef[2] > 0, SPECINV_EINVAL, name ": gamma must be > 0, got %g", coef[2]);                                           \
  SI_CHECK(gd_inout != nullptr || coef[2] == 1.0, SPECINV_EINVAL, name ": gamma = %g needs gd_inout", coef[2])

int specinv_agla_extrap_adjoint(specinv_plan* plan, const void* t_n, const void* t_nm1, const void* t_nm2, const double coef[5],
                                void* a_inout, void* gc_inout, void* gd_inout, void* c_prev_out, void* dots_dev_out) {
  AGLA_ADJ_ARGS("specinv_agla_extrap_adjoint");
  ENTER(plan);
  return plan->impl->agla_extrap_adjoint(t_n, t_nm1, t_nm2, coef, a_inout, gc_inout, gd_inout, c_prev_out, dots_dev_out, nullptr,
                                         nullptr);
}
int specinv_agla_step_adjoint(specinv_plan* plan, const void* t_n, const void* t_nm1, const void* t_nm2, const double coef[5],
                              void* a_inout, void* gc_inout, void* gd_inout, void* c_prev_out, void* dots_dev_out,
                              const void* mag_fm, void* gmag_fm_accum) {
  AGLA_ADJ_ARGS("specinv_agla_step_adjoint");
  SI_CHECK(mag_fm && gmag_fm_accum, SPECINV_EINVAL, "specinv_agla_step_adjoint: NULL %s", mag_fm ? "gmag_fm_accum" : "mag_fm");
  ENTER(plan);
  return plan->impl->agla_step_adjoint(t_n, t_nm1, t_nm2, coef, a_inout, gc_inout, gd_inout, c_prev_out, dots_dev_out, mag_fm,
                                       gmag_fm_accum, nullptr, nullptr);
}
int specinv_agla_first_adjoint(specinv_plan* plan, const void* c0, const void* a, void* gc_inout, const void* gd, const void* mag_fm,
                               void* gmag_fm_accum) {
  SI_CHECK(c0 && a && gc_inout && mag_fm && gmag_fm_accum, SPECINV_EINVAL, "specinv_agla_first_adjoint: NULL %s",
           !c0 ? "c0" : !a ? "a" : !gc_inout ? "gc_inout" : !mag_fm ? "mag_fm" : "gmag_fm_accum");
  ENTER(plan);
  return plan->impl->agla_first_adjoint(c0, a, gc_inout, gd, mag_fm, gmag_fm_accum, nullptr, nullptr);
}
#define CGLA_ADJ_ARGS(name)                                                                     \
  AGLA_ADJ_ARGS(name);                                                                          \
  SI_CHECK(goff_accum, SPECINV_EINVAL, name ": NULL goff_accum")

int specinv_cgla_extrap_adjoint(specinv_plan* plan, const void* t_n, const void* t_nm1, const void* t_nm2, const double coef[5],
                                const void* fixed_mask, void* a_inout, void* gc_inout, void* gd_inout, void* goff_accum,
                                void* c_prev_out, void* dots_dev_out) {
  CGLA_ADJ_ARGS("specinv_cgla_extrap_adjoint");
  ENTER(plan);
  return plan->impl->agla_extrap_adjoint(t_n, t_nm1, t_nm2, coef, a_inout, gc_inout, gd_inout, c_prev_out, dots_dev_out, fixed_mask,
                                         goff_accum);
}
int specinv_cgla_step_adjoint(specinv_plan* plan, const void* t_n, const void* t_nm1, const void* t_nm2, const double coef[5],
                              const void* fixed_mask, void* a_inout, void* gc_inout, void* gd_inout, void* goff_accum,
                              void* c_prev_out, void* dots_dev_out, const void* mag_fm, void* gmag_fm_accum) {
  CGLA_ADJ_ARGS("specinv_cgla_step_adjoint");
  SI_CHECK(mag_fm && gmag_fm_accum, SPECINV_EINVAL, "specinv_cgla_step_adjoint: NULL %s", mag_fm ? "gmag_fm_accum" : "mag_fm");
  ENTER(plan);
  return plan->impl->agla_step_adjoint(t_n, t_nm1, t_nm2, coef, a_inout, gc_inout, gd_inout, c_prev_out, dots_dev_out, mag_fm,
                                       gmag_fm_accum, fixed_mask, goff_accum);
}
int specinv_cgla_first_adjoint(specinv_plan* plan, const void* c0, const void* fixed_mask, const void* a, void* gc_inout, const void* gd,
                               void* goff_accum, const void* mag_fm, void* gmag_fm_accum) {
  SI_CHECK(c0 && a && gc_inout && goff_accum && mag_fm && gmag_fm_accum, SPECINV_EINVAL, "specinv_cgla_first_adjoint: NULL %s",
           !c0 ? "c0" : !a ? "a" : !gc_inout ? "gc_inout" : !goff_accum ? "goff_accum" : !mag_fm ? "mag_fm" : "gmag_fm_accum");
  ENTER(plan);
  return plan->impl->agla_first_adjoint(c0, a, gc_inout, gd, mag_fm, gmag_fm_accum, fixed_mask, goff_accum);
}
int specinv_project(specinv_plan* plan, const void* x, const void* mag_fm, void* y_out) {
  SI_CHECK(x && mag_fm && y_out, SPECINV_EINVAL, "specinv_project: NULL %s", !x ? "x" : !mag_fm ? "mag_fm" : "y_out");
  SI_CHECK(y_out != x, SPECINV_EINVAL, "specinv_project: y_out must not alias x");
  ENTER(plan);
  return plan->impl->project(x, mag_fm, y_out);
}
int specinv_project_adjoint(specinv_plan* plan, const void* x, const void* mag_fm, const void* g_y, void* g_x_out, void* gmag_fm_out) {
  SI_CHECK(x && mag_fm && g_y && g_x_out && gmag_fm_out, SPECINV_EINVAL, "specinv_project_adjoint: NULL %s",
           !x ? "x" : !mag_fm ? "mag_fm" : !g_y ? "g_y" : !g_x_out ? "g_x_out" : "gmag_fm_out");
  SI_CHECK(g_x_out != g_y && g_x_out != x, SPECINV_EINVAL, "specinv_project_adjoint: g_x_out must not alias g_y or x");
  ENTER(plan);
  return plan->impl->project_adjoint(x, mag_fm, g_y, g_x_out, gmag_fm_out);
}
int specinv_project_adjoint_kind(const specinv_plan* plan, int32_t* kind_out) {
  SI_CHECK(plan != nullptr && plan->impl && kind_out, SPECINV_EINVAL, "null argument");
  *kind_out = plan->impl->project_adjoint_kind();
  return SPECINV_OK;
}
int specinv_phase_init_adjoint(specinv_plan* plan, const void* mag, const void* g_spec, void* gmag_accum) {
  ENTER(plan);
  return plan->impl->phase_init_adjoint(mag, g_spec, gmag_accum);
}

int specinv_rtisi_run(specinv_plan* plan, const void* mag, int look_ahead, int asymmetric_window, int max_iter,
                      double alpha, void* x_out) {
  ENTER(plan);
  return plan->impl->rtisi_run(mag, look_ahead, asymmetric_window, max_iter, alpha, x_out);
}

int specinv_rtisi_record_elems(specinv_plan* plan, int look_ahead, int max_iter, int64_t* n_complex_out) {
  ENTER(plan);
  return plan->impl->rtisi_record_elems(look_ahead, max_iter, n_complex_out);
}
int specinv_rtisi_run_recorded(specinv_plan* plan, const void* mag, int look_ahead, int asymmetric_window, int max_iter,
                               double alpha, void* x_out, void* rec_out) {
  ENTER(plan);
  return plan->impl->rtisi_run_recorded(mag, look_ahead, asymmetric_window, max_iter, alpha, x_out, rec_out);
}
int specinv_rtisi_adjoint(specinv_plan* plan, const void* mag, const void* rec, const void* g_x, int look_ahead,
                          int asymmetric_window, int max_iter, double alpha, void* gmag_out) {
  ENTER(plan);
  return plan->impl->rtisi_adjoint(mag, rec, g_x, look_ahead, asymmetric_window, max_iter, alpha, gmag_out);
}
int specinv_rtisi_stream_begin(specinv_plan* plan, int look_ahead, int asymmetric_window, int max_iter, double alpha) {
  ENTER(plan);
  return plan->impl->rtisi_stream_begin(look_ahead, asymmetric_window, max_iter, alpha);
}
int specinv_rtisi_stream_push(specinv_plan* plan, const void* mag, int k, void* x_out, int64_t out_stride, int64_t* n_out) {
  ENTER(plan);
  return plan->impl->rtisi_stream_push(mag, k, x_out, out_stride, n_out);
}
int specinv_rtisi_stream_flush(specinv_plan* plan, void* x_out, int64_t out_stride, int64_t* n_out) {
  ENTER(plan);
  return plan->impl->rtisi_stream_flush(x_out, out_stride, n_out);
}

// (the scalar arguments are checked ahead of the plan: their messages need no GPU)
int specinv_mel_nnls_setup(specinv_plan* plan, const void* mel_fb, int n_mels, double lipschitz) {
  SI_CHECK(n_mels > 0, SPECINV_EINVAL, "mel_nnls_setup: n_mels must be > 0 (got %d)", n_mels);
  SI_CHECK(std::isfinite(lipschitz) && lipschitz > 0, SPECINV_EINVAL, "mel_nnls_setup: lipschitz must be finite and > 0 (got %g)",
           lipschitz);
  SI_CHECK(mel_fb != nullptr, SPECINV_EINVAL, "mel_nnls_setup: mel_fb is NULL");
  ENTER(plan);
  return mel_nnls_setup(*plan->impl, mel_fb, n_mels, lipschitz);
}
int specinv_mel_nnls(specinv_plan* plan, const void* mel, int n_iter, double power, void* mag_out) {
  SI_CHECK(n_iter >= 0, SPECINV_EINVAL, "mel_nnls: n_iter must be >= 0 (got %d)", n_iter);
  SI_CHECK(std::isfinite(power) && power > 0, SPECINV_EINVAL, "mel_nnls: power must be finite and > 0 (got %g)", power);
  SI_CHECK(mel != nullptr && mag_out != nullptr, SPECINV_EINVAL, "mel_nnls: mel / mag_out is NULL");
  PLAN_OR_FAIL(plan);
  SI_CHECK(plan->impl->mel_nnls != nullptr, SPECINV_EINVAL, "mel_nnls: specinv_mel_nnls_setup has not been called on this plan");
  ENTER(plan);
  return mel_nnls_run(*plan->impl, mel, n_iter, power, mag_out);
}
int specinv_mel_nnls_adjoint(specinv_plan* plan, const void* mel, int n_iter, double power, const void* gmag, void* gmel_out) {
  SI_CHECK(n_iter >= 0, SPECINV_EINVAL, "mel_nnls_adjoint: n_iter must be >= 0 (got %d)", n_iter);
  SI_CHECK(std::isfinite(power) && power > 0, SPECINV_EINVAL, "mel_nnls_adjoint: power must be finite and > 0 (got %g)", power);
  SI_CHECK(mel != nullptr && gmag != nullptr && gmel_out != nullptr, SPECINV_EINVAL, "mel_nnls_adjoint: mel / gmag / gmel_out is NULL");
  PLAN_OR_FAIL(plan);
  SI_CHECK(plan->impl->mel_nnls != nullptr, SPECINV_EINVAL,
           "mel_nnls_adjoint: specinv_mel_nnls_setup has not been called on this plan");
  ENTER(plan);
  return mel_nnls_adjoint_run(*plan->impl, mel, n_iter, power, gmag, gmel_out);
}
int specinv_mel_nnls_adjoint_max_iter(specinv_plan* plan, int* out) {
  SI_CHECK(out != nullptr, SPECINV_EINVAL, "mel_nnls_adjoint_max_iter: out is NULL");
  PLAN_OR_FAIL(plan);
  SI_CHECK(plan->impl->mel_nnls != nullptr, SPECINV_EINVAL,
           "mel_nnls_adjoint_max_iter: specinv_mel_nnls_setup has not been called on this plan");
  return mel_nnls_adjoint_max_iter(*plan->impl, out);
}

int specinv_transform_setup(specinv_plan* plan, int kind, const void* mel_fb, int n_mels) {
  ENTER(plan);
  return plan->impl->transform_setup(kind, mel_fb, n_mels);
}
int specinv_transform_forward(specinv_plan* plan, const void* x, int64_t length, void* v_out) {
  ENTER(plan);
  return plan->impl->transform_forward(x, length, v_out);
}
int specinv_transform_loss_grad(specinv_plan* plan, const void* x, int64_t length, const void* target,
                                double* loss_host, void* grad_out) {
  ENTER(plan);
  return plan->impl->transform_loss_grad(x, length, target, loss_host, grad_out);
}
int specinv_transform_loss_grad_dev(specinv_plan* plan, const void* x, int64_t length, const void* target,
                                    double* loss_dev, void* grad_out) {
  ENTER(plan);
  SI_CHECK(loss_dev, SPECINV_EINVAL, "loss_dev is NULL");
  return plan->impl->transform_loss_grad(x, length, target, nullptr, grad_out, loss_dev);
}
int specinv_transform_loss_grad_stats_dev(specinv_plan* plan, const void* x, int64_t length, const void* target, const void* d,
                                          double* out5_dev, void* grad_out) {
  ENTER(plan);
  SI_CHECK(out5_dev, SPECINV_EINVAL, "out5_dev is NULL");
  return plan->impl->transform_loss_grad(x, length, target, nullptr, grad_out, out5_dev, true, d);
}
int specinv_vec_dot(specinv_plan* plan, const void* a, const void* b, int64_t n, double* out_host) {
  ENTER(plan);
  return plan->impl->vec_dot(a, b, n, out_host);
}
int specinv_vec_axpy(specinv_plan* plan, double alpha, const void* x, void* y, int64_t n) {
  ENTER(plan);
  return plan->impl->vec_axpy(alpha, x, y, n);
}
int specinv_vec_scale(specinv_plan* plan, double alpha, const void* x, void* y, int64_t n) {
  ENTER(plan);
  return plan->impl->vec_scale(alpha, x, y, n);
}
int specinv_vec_absmax_abssum(specinv_plan* plan, const void* x, int64_t n, double out_host[2]) {
  ENTER(plan);
  return plan->impl->vec_absmax_abssum(x, n, out_host);
}

int specinv_vec_multi_dot(specinv_plan* plan, const void* g, const void* const* vecs_host, int k, int64_t n,
                          double* out_host) {
  ENTER(plan);
  return plan->impl->vec_multi_dot(g, vecs_host, k, n, out_host);
}
int specinv_vec_lincomb(specinv_plan* plan, const void* const* vecs_host, const double* coef_host, int k, int64_t n,
                        void* out) {
  ENTER(plan);
  return plan->impl->vec_lincomb(vecs_host, coef_host, k, n, out);
}
int specinv_vec_lincomb_step(specinv_plan* plan, const void* const* vecs_host, const double* coef_host, int k, int64_t n,
                             void* out, double t, void* x) {
  ENTER(plan);
  return plan->impl->vec_lincomb_step(vecs_host, coef_host, k, n, out, t, x);
}

int specinv_lbfgs_direction(specinv_plan* plan, const void* g, const void* const* s_list_host,
                            const void* const* y_list_host, const double* rho_host, int m, double h_diag, void* d_out,
                            int64_t n) {
  ENTER(plan);
  return plan->impl->lbfgs_direction(g, s_list_host, y_list_host, rho_host, m, h_diag, d_out, n);
}
int specinv_lbfgs_pair(specinv_plan* plan, const void* g, const void* g_prev, const void* d, double t, void* y_out,
                       void* s_out, int64_t n, double* out_host) {
  ENTER(plan);
  return plan->impl->lbfgs_pair(g, g_prev, d, t, y_out, s_out, n, out_host);
}
int specinv_lbfgs_stats(specinv_plan* plan, const void* g, const void* d, int64_t n, double* out_host) {
  ENTER(plan);
  return plan->impl->lbfgs_stats(g, d, n, out_host);
}

int specinv_vec_multi_dot_dev(specinv_plan* plan, const void* g, const void* const* vecs_host, int k, int64_t n,
                              double* out_dev) {
  ENTER(plan);
  SI_CHECK(out_dev, SPECINV_EINVAL, "out_dev is NULL");
  return plan->impl->vec_multi_dot(g, vecs_host, k, n, nullptr, out_dev);
}
int specinv_lbfgs_pair_dev(specinv_plan* plan, const void* g, const void* g_prev, const void* d, double t, void* y_out,
                           void* s_out, int64_t n, double* out_dev) {
  ENTER(plan);
  SI_CHECK(out_dev, SPECINV_EINVAL, "out_dev is NULL");
  return plan->impl->lbfgs_pair(g, g_prev, d, t, y_out, s_out, n, nullptr, out_dev);
}
int specinv_lbfgs_stats_dev(specinv_plan* plan, const void* g, const void* d, int64_t n, double* out_dev) {
  ENTER(plan);
  SI_CHECK(out_dev, SPECINV_EINVAL, "out_dev is NULL");
  return plan->impl->lbfgs_stats(g, d, n, nullptr, out_dev);
}
int specinv_lbfgs_pair_stats_dev(specinv_plan* plan, const void* g, const void* g_prev, const void* d, double t,
                                 void* y_out, void* s_out, int64_t n, double* out_dev) {
  ENTER(plan);
  SI_CHECK(out_dev, SPECINV_EINVAL, "out_dev is NULL");
  return plan->impl->lbfgs_pair_stats(g, g_prev, d, t, y_out, s_out, n, out_dev);
}
int specinv_read_doubles(specinv_plan* plan, const double* src_dev, int n, double* out_host) {
  ENTER(plan);
  return plan->impl->read_doubles(src_dev, n, out_host);
}
int specinv_board_alloc(specinv_plan* plan, int n, double** host_out, double** dev_out) {
  ENTER(plan);
  return plan->impl->board_alloc(n, host_out, dev_out);
}
int specinv_stream_wait(specinv_plan* plan) {
  ENTER(plan);
  return plan->impl->stream_wait();
}
int specinv_lbfgs_dev_create(specinv_plan* plan, int64_t n, const specinv_lbfgs_opts* opts, int32_t* handle_out) {
  ENTER(plan);
  return plan->impl->lbfgs_dev_create(n, opts, handle_out);
}
int specinv_lbfgs_dev_step(specinv_plan* plan, int32_t handle, void* x, int64_t length, const void* target,
                           specinv_lbfgs_info* info_out) {
  ENTER(plan);
  return plan->impl->lbfgs_dev_step(handle, x, length, target, info_out);
}
int specinv_lbfgs_dev_destroy(specinv_plan* plan, int32_t handle) {
  ENTER(plan);
  return plan->impl->lbfgs_dev_destroy(handle);
}

}  // extern "C"
