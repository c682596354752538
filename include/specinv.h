/*
 * specinv.h - C ABI of libspecinv.so, the MI355X (gfx950) spectrogram-inversion engine.
 *
 * The reference (yoyololicon/spectrogram-inversion, package torch_specinv) has no FFI of
 * its own: its hot path is a set of plain Python functions exported at
 * torch_specinv/__init__.py:6.  This header is the boundary a binding for that path would
 * use; every entry point names the reference code it replaces (paths relative to the
 * reference checkout).  The Python host layer in spectrogram_inversion_amd/ binds it with
 * ctypes and mirrors the reference's function signatures on top.
 *
 * Conventions
 *   - plain C: opaque plan handle, raw pointers, ints/doubles; no exceptions cross the ABI.
 *   - every function returns 0 on success or a negative SPECINV_E* code; the message for the
 *     calling thread's last failure is available from specinv_last_error().
 *   - all data pointers are DEVICE pointers (HIP, the plan's device) unless the parameter
 *     name ends in _host.  The caller owns them; the plan owns its internal state buffers.
 *   - spectrogram arguments use the reference's layout: row-major (batch, n_freq, n_frames),
 *     real (float/double) or complex interleaved (re, im).  Waveforms are (batch, length).
 *   - work is enqueued on the plan's stream (specinv_plan_set_stream; default: the null
 *     stream).  Functions that return scalars to the host synchronise that stream.
 *   - a plan is not thread-safe; different plans may be used from different threads.
 */
#ifndef SPECINV_H
#define SPECINV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPECINV_ABI_VERSION 1

enum {
  SPECINV_OK = 0,
  SPECINV_EINVAL = -1,       /* bad argument (the host layer raises AssertionError / ValueError) */
  SPECINV_EHIP = -2,         /* a HIP runtime call failed */
  SPECINV_EUNSUPPORTED = -3, /* configuration not implemented on the device path */
  SPECINV_ENOMEM = -4,
  SPECINV_ESTATE = -5        /* call sequence error (e.g. iterate before init) */
};

enum { SPECINV_F32 = 0, SPECINV_F64 = 1 };
enum { SPECINV_PAD_REFLECT = 0, SPECINV_PAD_CONSTANT = 1, SPECINV_PAD_REPLICATE = 2, SPECINV_PAD_CIRCULAR = 3 };
enum { SPECINV_METRIC_SC = 0, SPECINV_METRIC_SNR = 1, SPECINV_METRIC_SER = 2 };

/* Normalised STFT arguments: what torch_specinv/methods.py:21-91 (_args_helper) returns,
 * plus the problem shape.  `window_host` has n_fft elements of `dtype` and is already
 * centre-padded (methods.py:80-83). */
typedef struct specinv_stft_cfg {
  int32_t n_fft;
  int32_t hop_length;
  int32_t n_frames;      /* T */
  int32_t batch;         /* B, at most 65535 (the batch is a grid dimension of the layout kernels) */
  int32_t center;        /* bool */
  int32_t pad_mode;      /* SPECINV_PAD_* ; only read by the forward STFT when center != 0 */
  int32_t normalized;    /* bool: 'ortho' scaling both ways (methods.py:142-146) */
  int32_t onesided;      /* bool */
  int32_t dtype;         /* SPECINV_F32 / SPECINV_F64 */
  int32_t device;        /* HIP device ordinal */
  const void* window_host;
} specinv_stft_cfg;

typedef struct specinv_plan specinv_plan;

/* One evaluation of _training_loop (methods.py:180-184): metric value and F.mse_loss. */
typedef struct specinv_eval {
  int32_t iteration;     /* 0-based index of the iteration that was evaluated */
  double metric;
  double loss;
} specinv_eval;

/* Progress callback, called on the host after each evaluation; return non-zero to abort. */
typedef int (*specinv_eval_cb)(const specinv_eval* ev, void* user);

/* Whole-tensor sums behind metrics.py:14,28-29,43 and F.mse_loss:
 * sums[0] = sum((a-b)^2), sums[1] = sum(a^2), sums[2] = sum(b^2), sums[3] = element count. */

const char* specinv_last_error(void);
int specinv_abi_version(void);
/* Kept for compatibility: always 0.  The library carries no approximate-projection kernels; the reference's operation order
 * (specinv_plan_set_exact) is its only arithmetic. */
int specinv_has_approx(void);

/* ---- plan ---------------------------------------------------------------------------- */
int specinv_plan_create(const specinv_stft_cfg* cfg, specinv_plan** out);
int specinv_plan_destroy(specinv_plan* plan);
int specinv_plan_set_stream(specinv_plan* plan, void* hip_stream);
/* n_freq (F), signal length L = (T-1)*hop + n_fft - 2*pad (methods.py:127), and which iteration kernels the plan
 * uses: 1 = fused (one launch per iteration: wave-level FFT, register overlap-add; float32, one-sided, centred,
 * n_fft 512 / 1024 / 2048 / 4096, hop = n_fft/2, /4 or /8, >= n_fft/hop + 2 frames), 2 = the same wave-level frame
 * kernel + gather overlap-add (those n_fft, any hop / centring; two-sided float32 spectrograms as well), 3 = that frame
 * kernel walking chunks of frames with the overlap-add in LDS (n_fft <= 2048, hop <= n_fft, >= 12288 frames in the batch at
 * n_fft 2048, >= 32768 below; one- or two-sided), 0 = generic LDS-FFT kernels (everything else: float64, other sizes, a
 * two-sided run with specinv_plan_keep_state). */
int specinv_plan_n_freq(const specinv_plan* plan);
int64_t specinv_plan_length(const specinv_plan* plan);
int specinv_plan_fast_path(const specinv_plan* plan);
/* Device memory currently held by the plan's own buffers, in bytes (state, scratch, tables; grows as entry points
 * reserve what they need).  The host layer caps its plan cache with it. */
int64_t specinv_plan_device_bytes(const specinv_plan* plan);
/* Launch geometry of the iteration kernel (diagnostics; the tests assert that the benchmark's geometry is the one they
 * cover): out = { waves per workgroup, chunks of frames per item, waves per launch, kernel }, kernel: 0 generic
 * k_iter_pair, 1 k_fused4 (hop = n_fft/4 at n_fft 1024 / 2048), 2 k_fused<R, OV>, 3 k_semi, 4 k_hop, 5 k_fused4_td and
 * 6 k_fused_td<R, OV>, 7 k_hop_td (Griffin-Lim with the momentum carried as a signal; known once specinv_gla_init has run),
 * 8 k_wave_iter (the generic path's wave-level kernel: n_fft 128 ... 8192 (float32: 16384) and 400 / 800 / 1000; frames buffer + k_ola where out[1] is
 * the frame count, else the overlap-add in its registers), 9 k_wave_iter with the overlap-add in an LDS ring. */
int specinv_plan_launch_geometry(const specinv_plan* plan, int32_t out[4]);
/* 0: allow the fast path when the configuration supports it (default); 1: force the generic kernels. */
int specinv_plan_force_generic(specinv_plan* plan, int on);
/* Kept for compatibility: checks the plan and returns SPECINV_OK, whatever `on` is.  The float32 wave-level kernels (fused, frame,
 * chunked frame) always compute the magnitude projection S * m / (|S| + 1e-16) and the division by the overlap-add envelope
 * (torch_specinv/methods.py:132,246-247) in the reference's operation order - ATen executes the projection as (S * m) * r with r
 * the rounded reciprocal of |S| + 1e-16 (tools/ref_ops_probe.py) - with r the correctly rounded 1 / |S| (one Newton step on
 * v_rsq_f32) and a correctly rounded division by the envelope: 73 % of the projected bins bit-identical to the reference's chain,
 * every one within its rounding noise.  The generic kernels and float64 use IEEE operations in the reference's order throughout. */
int specinv_plan_set_exact(specinv_plan* plan, int on);
/* The float32 fast paths do not carry the reference's spectral state as such.
 * ADMM keeps only Y = X + U between iterations: methods.py:467-468 read the two as U + X, i.e. the Y that :475 has just
 * rounded, so the iterates are bit-identical and the state traffic halves.  Griffin-Lim on the fused shapes (hop = n_fft/2, /4, /8) and on the chunked
 * frame kernel keeps its momentum as the signal z_t = x_t - lr z_{t-1} (pre_t = STFT(z_t) + (-lr)^t c0 by linearity of the STFT):
 * pre_spec is never formed.
 * 1: ADMM - the last iteration of every specinv_admm_iterate call (and specinv_admm_init) also leaves X and U behind for
 * specinv_get_state_spec; Griffin-Lim - the iteration runs on pre_spec itself (the spectral-state kernel).
 * 0 (default): asking for X / U / pre_spec after an iteration is SPECINV_ESTATE.  Call before specinv_*_init: where the flag
 * selects the kernels (a two-sided float32 run keeps X and U on the generic kernels only) it is latched by specinv_gla_init /
 * specinv_admm_init - a later call takes effect at the next init, the running method keeps its kernels and buffers.
 * (The generic kernels keep X and U anyway; the frame-at-a-time and generic Griffin-Lim kernels keep pre_spec.) */
int specinv_plan_keep_state(specinv_plan* plan, int on);

/* ---- building blocks ------------------------------------------------------------------ */
/* torch.stft(x, n_fft, **processed_args) as called at methods.py:241.  x (B, L_in) -> spec
 * (B, F, T) complex.  L_in must give exactly the plan's T frames. */
int specinv_stft(specinv_plan* plan, const void* x, int64_t length, void* spec_out);
/* _istft + _ola, methods.py:114-150: spec (B, F, T) complex -> x (B, L) = OLA / envelope. */
int specinv_istft(specinv_plan* plan, const void* spec, void* x_out);
/* window-square envelope of methods.py:129-131, (L,) */
int specinv_envelope(specinv_plan* plan, void* env_out);
/* phase_init, methods.py:572-615: mag (B, F, T) real -> (B, F, T) complex */
int specinv_phase_init(specinv_plan* plan, const void* mag, void* spec_out);
/* The phase vocoder (not in the reference; csrc/kernels_pvoc.h): spec_in (B, F, n_frames_in) complex resampled along time to
 * spec_out (B, F, T_out) complex, T_out the plan's frame count - the plan is made for the OUTPUT, the one the inversion that
 * follows uses.  T_out must be the smallest n >= 1 with (double)n * rate >= n_frames_in; rate > 1 shortens.  With t_j = j * rate,
 * i = floor(t_j), a = t_j - i and frames at and beyond n_frames_in read as +0 + 0i:
 *     |P[j]| = a |S[i+1]| + (1 - a) |S[i]| ;  arg P[0] = arg S[0] ;  arg P[j+1] = arg P[j] + wrap(arg S[i+1] - arg S[i] - adv) + adv,
 * adv = 2 pi k_s hop / n_fft (k_s the signed bin), wrap(x) = x - 2 pi round(x / 2 pi).  Everything after the two angles is
 * float64 for both dtypes, the running sum included; the result is rounded once.  Stateless: a running method is not disturbed.
 * SPECINV_EINVAL, before the device is touched: a NULL pointer, spec_out == spec_in, n_frames_in < 1, a rate that is not finite and
 * positive, a NULL plan, a plan whose frame count is not T_out. */
int specinv_phase_vocoder(specinv_plan* plan, const void* spec_in, int32_t n_frames_in, double rate, void* spec_out);
/* The same with a phase-locking mode (csrc/kernels_pvoc_lock.h).  SPECINV_PVOC_LOCK_NONE is specinv_phase_vocoder, bit for bit.
 * SPECINV_PVOC_LOCK_IDENTITY is identity phase locking (Laroche & Dolson 1999): with S0 = S[i] and q[k] = re^2 + im^2 of S0[k] in
 * float64, bin k is a peak of output frame j when q[k] > q[k'] for k' = k +- 1, k +- 2 (modulo n_fft on a two-sided spectrum, dropped
 * outside 0 .. F - 1 on a one-sided one, dropped where k' + k = 0 mod n_fft: the bin's own mirror image); every bin takes the
 * nearest peak p of its frame (circular distance on a two-sided spectrum; a tie goes to the smaller |k_s|, then to the lower
 * index) and arg P[j][k] = (phi[p] - arg S0[p]) + arg S0[k], phi the unlocked running phase above, in float64; a frame without a
 * peak keeps phi.  |P| is unchanged.  Two launches; the first identity call reserves batch * F * T_out doubles in the plan.
 * The errors are specinv_phase_vocoder's, in its order; an unknown mode is SPECINV_EINVAL ("mode"), after the rate. */
enum { SPECINV_PVOC_LOCK_NONE = 0, SPECINV_PVOC_LOCK_IDENTITY = 1 };
int specinv_phase_vocoder_locked(specinv_plan* plan, const void* spec_in, int32_t n_frames_in, double rate, int32_t mode,
                                 void* spec_out);
/* Sample-rate conversion (not in the reference; csrc/kernels_resample.h): x (batch, n_in) -> y (batch, n_out), real device arrays of
 * `dtype` (SPECINV_F32 / SPECINV_F64) on HIP device `device`, enqueued on hip_stream (NULL: the null stream).  No plan: nothing is
 * kept between calls.  With o : n = orig_freq : new_freq reduced, base = min(o, n) * rolloff, W = lowpass_filter_width and x read
 * as zero outside 0 ... n_in - 1 (torchaudio's sinc_interp_hann resampling, per output sample):
 *     y[m] = (base / o) sum_{s : |tau| < W} sinc(tau) cos^2(pi tau / (2 W)) x[s] ;  tau = base (s n - m o) / (o n) ,
 * sinc(t) = sin(pi t) / (pi t).  n_out must be ceil(n * n_in / o).  Weights and sum are float64 for both dtypes; the result is
 * rounded once.  o == n copies x.  Any batch: it is not a launch dimension of its own.  SPECINV_EINVAL, before the device is
 * touched: a NULL pointer, y == x, batch or n_in < 1, orig_freq or new_freq < 1, lowpass_filter_width < 1, a rolloff outside (0, 1],
 * an n_out that is not ceil(n * n_in / o), n_out * o beyond 62 bits, an unknown dtype.  At the launch: ceil(W o / base) of 2^30 or more. */
int specinv_resample(const void* x, void* y, int64_t batch, int64_t n_in, int64_t n_out, int64_t orig_freq, int64_t new_freq,
                     int32_t lowpass_filter_width, double rolloff, int32_t dtype, int32_t device, void* hip_stream);
/* Harmonic-percussive separation (not in the reference; csrc/kernels_hpss.h): librosa.decompose.hpss in one launch.  spec is
 * (batch, n_freq, n_frames) on HIP device `device`, real non-negative magnitudes of `dtype` or, with is_complex != 0, (re, im) pairs
 * of `dtype`; enqueued on hip_stream (NULL: the null stream).  No plan: nothing about an STFT is read and nothing is kept.
 *     A = spec, or sqrt(re^2 + im^2) in float64 ;  refl(i, n) = j < n ? j : 2 n - 1 - j with j = i mod 2 n (>= 0) ;
 *     harm[f, t] = median{ A[f, refl(t + d, T)] : |d| <= win_harm / 2 } ;  perc[f, t] = median{ A[refl(f + d, F), t] : |d| <= win_perc / 2 } ;
 *     soft(X, R): power = inf: X > R ? 1 : 0 ; else Z = max(X, R) ; Z < tiny: (both margins 1 ? 0.5 : 0) ; else a = (X / Z)^power,
 *     r = (R / Z)^power, a / (a + r) ;  M_h = soft(harm, margin_harm * perc) ;  M_p = soft(perc, margin_perc * harm) ;
 * tiny is the smallest normal number of `dtype`.  The windows are odd, 1 ... 127, so a median is an element of its window (exact
 * selection).  From Z on everything is float64 for both dtypes and the result is rounded once.  out_a, out_b by out_mode:
 *     SPECINV_HPSS_COMPONENTS  spec * M_h, spec * M_p, of spec's kind (complex for a complex input) ;
 *     SPECINV_HPSS_MASKS       M_h, M_p, real ;      SPECINV_HPSS_MEDIANS     harm, perc, real.
 * Any batch: it is not a launch dimension of its own.  NaN input is unspecified.  Stateless: a running method is not disturbed.
 * SPECINV_EINVAL, before the device is touched, in this order: a NULL pointer (spec, out_a, out_b) ; an output that is spec or the
 * other output ; batch, n_freq or n_frames < 1 ; win_harm, then win_perc, even or outside 1 ... 127 ; power not > 0 (NaN included) ;
 * margin_harm, then margin_perc, < 1 or not finite ; an unknown out_mode ; an unknown dtype. */
enum { SPECINV_HPSS_COMPONENTS = 0, SPECINV_HPSS_MASKS = 1, SPECINV_HPSS_MEDIANS = 2 };
int specinv_hpss(const void* spec, void* out_a, void* out_b, int64_t batch, int32_t n_freq, int32_t n_frames, int32_t win_harm,
                 int32_t win_perc, double power, double margin_harm, double margin_perc, int32_t out_mode, int32_t is_complex,
                 int32_t dtype, int32_t device, void* hip_stream);
/* Spectral envelope (not in the reference; csrc/kernels_envelope.h): the true-envelope estimator of Roebel & Rodet 2005 in one
 * launch.  spec is a one-sided spectrogram on HIP device `device`, (batch, n_freq, n_frames) or with frame_major != 0
 * (batch, n_frames, n_freq), real non-negative magnitudes of `dtype` or, with is_complex != 0, (re, im) pairs of `dtype`; out is real,
 * in the same layout; amin is a (batch,) device array of `dtype`; enqueued on hip_stream (NULL: the null stream).  No plan: nothing
 * about an STFT is read but N = 2 (n_freq - 1), and nothing is kept.  Per item and frame:
 *     a0[k] = log(max(|spec[k]|, amin[item])), or 0 for every k where amin[item] <= 0 (an all-zero item) ;
 *     C(a)  = Re rfft(irfft(a, N) * l),  l[q] = 1 if min(q, N - q) <= order else 0 ;
 *     V_0 = C(a0), V_i = C(max(a0, V_{i-1})) for i = 1 ... n_iter ;  out = V_{n_iter} if out_log != 0 else exp(V_{n_iter}).
 * n_iter is a count, not a stop rule; n_iter = 0 is plain cepstral smoothing; order = N / 2 is the identity.  Any batch: it is not
 * a launch dimension of its own.  NaN input is unspecified.  Stateless: a running method is not disturbed.
 * Before the device is touched, in this order: SPECINV_EINVAL for a NULL pointer (spec, out, amin) ; out == spec ; batch or
 * n_frames < 1 ; n_iter outside 0 ... 256 ; an unknown dtype ; then SPECINV_EUNSUPPORTED for SPECINV_F64 ; an n_freq that is not
 * 129, 257, 513 or 1025 (n_fft 256, 512, 1024, 2048) ; then SPECINV_EINVAL for order outside 0 ... N / 2. */
int specinv_spectral_envelope(const void* spec, void* out, const void* amin, int64_t batch, int32_t n_freq, int32_t n_frames,
                              int32_t order, int32_t n_iter, int32_t out_log, int32_t is_complex, int32_t frame_major, int32_t dtype,
                              int32_t device, void* hip_stream);
/* YIN f0 tracking (not in the reference; csrc/kernels_yin.h): the estimator of de Cheveigne & Kawahara 2002 in one launch.  x is
 * (batch, length), real, of `dtype`, on HIP device `device`; period_out and aper_out are (batch, T) float32, tau_out (batch, T) int32 or
 * NULL, cmnd_out (batch, T, W + 1) float32 or NULL; enqueued on hip_stream (NULL: the null stream).  No plan: nothing is kept between
 * calls.  With N = frame, W = N / 2, H = hop and xz(i) = x[i] for 0 <= i < length, else 0:
 *     Frames.      center != 0: T = 1 + length / H, s_m = m H - W ;  center == 0: T = 1 + (length - N) / H, s_m = m H ;
 *                  f_m[j] = xz(s_m + j), j < N.
 *     Difference.  d(tau) = sum_{j<W} (f[j] - f[j+tau])^2 = E(0) + E(tau) - 2 r(tau), tau = 0 ... W ;
 *                  E(tau) = sum_{j=tau}^{tau+W-1} f[j]^2 ;  r(tau) = sum_{j<W} f[j] f[j+tau].
 *     Normalised.  d'(0) = 1 ;  c(tau) = sum_{k=1}^{tau} d(k) ;  d'(tau) = d(tau) tau / c(tau) where c(tau) > 0, else 1.
 *     Pick.        tau0 = the smallest tau in [tau_min, tau_max] with d'(tau) < threshold.  If it exists, tau* = tau0 advanced while
 *                  tau* + 1 <= tau_max and d'(tau* + 1) < d'(tau*) ; if not, tau* = the first arg-min of d' over the range.
 *     Refinement.  a, b, c = d'(tau* - 1), d'(tau*), d'(tau* + 1), q = a - 2 b + c ;  s = (a - c) / (2 q) if q > 0 and |a - c| < q,
 *                  else 0 ;  period_out = tau* + s, aper_out = b, tau_out = tau*, cmnd_out = d'(0 ... W).  b < threshold is exactly
 *                  the condition that tau0 existed (a voiced frame).
 * r goes through a float32 FFT (two complex transforms of length N per frame; the lags 1 ... 8 take d from the literal sum in
 * float64 instead); E, d and c are float64; d' is rounded once to float32 and the pick runs on those values, the ones cmnd_out
 * receives, against the float64 threshold; the refinement is float64 from the three float32 values, rounded once.  A silent frame
 * is d' = 1 throughout, tau* = tau_min and unvoiced.  With cmnd_out given the pick still runs.  Any batch: it is not a launch
 * dimension of its own.  NaN input is unspecified.  Stateless: a running method is not disturbed.
 * Before the device is touched, in this order: SPECINV_EINVAL for a NULL x, period_out or aper_out ; an output that is x or another
 * output ; batch < 1 ; an unknown dtype ; then SPECINV_EUNSUPPORTED for SPECINV_F64 ; a frame that is not 256, 512, 1024 or 2048 ;
 * then SPECINV_EINVAL for hop outside 1 ... frame ; a length that gives no frame (length < 1, or length < frame with center == 0) ;
 * tau_min < 1, tau_max > frame / 2 - 1 or tau_min >= tau_max ; a threshold that is not finite and > 0. */
int specinv_yin(const void* x, void* period_out, void* aper_out, void* tau_out, void* cmnd_out, int64_t batch, int64_t length,
                int32_t frame, int32_t hop, int32_t center, int32_t tau_min, int32_t tau_max, double threshold, int32_t dtype,
                int32_t device, void* hip_stream);
/* Probabilistic YIN (not in the reference; csrc/kernels_pyin.h; Mauch & Dixon 2014) on the d' that specinv_yin writes to cmnd_out:
 * two stateless launches on HIP device `device`, enqueued on hip_stream (NULL: the null stream).  tiny = DBL_MIN.
 * specinv_pyin_obs: cmnd (frames, W + 1) float32, W = frame / 2 -> obs_out (frames, n_bins) float32 and vprob_out (frames,) float32.
 * `tables` is one float64 device array: s_k (K = n_thresholds entries), w_k (K), cum[0 ... K] with cum[m] = w_1 + ... + w_m,
 * boltz[r] = (1 - e^-lambda) e^(-lambda r) (n_ranks entries), inv[n] = 1 / (1 - e^(-lambda n)) (n_ranks + 1 entries, inv[0] unused).
 *     Troughs.     tau in [tau_min, tau_max] with d'(tau) < d'(tau - 1) and d'(tau) <= d'(tau + 1), compared in float32.
 *     Candidates.  For k = 1 ... K in rising order: the n troughs with d'(tau) < s_k (float64), ranked r = 0 ... n - 1 by rising lag,
 *                  take p(tau) += (w_k inv[n]) boltz[r].  The first arg-min trough then takes no_trough_prob cum[m], m the number
 *                  of k with d'(tau) >= s_k.  Float64, not contracted.
 *     Bins.        A trough with p > 0: period = tau + shift (specinv_yin's refinement), bin = rint(12 bins_per_semitone
 *                  log2(sample_rate / period / fmin)); below 0 it is bin 0, above n_bins - 1 it is dropped; of several in one bin
 *                  the largest lag stands.  obs_out[bin] = (float) p, every other entry 0; vprob_out = clip(sum of the standing p, 0, 1).
 * Before the device is touched, in this order: SPECINV_EINVAL for a NULL cmnd, tables, obs_out or vprob_out ; an output that is an
 * input or the other output ; frames < 1 ; an unknown dtype ; then SPECINV_EUNSUPPORTED for SPECINV_F64 ; a frame that is not 256,
 * 512, 1024 or 2048 ; n_bins outside 1 ... 1024 ; n_thresholds outside 1 ... 1024 ; then SPECINV_EINVAL for tau_min < 1, tau_max >
 * frame / 2 - 1 or tau_min >= tau_max ; n_ranks < (tau_max - tau_min) / 2 + 1, the troughs a range can hold ; bins_per_semitone < 1 ;
 * sample_rate or fmin not finite and > 0 ; no_trough_prob outside 0 ... 1. */
int specinv_pyin_obs(const void* cmnd, const void* tables, void* obs_out, void* vprob_out, int64_t frames, int32_t frame,
                     int32_t tau_min, int32_t tau_max, int32_t n_thresholds, int32_t n_ranks, int32_t n_bins, int32_t bins_per_semitone,
                     double sample_rate, double fmin, double no_trough_prob, int32_t dtype, int32_t device, void* hip_stream);
/* specinv_pyin_viterbi: obs (batch, n_frames, P) float32 and vprob (batch, n_frames) float32, P = n_bins -> states_out (batch,
 * n_frames) int32, the Viterbi path of the 2 P-state model, one workgroup per item.  State j < P is voiced bin j, P + j unvoiced bin j.
 * `tables` is one float64 device array: log tri(k), k = 0 ... half_width, then -log Z_i, i < P, with tri(k) = 1 - |k| / (half_width + 1)
 * and Z_i the sum of tri(j - i) over |j - i| <= half_width, 0 <= j < P.  backptr is scratch, (batch, n_frames, 2 P) int16.
 *     log B_t[j] = log(obs[t][j] + tiny) voiced, log((1 - vprob[t]) / P + tiny) unvoiced ;  init = 0 voiced, 1 / P unvoiced ;
 *     A = [[1 - s, s], [s, 1 - s]] (x) tri(j - i) / Z_i inside |j - i| <= half_width, 0 outside, s = switch_prob ;
 *     delta_0 = log(init + tiny) + log B_0 ;  delta_t[j] = max_i(delta_{t-1}[i] + log(A[i][j] + tiny)) + log B_t[j], the lowest i on
 *     ties ;  the last frame's arg-max, the lowest index on ties, is walked back.  Float64.  In the band log A is the sum of the
 *     tables' terms and log(1 - s) or log s; outside it is log tiny, offered by each group's maximum.
 * ticks_out is NULL or (batch, 3) int64: the 100 MHz wall clock at an item's start, before the walk back and at its end (a
 * measuring aid).  Any batch.  Before the device is touched, in this order: SPECINV_EINVAL for a NULL obs, vprob, tables, backptr
 * or states_out ; backptr, states_out or ticks_out equal to an earlier argument ; batch or n_frames < 1 ; an unknown dtype ; then
 * SPECINV_EUNSUPPORTED for SPECINV_F64 ; n_bins outside 1 ... 1024 ; half_width outside 0 ... 512 ; then SPECINV_EINVAL for a
 * switch_prob outside (0, 1). */
int specinv_pyin_viterbi(const void* obs, const void* vprob, const void* tables, void* backptr, void* states_out, void* ticks_out,
                         int64_t batch, int64_t n_frames, int32_t n_bins, int32_t half_width, double switch_prob, int32_t dtype,
                         int32_t device, void* hip_stream);
/* Single-channel speech enhancement (not in the reference; csrc/kernels_enhance.h): the noise-power tracker of Gerkmann & Hendriks
 * 2012, the decision-directed a-priori SNR and the Wiener or log-spectral-amplitude gain of Ephraim & Malah 1984 / 1985, one
 * stateless launch on HIP device `device`, enqueued on hip_stream (NULL: the null stream).  spec is (batch, n_freq, n_frames), or
 * (batch, n_frames, n_freq) with frame_major != 0, real magnitudes or (is_complex != 0) interleaved complex values of `dtype`.
 * Outputs, each NULL or a device array: noise_out (sigma^2), spp_out (p), gain_out (G), snr_out (xi), real, of `dtype`, in spec's
 * layout; enhanced_out (G spec), of spec's type and layout; state_out (batch, n_freq, 3) float64, the last frame's sigma^2, Pbar,
 * A^2 in either layout.  state_in is NULL or such an array: it replaces the start rules.  noise_mode SPECINV_ENHANCE_TRACK runs the
 * tracker (noise NULL); SPECINV_ENHANCE_NOISE_FULL reads sigma^2 from `noise`, real, of `dtype`, in spec's layout;
 * SPECINV_ENHANCE_NOISE_PROFILE from `noise` (batch, n_freq), one value per chain.  Per item and bin, frames l = 0 ... T - 1, in
 * float64 whatever `dtype`, products and sums not contracted; P_l = re^2 + im^2 or m^2; tiny = 1e-300; q(a) = min(a / max(sigma^2,
 * tiny), 1e300); xi1 = prior_snr, c = xi1 / (1 + xi1):
 *     Start.    state_in NULL: sigma^2_{-1} = the mean of P_l over the first min(init_frames, T) frames, summed in frame order;
 *               Pbar_{-1} = 0; the first term of xi_0 is alpha.
 *     Tracker.  g' = q(P_l) on sigma^2_{l-1} ;  p = 1 / (1 + (1 + xi1) exp(-(g' c))) ;  Pbar_l = alpha_spp Pbar_{l-1} + (1 - alpha_spp) p ;
 *               if Pbar_l > 0.99: p = min(p, 0.99) ;  sigma^2_l = alpha_pow sigma^2_{l-1} + (1 - alpha_pow) ((1 - p) P_l + p sigma^2_{l-1}).
 *     Gain.     g = q(P_l), r = q(A^2_{l-1}) on sigma^2_l ;  xi_l = max(alpha r + (1 - alpha) max(g - 1, 0), xi_min) ;  w = xi_l / (1 + xi_l) ;
 *               SPECINV_ENHANCE_WIENER: G = w ;  SPECINV_ENHANCE_LSA: G = w exp(E1(max(w g, 1e-12)) / 2) ;
 *               G_l = min(max(G, gain_min), 1) ;  A^2_l = G_l^2 P_l.
 * E1 is the exponential integral, evaluated to a relative error below 1e-13 on [1e-12, 700] and as 0 beyond.  prior_snr, xi_min
 * and gain_min are plain ratios, not decibels.  One call on T frames and two calls chained through the state give the same bits.
 * Any batch, n_freq and n_frames: none is a launch dimension of its own.  NaN input is unspecified.  A running method is not disturbed.
 * Before the device is touched, in this order: SPECINV_EINVAL for a NULL spec ; every output NULL ; an unknown noise_mode ; noise
 * given with SPECINV_ENHANCE_TRACK or NULL without ; noise given with noise_out or spp_out ; a pointer equal to an earlier
 * argument ; batch, n_freq or n_frames < 1 ; more than 2^58 elements ; init_frames < 1 ; an unknown dtype ; an unknown rule ;
 * alpha_pow, alpha_spp or alpha outside 0 ... 1 ; prior_snr or xi_min not finite and > 0 ; gain_min outside (0, 1]. */
enum { SPECINV_ENHANCE_WIENER = 0, SPECINV_ENHANCE_LSA = 1 };
enum { SPECINV_ENHANCE_TRACK = 0, SPECINV_ENHANCE_NOISE_FULL = 1, SPECINV_ENHANCE_NOISE_PROFILE = 2 };
int specinv_enhance(const void* spec, const void* noise, const void* state_in, void* noise_out, void* spp_out, void* gain_out,
                    void* snr_out, void* enhanced_out, void* state_out, int64_t batch, int64_t n_freq, int64_t n_frames,
                    int32_t init_frames, int32_t noise_mode, int32_t rule, double alpha_pow, double alpha_spp, double prior_snr,
                    double alpha, double xi_min, double gain_min, int32_t is_complex, int32_t frame_major, int32_t dtype,
                    int32_t device, void* hip_stream);
/* Weighted prediction error dereverberation (not in the reference; csrc/kernels_wpe.h; Nakatani et al. 2010, the offline form),
 * one stateless launch for all iterations on HIP device `device`, enqueued on hip_stream (NULL: the null stream).  spec and out
 * are (batch, channels, n_freq, n_frames) interleaved complex values of `dtype`.  Per item and bin f, with K = taps, D = channels K,
 * x_t = spec[:, f, t] and the stacked past xs_t in C^D, entry (c', k) at row c' K + k = spec[c', f, t - delay - k], zero before frame 0:
 *     q_t   = mean_c |Y[c, f, t]|^2, Y the previous iteration's result in float64 (never a rounded copy), spec itself in the
 *             first; or power[f, t] in the first when `power` (batch, n_freq, n_frames) float64 is given
 *     p_t   = the mean of q over the frames t - psd_context ... t + psd_context that exist
 *     lam_t = max(p_t, eps max_t p_t, tiny), tiny = the smallest normal double
 *     R = sum_t xs_t xs_t^H / lam_t ;  P = sum_t xs_t x_t^H / lam_t ;  R += (diag_load tr(R) / D + tiny) I ;  G = R^-1 P
 *     Y[:, f, t] = x_t - G^H xs_t
 * repeated n_iter times; out = Y rounded once to `dtype`.  All sums, the factorisation (U D U^H, pivots floored at tiny) and the
 * solve are float64.  n_iter = 0 gives G = 0 and out = spec.  A silent bin gives G = 0 and out = 0; nothing is NaN for finite input.
 * filt_out is NULL or (batch, n_freq, D, channels) complex float64: G, entry [c' K + k][c] the weight of channel c' at lag delay + k
 * in the prediction of channel c.  lam (batch, n_freq, n_frames) float64 receives the last lam and is the estimate's work array:
 * never NULL when estimating.  scratch is a second such array, needed when psd_context > 0.
 * Filter-only mode: filt_in, an array like filt_out, is given; nothing is estimated and out = spec - G^H xs, by the same
 * instructions as the estimating call's last pass (the same bits when G came from it); power, filt_out and lam must be NULL.
 * Any batch, n_freq, n_frames and delay; n_iter <= 100 and psd_context <= 64 (the context mean is 2 psd_context + 1 reads a frame:
 * the launch's length stays bounded); an item's result does not depend on the batch around it.
 * Before the device is touched, in this order: SPECINV_EINVAL for a NULL spec or out ; filt_in given with power, filt_out or lam ;
 * lam NULL without filt_in ; psd_context > 0 without scratch (and without filt_in) ; out, filt_out, lam or scratch equal to an
 * earlier argument ; batch, channels, n_freq or n_frames < 1 ; more than 2^51 elements a channel ; taps < 1 ; delay < 1 ; n_iter or
 * psd_context < 0 ; eps or diag_load negative or not finite ; an unknown dtype ; then SPECINV_EUNSUPPORTED for channels taps > 64 ;
 * n_iter > 100 or psd_context > 64. */
int specinv_wpe(const void* spec, const void* power, const void* filt_in, void* out, void* filt_out, void* lam, void* scratch,
                int64_t batch, int32_t channels, int64_t n_freq, int64_t n_frames, int32_t taps, int64_t delay, int32_t n_iter,
                int64_t psd_context, double eps, double diag_load, int32_t dtype, int32_t device, void* hip_stream);
/* Mask-based beamforming (not in the reference; csrc/kernels_beamform.h), one stateless launch on HIP device `device`, enqueued on
 * hip_stream (NULL: the null stream).  spec is (batch, channels, n_freq, n_frames) interleaved complex values of `dtype`, out
 * (batch, n_freq, n_frames) of the same.  Per item and bin f, with C = channels, x_t = spec[:, f, t], m = mask_target[f, t] (1 when
 * NULL), n = mask_noise[f, t] (1 - m when NULL), both (batch, n_freq, n_frames) float64 and non-negative:
 *     Phi(m)  = sum_t m_t x_t x_t^H / max(sum_t m_t, tiny), tiny = the smallest normal double ;  Phi_s = Phi(m), Phi_n = Phi(n)
 *     load(A) = A + (diag_load Re tr(A) / C + tiny) I
 *     SOUDEN:     A = load(Phi_n) ;  N = A^-1 Phi_s ;  w = N[:, ref_channel] / max(Re tr(N), tiny)
 *     RTF_POWER:  A, N as above ;  v = N[:, ref_channel] ;  n_power_iter - 1 times v <- N (v / max(|Re v|_inf, |Im v|_inf, tiny)) ;
 *                 a = A v ;  w = v conj(a[ref_channel]) / max(Re(a^H v), tiny)
 *     MWF:        A = load(Phi_s + mu Phi_n) ;  w = A^-1 Phi_s[:, ref_channel]
 *     out[f, t] = w^H x_t, rounded once to `dtype`
 * All sums, the factorisation (U D U^H, pivots floored at tiny) and the solves are float64.  A silent bin or an all-zero mask gives
 * Phi = 0, w = 0 and out = 0; nothing is NaN for finite input.  scm_target / scm_noise are NULL or (batch, n_freq, C, C) complex
 * float64 and receive Phi_s / Phi_n before the loading, exactly Hermitian.  weights_out is NULL or (batch, n_freq, C) complex float64: w.
 * Covariance-only mode: out and weights_out NULL; only the sums run (mask_target may then be NULL: all ones).
 * Filter-only mode: weights_in, an array like weights_out, is given; nothing is estimated and out = w^H x by the same instructions
 * as the estimating call's (the same bits when w came from it); the masks, weights_out and the covariances must be NULL.
 * Any batch, n_freq and n_frames; an item's result does not depend on the batch around it or on the mode.
 * Before the device is touched, in this order: SPECINV_EINVAL for a NULL spec ; weights_in given without out or with a mask,
 * weights_out or a covariance ; no result asked for ; out or weights_out without mask_target (and without weights_in) ; out,
 * weights_out, scm_target or scm_noise equal to an earlier argument ; batch, channels, n_freq or n_frames < 1 ; more than 2^51
 * elements a channel ; an unknown solution ; ref_channel outside [0, channels) ; n_power_iter < 1 ; diag_load or mu negative or not
 * finite ; an unknown dtype ; then SPECINV_EUNSUPPORTED for channels > 16 ; n_power_iter > 64. */
enum { SPECINV_BEAMFORM_SOUDEN = 0, SPECINV_BEAMFORM_RTF_POWER = 1, SPECINV_BEAMFORM_MWF = 2 };
int specinv_beamform(const void* spec, const void* mask_target, const void* mask_noise, const void* weights_in, void* out,
                     void* weights_out, void* scm_target, void* scm_noise, int64_t batch, int32_t channels, int64_t n_freq,
                     int64_t n_frames, int32_t solution, int32_t ref_channel, int32_t n_power_iter, double diag_load, double mu,
                     int32_t dtype, int32_t device, void* hip_stream);
/* Time-domain time-scale modification (not in the reference; csrc/kernels_wsola.h): waveform-similarity overlap-add, and plain
 * overlap-add at tol = 0.  x (batch, n_in) -> y (batch, n_out) and lags (batch, n_frames) int32, device arrays on HIP device
 * `device`, x, window (frame entries) and y of `dtype`, enqueued on hip_stream (NULL: the null stream).  No plan: nothing is kept
 * between calls.  With N = frame (even, 2 ... 2048), Hs = hop (the synthesis hop, 1 ... N), D = tol (0 ... 1024), w = window and
 * xz(i) = x[i] for 0 <= i < n_in, else 0:
 *     Frames.  M = n_frames = (n_out - 1 + N/2) / Hs + 1, exactly the frames whose support [m Hs - N/2, m Hs + N/2) meets [0, n_out).
 *     Analysis centres.  a_m = centres[m], m < M: any non-decreasing int64 array (for a fixed rate the caller makes
 *       floor(m Hs rate + 0.5) once in float64; the kernels never evaluate that expression).
 *     Lag chain.  del_0 = 0; for m = 0 ... M - 2, with u_m = a_m + del_m - N/2:
 *       p[n]      = xz(u_m + Hs + n), n < N                            (the natural continuation of frame m)
 *       c[d]      = sum_n xz(a_{m+1} - N/2 + d + n) p[n], |d| <= D     (float64 products and sums for both dtypes)
 *       del_{m+1} = the d with the largest c[d]; among equals the smallest |d|; of +-d the negative one
 *     Overlap-add.  For 0 <= j < n_out, over the frames m in [0, M) with 0 <= n = j - m Hs + N/2 < N, in ascending m, in float64:
 *       acc[j] = sum_m w[n] xz(u_m + n) ;  ow[j] = sum_m w[n] ;  y[j] = acc[j] / (ow[j] >= 1e-3 ? ow[j] : 1), rounded once.
 * lags = del is always written, as zeros when tol == 0; the chain is not run when tol == 0 or n_frames == 1.  ow does not depend
 * on the data.  Every read is guarded against [0, n_in): no centre and no lag can read outside a row.  Any batch: it is not a
 * launch dimension of its own.  NaN input is unspecified.  Stateless: a running method is not disturbed.
 * SPECINV_EINVAL, before the device is touched, in this order: a NULL pointer (x, centres, window, lags, y) ; y == x ; batch, n_in
 * or n_out < 1 ; frame odd or outside 2 ... 2048 ; hop outside 1 ... frame ; tol outside 0 ... 1024 ;
 * n_frames != (n_out - 1 + frame / 2) / hop + 1 ; an unknown dtype. */
int specinv_wsola(const void* x, const int64_t* centres, const void* window, int32_t* lags, void* y, int64_t batch, int64_t n_in,
                  int64_t n_out, int32_t n_frames, int32_t frame, int32_t hop, int32_t tol, int32_t dtype, int32_t device,
                  void* hip_stream);
/* Phase gradient heap integration in its real-time form with one look-ahead frame (RTPGHI, Prusa & Sondergaard 2016; not in the
 * reference; csrc/kernels_pghi.h): a phase for magnitudes alone, in one launch.  mag (batch, n_freq, n_frames) real and non-negative
 * -> spec_out (batch, n_freq, n_frames) complex = mag exp(i phi), interleaved (re, im) of `dtype`; optionally phase_out, the unwrapped
 * float64 phi, and parents_out, int8 codes; device arrays on HIP device `device`, enqueued on hip_stream (NULL: the null stream).  No
 * plan: nothing is kept between calls.  Per item, with N = n_fft, a = hop, F = n_freq = N/2 + 1, T = n_frames, s[m,n] the
 * magnitudes, g = gamma, all arithmetic float64 for both dtypes:
 *     floor = tol * max(0, max s) ; (m,n) is live iff s > 0 and s >= floor ; l[m,n] = log(max(s, floor)), mirrored in frequency:
 *       l[-1] = l[1], l[F] = l[F-2].  An item whose maximum is 0 has no live bin.
 *     wt[m,n] = (2 pi / N) ((a m) mod N) + (a N / g) ((l[m+1,n] - l[m-1,n]) / 2)       (a m reduced as an integer)
 *     wf[m,n] = pi - (g / (a N)) D[m,n] ;  D = (l[m,n+1] - l[m,n-1]) / 2 for 0 < n < T-1, l[m,1] - l[m,0] at n = 0,
 *       l[m,T-1] - l[m,T-2] at n = T-1, 0 for T = 1      (the pi: frames start at sample 0, the window centre sits at N/2)
 *     Frame n given frame n-1:  c[m] = s[m,n] if live else -inf ; p[m] = s[m,n-1] if (m,n-1) is live else -inf ; for n = 0 every
 *       p[m] = -inf but for the lowest-index maximum of s[:,0], which has p = +inf if it is live.
 *       Lf[0] = -inf, Lf[m] = min(c[m-1], max(p[m-1], Lf[m-1])) ;  Rg[F-1] = -inf, Rg[m] = min(c[m+1], max(p[m+1], Rg[m+1]))
 *       Parent of a live bin, b = max(p[m], Lf[m], Rg[m]):  code 0 if p[m] >= b (time wins ties, and when all three are -inf),
 *       else code 1 if Lf[m] >= b, else code 2 ; a bin that is not live has code 3.
 *     phi:  code 0: phi[m,n-1] + (wt[m,n-1] + wt[m,n]) / 2, in frame 0 exactly 0 ;  code 1: phi[m-1,n] + (wf[m-1,n] + wf[m,n]) / 2 ;
 *       code 2: phi[m+1,n] - (wf[m+1,n] + wf[m,n]) / 2 ;  code 3: 0, and that 0 is what a later time step reads.
 *     spec_out = (s cos phi, s sin phi), evaluated in float64 and rounded once.
 * This is the heap of RTPGHI (the heap holds frame n-1 with keys p, a popped bin sets its unset neighbours and pushes them with
 * key c): a bin is set by the candidate with the widest max-min path, and min(c, max(p, .)) composes associatively.  Every decision
 * compares input values exactly.  n_fft is even, 2 ... 5828 (SPECINV_EUNSUPPORTED above: the frame's state no longer fits a compute
 * unit's LDS); any batch, it is not a launch dimension of its own.  NaN input is unspecified.  Stateless: a running method is not
 * disturbed.  SPECINV_EINVAL, before the device is touched, in this order: NULL mag or spec_out ; spec_out == mag ; batch, n_freq or
 * n_frames < 1 ; n_fft < 2 or odd, or n_freq != n_fft / 2 + 1 ; hop < 1 ; gamma not finite and positive ; tol outside (0, 1) ; an
 * unknown dtype. */
int specinv_pghi(const void* mag, void* spec_out, double* phase_out, int8_t* parents_out, int64_t batch, int32_t n_freq,
                 int32_t n_frames, int32_t n_fft, int32_t hop, double gamma, double tol, int32_t dtype, int32_t device,
                 void* hip_stream);
/* The phase vocoder with heap-integrated phase (Prusa & Holighaus 2017, "phase vocoder done right", in specinv_phase_vocoder's
 * frame-resampling form; not in the reference; csrc/kernels_pvoc_pghi.h), in one launch.  spec_in (batch, n_freq,
 * n_frames_in) complex, one-sided, -> spec_out (batch, n_freq, n_frames_out) complex, interleaved (re, im) of `dtype`; optionally
 * parents_out, int8 codes of spec_out's shape; device arrays on HIP device `device`, enqueued on hip_stream (NULL: the null stream).
 * No plan: nothing is kept between calls.  Per item, with t_j = (double)j * rate, i = floor(t_j), a = t_j - i, S0 = S[i],
 * S1 = S[i+1] (frames at and beyond n_frames_in are +0 + 0i), adv = 2 pi k hop / n_fft, wrap(x) = x - 2 pi round(x / 2 pi),
 * d_j = wrap(arg S1 - arg S0 - adv) + adv as for specinv_phase_vocoder; theta0 = arg S0 and theta1 = arg S1 are taken in `dtype`
 * and widened, everything after them is float64 for both dtypes with no contraction:
 *     q(z) = re re + im im from the input's own bits ;  r(z) = sqrt(q(z)) ;  m_j[k] = fl(fl(a r(S1[k])) + fl(fl(1 - a) r(S0[k])))
 *     floor = tol * sqrt(max q over the item's input) ;  (j,k) is live iff m_j[k] > 0 and m_j[k] >= floor
 *     Frame 0:  psi_0 = theta0 ;  code 0 where live, 3 elsewhere.
 *     Frame j >= 1:  c[k] = m_j[k] if live else -inf ;  p[k] = m_{j-1}[k] if (j-1,k) is live else -inf ;
 *       Lf[0] = -inf, Lf[k] = min(c[k-1], max(p[k-1], Lf[k-1])) ;  Rg[F-1] = -inf, Rg[k] = min(c[k+1], max(p[k+1], Rg[k+1]))
 *       Parent of a live bin, b = max(p[k], Lf[k], Rg[k]):  code 0 if p[k] >= b (time wins ties, and when all three are -inf),
 *       else code 1 if Lf[k] >= b, else code 2 ; a bin that is not live has code 3.
 *       phi_j[k] = psi_{j-1}[k] + d_{j-1}[k] for every bin, one addition.
 *       root(k) = k for codes 0 and 3 ; root(k+1) for code 2 (resolved first) ; root(k-1) for code 1.
 *       psi_j[k] = phi_j[k] if root(k) = k, else (phi_j[root] - theta0_j[root]) + theta0_j[k], in that association.
 *     spec_out[j][k] = (m cos psi, m sin psi), evaluated in float64 and rounded once.
 * This is the per-frame heap of RTPGHI (specinv_pghi) with the analysis phase differences as the gradients: the frequency steps
 * along a chain telescope to theta0[k] - theta0[root].  A bin that is not live keeps its own time-propagated phase and is never a
 * parent; a silent item gives exact zeros.  |spec_out| may differ from specinv_phase_vocoder's by one rounding (that entry forms |z|
 * with fma and hypot).  n_freq <= 2915 (SPECINV_EUNSUPPORTED above); any batch, it is not a launch dimension of its own.  float64
 * input whose q over- or underflows (|z| beyond about 1e150 or below 1e-150) and NaN input are unspecified.  Stateless: a running
 * method is not disturbed.  SPECINV_EINVAL, before the device is touched, in this order: NULL spec_in or spec_out ; spec_out ==
 * spec_in ; batch, n_freq, n_frames_in, n_frames_out or n_fft < 1 ; n_freq != n_fft / 2 + 1 ; hop < 1 ; rate not finite and
 * positive ; n_frames_out != the smallest n >= 1 with (double)n * rate >= n_frames_in ; tol outside (0, 1) ; an unknown dtype. */
int specinv_pvoc_pghi(const void* spec_in, void* spec_out, int8_t* parents_out, int64_t batch, int32_t n_freq, int32_t n_frames_in,
                      int32_t n_frames_out, int32_t n_fft, int32_t hop, double rate, double tol, int32_t dtype, int32_t device,
                      void* hip_stream);
/* Consistent Wiener filtering (Le Roux & Vincent, IEEE SPL 2013; not in the reference; csrc/kernels_cwf.h): the
 * whole loop on the plan's stream.  mix, S_out, N_out are (batch, n_freq, n_frames) complex as specinv_stft writes them; var_s,
 * var_n are (batch, n_freq, n_frames) real and >= 0, all device arrays of the plan's dtype at 16-byte aligned addresses.  Per
 * item, with X = mix, v_s = var_s, v_n = var_n, a = hop_length, N = n_fft; every scalar and sum is float64 for both dtypes, the
 * arrays are held in the plan's dtype:
 *     m = floor * max(v_s + v_n) ; m == 0: the item's S is 0 and it takes no part ; v_s, v_n <- max(v_s, m), max(v_n, m)
 *     Lam = 1 / v_s + 1 / v_n ;  g = gamma / mean(v_s v_n / (v_s + v_n)) if relative, else gamma
 *     G Z = specinv_stft(specinv_istft(Z)) ;  G' U = specinv_istft_adjoint(specinv_stft_adjoint(U)), the real adjoint of G under
 *       <a, b> = sum Re a Re b + Im a Im b over the item's bins, unweighted
 *     A P = Lam P + g (u - G' u), u = P - G P ;  M = Lam + g (1 - a / N)
 *     S_0 = v_s / (v_s + v_n) X ;  r = X / v_n - A S_0 ;  z = r / M ;  p = z ;  rz = <r, z> ;  rz0 = rz
 *     n_iter times:  q = A p ; alpha = rz / <p, q> ; S += alpha p ; r -= alpha q ; z = r / M ; rz' = <r, z> ; beta = rz' / rz ;
 *       p = z + beta p ; rz = rz'
 *     an item whose rz is 0 or whose <p, q> is not > 0 is finished: alpha = beta = 0 from then on.
 * S_out is the last iterate - preconditioned conjugate gradients on A S = X / v_n, the stationarity condition of
 * sum |X - S|^2 / v_n + |S|^2 / v_s + g |S - G S|^2 - and N_out = X - S_out, formed once at the end; N_out is the loop's scratch
 * until then.  An item's result does not depend on the other items, alpha and beta never visit the host, no atomics: two calls give
 * the same bits.  tol > 0: the residuals sqrt(rz / rz0) (0 for a finished item) are read back after every eva_iter-th iteration and
 * the loop stops when every item's is <= tol; tol == 0: nothing is read back before the end.  residual_out_host (batch doubles, or
 * NULL: no read-back at all) receives the final residuals, *iters_out (or NULL) the iterations run.  Stateless: scratch only (three
 * spectra, Lam and one signal, kept by the plan for the next call), a running method is not disturbed.  SPECINV_EINVAL, before the
 * device is touched, in this order: a NULL array (mix, var_s, var_n, S_out, N_out) ; an output that aliases the other or an input ;
 * an array off a 16-byte boundary ; gamma not finite and positive ; floor outside (0, 1) ; n_iter < 0 ; eva_iter < 1 ; tol < 0 or
 * NaN ; a NULL plan.  SPECINV_EUNSUPPORTED: a two-sided plan. */
int specinv_cwf_run(specinv_plan* plan, const void* mix, const void* var_s, const void* var_n, double gamma, int relative, double floor,
                    int n_iter, int eva_iter, double tol, void* S_out, void* N_out, double* residual_out_host, int* iters_out);
/* metrics.py sums over n elements of two real device arrays of the plan's dtype */
int specinv_metric_sums(specinv_plan* plan, const void* a, const void* b, int64_t n, double sums_host[4]);

/* ---- griffin_lim (methods.py:193-270) -------------------------------------------------- */
/* Setup :223-235.  `init_spec` (B,F,T) complex is the starting spectrogram (cmplx_spec);
 * `mag` (B,F,T) real is target_spec.  If init_spec is NULL the plan runs phase_init(mag). */
int specinv_gla_init(specinv_plan* plan, const void* init_spec, const void* mag, double alpha);
/* n_iter closure calls (:237-250).  If eval_last != 0 the |STFT| of the last call is reduced
 * against the target into sums_host[4] (this synchronises the stream). */
int specinv_gla_iterate(specinv_plan* plan, int n_iter, int eval_last, double sums_host[4]);
/* The whole _training_loop (:153-190) on the device side: evaluation every eva_iter, early
 * stop rule :186-190.  evals_out (may be NULL) receives up to max_iter/eva_iter entries. */
int specinv_gla_run(specinv_plan* plan, int max_iter, int eva_iter, double tol, int metric,
                    specinv_eval* evals_out, int* n_evals_out, int* iters_done_out,
                    specinv_eval_cb cb, void* user);

/* ---- ADMM (methods.py:415-506) --------------------------------------------------------- */
int specinv_admm_init(specinv_plan* plan, const void* init_spec, const void* mag, double rho);
int specinv_admm_iterate(specinv_plan* plan, int n_iter, int eval_last, double sums_host[4]);
/* n_iter iterations of the running method (Griffin-Lim or ADMM), the last one evaluating (methods.py:180-182) - its four sums
 * {sum (|S| - m)^2, sum |S|^2, sum m^2, count} left in DEVICE memory (4 doubles) instead of on the host: nothing waits.  For callers
 * that reduce the sums over several plans / ranks before they look at them (`_training_loop`'s whole-batch metric across GPUs,
 * methods.py:181-190: one all-reduce on the device, one read). */
int specinv_iterate_eval_dev(specinv_plan* plan, int n_iter, void* sums_dev);
int specinv_admm_run(specinv_plan* plan, int max_iter, int eva_iter, double tol, int metric,
                     specinv_eval* evals_out, int* n_evals_out, int* iters_done_out,
                     specinv_eval_cb cb, void* user);

/* ---- MISI (Gunawan & Sen 2010: multiple input spectrogram inversion) -------------------- */
/* MISI: Griffin-Lim without momentum on batch = n_mix * n_src items (item b*n_src + k is source k of mixture b), coupled after
 * every inverse transform by x_k += (mix_b - sum_k x_k) / n_src.  init_spec / mag as specinv_gla_init (init_spec required:
 * the host layer forms the mixture-phase start); mixture (n_mix, mix_stride) device array of the plan's dtype, the first
 * specinv_plan_length samples of each row are used (the plan keeps a copy).  SPECINV_EINVAL, before anything is enqueued: NULL
 * init_spec or mixture, n_src < 1, a batch that is no multiple of n_src, mix_stride below the plan's length. */
int specinv_misi_init(specinv_plan* plan, const void* init_spec, const void* mag, const void* mixture, int64_t mix_stride, int n_src);
/* n_iter times: one projection launch, one coupling launch.  An evaluating iteration's sums are the projection's: |STFT| of the
 * mixed signals that entered it against the target.  SPECINV_ESTATE before specinv_misi_init; specinv_gla_iterate / _run and
 * specinv_admm_iterate / _run return SPECINV_ESTATE on a plan in the MISI state (they would drop the coupling step). */
int specinv_misi_iterate(specinv_plan* plan, int n_iter, int eval_last, double sums_host[4]);
int specinv_misi_run(specinv_plan* plan, int max_iter, int eva_iter, double tol, int metric, specinv_eval* evals_out,
                     int* n_evals_out, int* iters_done_out, specinv_eval_cb cb, void* user);

/* ---- AGLA (Peer, Welker & Gerkmann 2022: accelerated Griffin-Lim) ------------------------ */
/* Accelerated Griffin-Lim.  With P(x) = ISTFT(S m / (|S| + 1e-16)), S = STFT(x) - one Griffin-Lim iteration without momentum -
 * and c_0 = ISTFT(start), iteration 1 sets t_1 = c_1 = d_1 = P(c_0) and iteration n > 1 computes, on signals of
 * specinv_plan_length samples and in the plan's dtype,
 *     y = P(c_{n-1});  t_n = (1 - gamma) d_{n-1} + gamma y;  c_n = t_n + alpha (t_n - t_{n-1});  d_n = t_n + beta (t_n - t_{n-1}).
 * gamma = 1 is Fast Griffin-Lim (Perraudin, Balazs & Soendergaard 2013, the method of librosa and torchaudio): d is then never
 * formed and beta has no effect; alpha = 0, gamma = 1 is Griffin-Lim without momentum.  init_spec / mag as specinv_gla_init
 * (either may be NULL).  SPECINV_EINVAL, before the device is touched: alpha < 0, beta < 0, gamma <= 0, a NULL plan. */
int specinv_agla_init(specinv_plan* plan, const void* init_spec, const void* mag, double alpha, double beta, double gamma);
/* specinv_agla_init with a schedule: iteration n takes entry min(n, n_sched) - 1 of the three host arrays of n_sched doubles (they
 * are copied; iteration 1 does not extrapolate, entry 0 has no effect).  Each entry is rounded to the plan's dtype once; d exists
 * iff some gamma entry != 1.  specinv_agla_init is the case n_sched = 1.  SPECINV_EINVAL, before the device is touched: n_sched < 1,
 * a NULL array, an alpha or beta entry < 0, a gamma entry <= 0, a NULL plan. */
int specinv_agla_init_sched(specinv_plan* plan, const void* init_spec, const void* mag, int n_sched, const double* alpha,
                            const double* beta, const double* gamma);
/* Known bins and known samples for the iterations that follow (constrained_griffin_lim; csrc/kernels_agla.h).  With M the mask of
 * known bins and K their values, the host layer passes mag = where(M, 0, m) to specinv_agla_init and here
 *     offset = where(W, xk, ISTFT(where(M, K, 0))),  (batch, length) in the plan's dtype,
 *     fixed_mask = W, (batch, length) uint8, non-zero where the sample xk is known - or NULL: no sample is.
 * Both are device arrays; the plan keeps copies (device_bytes grows by batch * length * (sizeof(T) [+ 1])).  Every iteration then
 * runs the constrained form of k_agla_step:  u = y + offset;  t_n = where(W, offset, (1 - gamma) d_{n-1} + gamma u);  c_n and d_n as above;
 * t, c and d hold xk bit for bit under W.  Both NULL clears the constraint, and so does every specinv_*_init.  An evaluating
 * iteration's sums compare against mag, zeros under M: evaluate |STFT(t_n)| against the full target instead (specinv_stft,
 * specinv_metric_sums).  SPECINV_ESTATE: the plan is not in the AGLA state (call after specinv_agla_init / _init_sched).
 * SPECINV_EINVAL, before anything is enqueued: a NULL offset with a fixed_mask, a NULL plan. */
int specinv_agla_constrain(specinv_plan* plan, const void* offset, const void* fixed_mask);
/* n_iter times: one projection launch, one extrapolation launch (k_agla_step).  An evaluating iteration's sums compare
 * |STFT(c_{n-1})|, the signal that entered the projection, against the target.  SPECINV_ESTATE before specinv_agla_init;
 * specinv_gla_iterate / _run, specinv_admm_iterate / _run and specinv_misi_iterate / _run return SPECINV_ESTATE on a plan in
 * the AGLA state (they would drop the extrapolation), specinv_agla_iterate / _run on a plan in any other state. */
int specinv_agla_iterate(specinv_plan* plan, int n_iter, int eval_last, double sums_host[4]);
int specinv_agla_run(specinv_plan* plan, int max_iter, int eva_iter, double tol, int metric, specinv_eval* evals_out,
                     int* n_evals_out, int* iters_done_out, specinv_eval_cb cb, void* user);

/* current waveform estimate status_dict['x'] (B, L) of the running GLA / ADMM / MISI state.  In the AGLA state: t_n, the
 * method's result (ISTFT(start) before the first iteration) - not the extrapolated c_n the next projection reads */
int specinv_get_wave(specinv_plan* plan, void* x_out);
/* running state as (B, F, T) complex: which = 0 pre_spec (GLA) or X (ADMM), 1 U (ADMM), 2 Y = X + U (ADMM, always
 * available; X and U need specinv_plan_keep_state) - for state-parity tests */
int specinv_get_state_spec(specinv_plan* plan, int which, void* spec_out);

/* ---- differentiating griffin_lim w.r.t. the spectrogram (the reference's outputs are autograd-differentiable:
 * test/test_griffin.py:54,65-66).  Element-wise pieces work on (B, F, T) arrays; "g*" are cotangents. ---------- */
/* one closure call without the transforms, methods.py:243-247: S = R - lr*P ; Q = S*mag/(|S| + 1e-16) */
int specinv_gla_update(specinv_plan* plan, const void* R, const void* P, const void* mag, double lr, void* S_out,
                       void* Q_out);
/* its adjoint: gR = gS, gP = -lr*gS, gmag += d/dmag, with gS = proj^T(gQ) + gP_next (gP_next may be NULL) */
int specinv_gla_update_adjoint(specinv_plan* plan, const void* gQ, const void* gP_next, const void* S, const void* mag,
                               double lr, void* gR_out, void* gP_out, void* gmag_accum);
/* one ADMM closure call without the transforms, methods.py:467-475 (V is the pre-projection value Z - U', kept for
 * the adjoint; Yn = X' + U' feeds the ISTFT) and its adjoint (gXn / gUn may be NULL) */
int specinv_admm_update(specinv_plan* plan, const void* R, const void* X, const void* U, const void* mag, double rho,
                        void* Xn_out, void* Un_out, void* V_out, void* Yn_out);
int specinv_admm_update_adjoint(specinv_plan* plan, const void* gYn, const void* gXn, const void* gUn, const void* V,
                                const void* mag, double rho, void* gR_out, void* gX_out, void* gU_out, void* gmag_accum);
/* adjoint of specinv_istft: cotangent of x (B, L) -> cotangent of the spectrogram (B, F, T) complex */
int specinv_istft_adjoint(specinv_plan* plan, const void* g_x, void* g_spec_out);
/* adjoint of specinv_stft: cotangent of the spectrogram -> cotangent of x (B, length) */
int specinv_stft_adjoint(specinv_plan* plan, const void* g_spec, int64_t length, void* g_x_out);
/* ---- MISI's backward sweep (misi_unfolded; csrc/kernels_misi_adjoint.h) ------------------- */
/* Both calls are stateless: they work on a plan in any method state, write only scratch buffers and leave a running method's
 * state as it is.  batch = n_mix * n_src items, item b * n_src + k source k of mixture b (specinv_misi_init).  SPECINV_EINVAL,
 * before anything is enqueued: a NULL pointer, n_src < 1, a batch that is no multiple of n_src. */
/* adjoint of the coupling step x_k += (mix - sum_j x_j) / n_src: g_inout (batch, length) holds the cotangents of the coupled
 * signals and receives g_k - c, c = (1 / n_src) sum_k g_k; c is added to gmix_accum (n_mix, length). */
int specinv_misi_mix_adjoint(specinv_plan* plan, int n_src, void* g_inout, void* gmix_accum);
/* adjoint of one MISI iteration x_n = mix_step(ISTFT(mag * S / (|S| + 1e-16))), S = STFT(x_prev): g_inout (batch, length) holds
 * the cotangent of x_n and receives that of x_prev (batch, length); gmix_accum (n_mix, length) and gmag_fm_accum accumulate the
 * mixture's and the magnitude's.  mag_fm and gmag_fm_accum are frame-major, (batch, n_frames, n_freq): the transposes of the
 * caller-layout arrays, made once per sweep and not once per iteration.  S is recomputed from x_prev. */
int specinv_misi_step_adjoint(specinv_plan* plan, int n_src, const void* x_prev, const void* mag_fm, void* g_inout,
                              void* gmix_accum, void* gmag_fm_accum);
/* the backward sweep of agla_unfolded (csrc/kernels_agla_adjoint.h), one call per iteration n = N ... 2, then the closing call.
 * Stateless as the MISI entries above.  All signals are (batch, length) in the plan's dtype.  The sweep's state: a_inout, the
 * cotangent of t_n (complete); gc_inout and gd_inout, those of c_n and d_n (gd_inout NULL: the form for schedules whose every gamma
 * is 1, where it is identically 0; gamma_n must then be 1).  t_n, t_nm1, t_nm2 are the recorded results of iterations n, n - 1,
 * n - 2 (t_nm2 NULL: n = 2).  coef (host) = {alpha_n, beta_n, gamma_n, alpha_{n-1}, beta_{n-1}}, each rounded to the plan's dtype
 * once; the last two are not read for n = 2.  With s = a + (1 + alpha_n) gc + (1 + beta_n) gd and delta = t_n - t_nm1:
 *   dots_dev_out (3 doubles on the device) = {<gc, delta>, <gd, delta>, <s, t_n - d_{n-1}> / gamma_n}, the gradients of alpha_n,
 *     beta_n, gamma_n, summed over all batch * length samples in double, in a fixed order (no atomics; nothing is read back);
 *   a <- -alpha_n gc - beta_n gd ;  gd <- (1 - gamma_n) s ;  gc <- gamma_n s / envelope ;
 *   c_prev_out <- c_{n-1} = t_nm1 + alpha_{n-1} (t_nm1 - t_nm2) (n = 2: t_nm1); d_{n-1} is formed likewise with beta_{n-1}.
 * SPECINV_EINVAL before anything is enqueued: a NULL pointer other than t_nm2 / gd_inout, alpha or beta < 0, gamma <= 0, gamma_n != 1
 * without gd_inout. */
int specinv_agla_extrap_adjoint(specinv_plan* plan, const void* t_n, const void* t_nm1, const void* t_nm2, const double coef[5],
                                void* a_inout, void* gc_inout, void* gd_inout, void* c_prev_out, void* dots_dev_out);
/* ... followed by the adjoint of the projection of iteration n at c_prev_out (the stages of specinv_misi_step_adjoint after its
 * coupling step): gc_inout receives the cotangent of c_{n-1}, gmag_fm_accum accumulates the magnitude's; mag_fm and gmag_fm_accum are
 * frame-major, (batch, n_frames, n_freq). */
int specinv_agla_step_adjoint(specinv_plan* plan, const void* t_n, const void* t_nm1, const void* t_nm2, const double coef[5],
                              void* a_inout, void* gc_inout, void* gd_inout, void* c_prev_out, void* dots_dev_out,
                              const void* mag_fm, void* gmag_fm_accum);
/* the closing step, iteration 1: t_1 = c_1 = d_1 = P(c_0), c0 = ISTFT(start) as recorded.  gc_inout <- (a + gc + gd) / envelope
 * (gd NULL: absent), then the projection's adjoint at c0: gc_inout receives the cotangent of c0, which specinv_istft_adjoint takes
 * to the start. */
int specinv_agla_first_adjoint(specinv_plan* plan, const void* c0, const void* a, void* gc_inout, const void* gd, const void* mag_fm,
                               void* gmag_fm_accum);
/* the backward sweep of constrained_unfolded (csrc/kernels_agla_adjoint.h): the three entries above under the constraint of
 * specinv_agla_constrain, in their argument order and with their error rules.  fixed_mask is W, (batch, length) uint8, non-zero where
 * the sample is known, or NULL: no sample is.  goff_accum (batch, length) accumulates the cotangent of offset = where(W, xk, k).
 * Iteration n >= 2 is t_n = where(W, offset, (1 - gamma_n) d_{n-1} + gamma_n (P(c_{n-1}) + offset)); with s as above and
 * s' = W ? 0 : s, what passes the select:
 *   dots_dev_out = {<gc, delta>, <gd, delta>, <s', t_n - d_{n-1}> / gamma_n};
 *   goff_accum += W ? s : gamma_n s' ;
 *   a <- -alpha_n gc - beta_n gd ;  gd <- (1 - gamma_n) s' ;  gc <- gamma_n s' / envelope ;  c_prev_out <- c_{n-1}.
 * SPECINV_EINVAL before anything is enqueued: those of specinv_agla_extrap_adjoint, a NULL goff_accum. */
int specinv_cgla_extrap_adjoint(specinv_plan* plan, const void* t_n, const void* t_nm1, const void* t_nm2, const double coef[5],
                                const void* fixed_mask, void* a_inout, void* gc_inout, void* gd_inout, void* goff_accum,
                                void* c_prev_out, void* dots_dev_out);
/* ... followed by the adjoint of the projection of iteration n at c_prev_out; mag_fm is where(M, 0, m) in frame-major layout, made
 * once per sweep, M the mask of known bins. */
int specinv_cgla_step_adjoint(specinv_plan* plan, const void* t_n, const void* t_nm1, const void* t_nm2, const double coef[5],
                              const void* fixed_mask, void* a_inout, void* gc_inout, void* gd_inout, void* goff_accum,
                              void* c_prev_out, void* dots_dev_out, const void* mag_fm, void* gmag_fm_accum);
/* the closing step, iteration 1: t_1 = c_1 = d_1 = where(W, offset, P(c_0) + offset).  With s = a + gc + gd (gd NULL: absent):
 * goff_accum += s ; gc_inout <- (W ? 0 : s) / envelope, then the projection's adjoint at c0: gc_inout receives the cotangent of c0. */
int specinv_cgla_first_adjoint(specinv_plan* plan, const void* c0, const void* fixed_mask, const void* a, void* gc_inout, const void* gd,
                               void* goff_accum, const void* mag_fm, void* gmag_fm_accum);
/* ---- one projection as a layer (gla_projection; csrc/kernels_proj_adjoint.h) ---------------
 * y = P(x; m) = ISTFT(m S / (|S| + 1e-16)), S = STFT(x): one Griffin-Lim iteration without momentum (methods.py:241-248), on
 * signals.  x and y_out are (batch, length), mag_fm is frame-major, (batch, n_frames, n_freq); y_out must not alias x.  All three
 * entries are stateless as the MISI / AGLA adjoint entries above: a plan in any method state, scratch only.  SPECINV_EINVAL before
 * anything is enqueued: a NULL pointer, an aliased output. */
int specinv_project(specinv_plan* plan, const void* x, const void* mag_fm, void* y_out);
/* its adjoint at (x, mag_fm): g_y (batch, length), the cotangent of y, is read and left as it is; g_x_out (batch, length) and
 * gmag_fm_out (batch, n_frames, n_freq) are written in full, not accumulated.  S is recomputed from x.  Where |S| = 0 the second
 * term of the projection's derivative is 0 (k_misi_proj_adjoint's convention).  No atomics: two calls give the same bits. */
int specinv_project_adjoint(specinv_plan* plan, const void* x, const void* mag_fm, const void* g_y, void* g_x_out,
                            void* gmag_fm_out);
/* How specinv_project_adjoint runs on this plan (diagnostics; the tests assert which path they exercised): *kind_out = 0 the
 * staged path (two transforms, the element-wise adjoint, the inverse transform, every spectrum through device memory: any
 * configuration), 1 one fused launch that keeps a frame's spectra on the chip (one-sided, n_fft 128 / 256 / 512 / 1024 / 2048,
 * float32 and float64; SPECINV_PROJ_ADJ_FUSED=0 in the environment when the plan is created selects 0 instead). */
int specinv_project_adjoint_kind(const specinv_plan* plan, int32_t* kind_out);
/* adjoint of specinv_phase_init: gmag += d/dmag of <g_spec, phase_init(mag)> */
int specinv_phase_init_adjoint(specinv_plan* plan, const void* mag, const void* g_spec, void* gmag_accum);

/* ---- RTISI-LA (methods.py:273-412) ------------------------------------------------------ */
int specinv_rtisi_run(specinv_plan* plan, const void* mag, int look_ahead, int asymmetric_window,
                      int max_iter, double alpha, void* x_out);

/* RTISI_LA with a gradient (the reference's result is differentiable w.r.t. spec: test/test_rtisila.py:58-70).
 * `_run_recorded` is specinv_rtisi_run on the generic kernel that also stores every pre-projection spectrum in
 * `rec` (specinv_rtisi_record_elems() complex numbers of the plan's dtype); `_adjoint` sweeps the recursion
 * backwards: g_x (B, L) -> gmag_out (B, F, T), overwritten. */
int specinv_rtisi_record_elems(specinv_plan* plan, int look_ahead, int max_iter, int64_t* n_complex_out);
int specinv_rtisi_run_recorded(specinv_plan* plan, const void* mag, int look_ahead, int asymmetric_window, int max_iter,
                               double alpha, void* x_out, void* rec_out);
int specinv_rtisi_adjoint(specinv_plan* plan, const void* mag, const void* rec, const void* g_x, int look_ahead,
                          int asymmetric_window, int max_iter, double alpha, void* gmag_out);

/* Streaming RTISI-LA: the recursion of methods.py:363-404 fed a few frames at a time (what "real-time" in its name
 * is about, :275-278).  The plan's n_frames is the largest number of frames one push may carry; the stream length
 * is open-ended.  `push` takes (B, F, k) magnitudes and appends the samples that became final to x_out (row b at
 * x_out + b*out_stride; at most k*hop of them, *n_out per row, the first pushes give fewer: a sample is final once
 * look_ahead more frames are known).  `flush` ends the signal and returns the rest (at most look_ahead*hop + n_fft).
 * Concatenated, the pieces are the (B, L) result of specinv_rtisi_run on the whole spectrogram. */
int specinv_rtisi_stream_begin(specinv_plan* plan, int look_ahead, int asymmetric_window, int max_iter, double alpha);
int specinv_rtisi_stream_push(specinv_plan* plan, const void* mag, int k, void* x_out, int64_t out_stride,
                              int64_t* n_out);
int specinv_rtisi_stream_flush(specinv_plan* plan, void* x_out, int64_t out_stride, int64_t* n_out);

/* ---- Mel-spectrogram inversion, first stage: the linear magnitude (librosa's mel_to_stft) -------
 * Not in the reference, whose recipe for a mel spectrogram is L_BFGS on a log-mel transform (its README).  Per frame
 * (item b, frame t) with M the (n_mels, F) filterbank and y the mel column:
 *     minimise 1/2 |M s - y|^2 subject to s >= 0
 * by FISTA from s = 0, n_iter iterations of step 1 / lipschitz (z = s = 0, t = 1; g = M^T (M z - y),
 * s' = max(0, z - g / L), t' = (1 + sqrt(1 + 4 t^2)) / 2, z = s' + ((t - 1) / t') (s' - s)), then s ** (1 / power).
 * One launch runs every iteration of every frame.
 * `setup` takes the filterbank (a device array of the plan's dtype, F = specinv_plan_n_freq columns) and its constant
 * lipschitz = lambda_max(M M^T) (the host computes it, in float64); any matrix is valid, a sparse (banded) one is fast.
 * The plan keeps what it built until the next setup or its destruction.  EINVAL: n_mels <= 0, lipschitz <= 0 or not finite,
 * mel_fb NULL; EUNSUPPORTED: more than 32767 bands. */
int specinv_mel_nnls_setup(specinv_plan* plan, const void* mel_fb, int n_mels, double lipschitz);
/* mel (B, n_mels, T) -> mag_out (B, F, T), the plan's batch and frames, on its stream.  `power` is the exponent the mel was
 * built with (mel = M |S|^power: 1 magnitude, 2 power).  n_iter = 0 gives zeros; all-zero frames give exact zeros; negative
 * mel entries are valid.  EINVAL: n_iter < 0, power <= 0 or not finite, NULL pointers, no setup on this plan (all checked
 * before anything is enqueued); EUNSUPPORTED: a frame that does not fit a CU's LDS (beyond n_fft 8192 in float64). */
int specinv_mel_nnls(specinv_plan* plan, const void* mel, int n_iter, double power, void* mag_out);
/* The reverse sweep of specinv_mel_nnls (mel_to_stft_unfolded): gmag (B, F, T), the gradient of a loss with respect to mag_out,
 * -> gmel_out (B, n_mels, T), its gradient with respect to mel, for the same mel, n_iter and power, in one launch on the plan's
 * stream.  The launch recomputes the iteration from mel and keeps its active sets [s_k > 0] in LDS, one bit per bin and
 * iteration, so nothing is recorded by the forward call.  d max(0, u) / du is 0 at u = 0 and the root's derivative 0 at s = 0:
 * a silent frame and a band that touches no bin get exact zeros; n_iter = 0 gives zeros.  The filterbank is a constant.
 * EINVAL: as specinv_mel_nnls, gmag / gmel_out NULL (all checked before anything is enqueued); EUNSUPPORTED: n_iter beyond
 * specinv_mel_nnls_adjoint_max_iter (the message states the limit). */
int specinv_mel_nnls_adjoint(specinv_plan* plan, const void* mel, int n_iter, double power, const void* gmag, void* gmel_out);
/* *out = the largest n_iter specinv_mel_nnls_adjoint admits on this plan with its filterbank: what a CU's LDS holds beside one
 * frame.  EINVAL: out NULL, no setup on this plan; EUNSUPPORTED: the frame alone does not fit. */
int specinv_mel_nnls_adjoint_max_iter(specinv_plan* plan, int* out);

/* ---- L_BFGS building blocks (methods.py:509-569 + torch.optim.LBFGS) -------------------- */
/* transform kinds for the fused forward/backward: V = |STFT(x)| or V = log1p(M |STFT(x)|) */
enum { SPECINV_TF_MAG = 0, SPECINV_TF_LOGMEL = 1 };
/* mel_fb: (n_mels, F) device array or NULL for SPECINV_TF_MAG */
int specinv_transform_setup(specinv_plan* plan, int kind, const void* mel_fb, int n_mels);
/* V = transform(x): x (B, L_x) -> (B, n_out, T) with n_out = F or n_mels */
int specinv_transform_forward(specinv_plan* plan, const void* x, int64_t length, void* v_out);
/* loss = mean((transform(x) - target)^2) and d loss / d x (methods.py:545-550) */
int specinv_transform_loss_grad(specinv_plan* plan, const void* x, int64_t length, const void* target,
                                double* loss_host, void* grad_out);
/* How the last specinv_transform_loss_grad / _dev / lbfgs_dev_step of this plan evaluated the objective (diagnostics; the tests
 * assert that every implementation is covered): 0 a chain of kernels with the spectrum in device memory (any configuration),
 * 1 one launch, the mel contractions on the matrix cores (float32, one-sided, n_fft 1024 / 2048, <= 128 bands, any matrix),
 * 2 one launch, the filterbank in band form on the vector units (a sparse matrix - at most 4 rows per bin, <= 140 bands:
 * what a mel filterbank is; SPECINV_OBJ_SPARSE=0 in the environment selects 1 instead), 3 the frame walk (a wave per chunk of
 * frames, the contractions on each frame's own spectrum: hop = n_fft / 2, / 4, / 8, centred, at most two rows per bin; SPECINV_OBJ_WALK=0
 * selects 2 instead), -1 none yet. */
int specinv_transform_objective_kind(const specinv_plan* plan);
/* flat-vector kernels of the two-loop recursion (n elements of the plan dtype) */
int specinv_vec_dot(specinv_plan* plan, const void* a, const void* b, int64_t n, double* out_host);
int specinv_vec_axpy(specinv_plan* plan, double alpha, const void* x, void* y, int64_t n);
int specinv_vec_scale(specinv_plan* plan, double alpha, const void* x, void* y, int64_t n);
int specinv_vec_absmax_abssum(specinv_plan* plan, const void* x, int64_t n, double out_host[2]);
/* Many vectors in one pass: out_host[j] = g . v_j for the k device vectors whose addresses are in the HOST array
 * vecs_host; and out = sum_j coef_host[j] * v_j (float64 accumulation, rounded once).  With the k = 2m vectors of the
 * L-BFGS memory these two passes carry the whole two-loop recursion (the recursion itself then runs on the m x m
 * Gram matrices s_i.y_j, y_i.y_j on the host, which follow from the g . v_j of consecutive iterations by linearity):
 * 2 (2m + 1) vector reads per iteration instead of 10 m (`lbfgs.py:LBFGS._direction_gram`). */
int specinv_vec_multi_dot(specinv_plan* plan, const void* g, const void* const* vecs_host, int k, int64_t n,
                          double* out_host);
int specinv_vec_lincomb(specinv_plan* plan, const void* const* vecs_host, const double* coef_host, int k, int64_t n,
                        void* out);
/* The same, and the step x += t * out in the same pass (torch.optim.LBFGS.step: "p.add_(d, alpha=t)" right after the
 * direction): out is rounded first, x then takes fma(t, out, x) - what a separate specinv_vec_axpy would compute. */
int specinv_vec_lincomb_step(specinv_plan* plan, const void* const* vecs_host, const double* coef_host, int k, int64_t n,
                             void* out, double t, void* x);
/* The whole L-BFGS two-loop recursion d = -H g on the device (torch.optim.LBFGS.step's "compute the approximate
 * inverse Hessian multiplied by the gradient"): s_list_host / y_list_host are HOST arrays of m device pointers
 * (old_stps / old_dirs, oldest first), rho_host[m] = 1 / (y_i . s_i).  All 2m dot products stay on the device
 * (no host synchronisation); d_out receives the direction. */
int specinv_lbfgs_direction(specinv_plan* plan, const void* g, const void* const* s_list_host,
                            const void* const* y_list_host, const double* rho_host, int m, double h_diag,
                            void* d_out, int64_t n);
/* fused passes of one L-BFGS iteration (torch.optim.LBFGS.step): the curvature pair y = g - g_prev, s = t*d with
 * out_host = {y.s, y.y}; and the statistics of a step, out_host = {g.d, sum|g|, max|g|, max|d|}. */
int specinv_lbfgs_pair(specinv_plan* plan, const void* g, const void* g_prev, const void* d, double t, void* y_out,
                       void* s_out, int64_t n, double* out_host);
int specinv_lbfgs_stats(specinv_plan* plan, const void* g, const void* d, int64_t n, double* out_host);

/* The same passes with their scalar results left in DEVICE memory (doubles) and no host synchronisation, so that one
 * L-BFGS iteration (objective, step statistics, curvature pair, memory products) is enqueued back to back and the host
 * reads everything it needs for its decisions (torch.optim.LBFGS.step: y.s > 1e-10, the tolerance tests) with ONE
 * synchronisation: specinv_read_doubles.  pair: out_dev[4] = {y.s, y.y, g.g, g.g_prev}; stats: out_dev[4] as above;
 * multi_dot: out_dev[k]; loss_grad: *loss_dev = the loss. */
int specinv_transform_loss_grad_dev(specinv_plan* plan, const void* x, int64_t length, const void* target,
                                    double* loss_dev, void* grad_out);
/* The objective and the step statistics of its gradient in one go: out5_dev = {loss, g.d, sum|g|, max|g|, max|d|} with g the
 * gradient written to grad_out and d a device vector of the signal's shape (NULL: d = g) - what a trial point of the strong-Wolfe
 * search needs (torch.optim.lbfgs._strong_wolfe: f_new, gtd_new; torch.optim.LBFGS.step: opt_cond, d.abs().max()).  Where the
 * one-launch objective serves the plan the statistics are taken inside its launches, as each gradient sample becomes final;
 * otherwise by specinv_lbfgs_stats_dev's pass. */
int specinv_transform_loss_grad_stats_dev(specinv_plan* plan, const void* x, int64_t length, const void* target, const void* d,
                                          double* out5_dev, void* grad_out);
int specinv_vec_multi_dot_dev(specinv_plan* plan, const void* g, const void* const* vecs_host, int k, int64_t n,
                              double* out_dev);
int specinv_lbfgs_pair_dev(specinv_plan* plan, const void* g, const void* g_prev, const void* d, double t, void* y_out,
                           void* s_out, int64_t n, double* out_dev);
int specinv_lbfgs_stats_dev(specinv_plan* plan, const void* g, const void* d, int64_t n, double* out_dev);
/* both in one pass over g, g_prev, d: out_dev[8] = {g.d, sum|g|, max|g|, max|d|, y.s, y.y, g.g, g.g_prev} */
int specinv_lbfgs_pair_stats_dev(specinv_plan* plan, const void* g, const void* g_prev, const void* d, double t,
                                 void* y_out, void* s_out, int64_t n, double* out_dev);
/* n doubles from device memory to the host, after everything enqueued on the plan's stream so far */
int specinv_read_doubles(specinv_plan* plan, const double* src_dev, int n, double* out_host);
/* A board of n doubles in pinned host memory that the device writes directly (pass *dev_out + slot to the *_dev entry points):
 * the scalars of an iteration land in host memory without a copy kernel; specinv_stream_wait (everything enqueued on the
 * plan's stream so far has finished) makes *host_out readable.  The board lives as long as the plan. */
int specinv_board_alloc(specinv_plan* plan, int n, double** host_out, double** dev_out);
int specinv_stream_wait(specinv_plan* plan);

/* ---- L-BFGS with the decisions on the device (float32, the one-launch objective of specinv_transform_setup) --------------
 * Replaces the inner loop of torch.optim.LBFGS.step as torch_specinv/methods.py:553 drives it (no line search): one call
 * enqueues a whole optimizer.step - for each inner iteration the objective (which takes the statistics of its gradient on the
 * way) and ONE kernel that decides (tolerance tests, y.s > 1e-10, step length) and forms direction + step; with pairs in the
 * memory also the products with them and a one-workgroup decision kernel (memory ring, two-loop recursion on Gram matrices) -
 * and synchronises ONCE, at the end; after a break the rest of the enqueued step runs as no-ops.  The optimiser's state (memory, d, t, previous gradient / loss, counters) lives on the device between steps.
 * Options carry torch.optim.LBFGS's names; max_eval <= 0 means max_iter * 5 / 4.  history_size <= 120.
 * SPECINV_EUNSUPPORTED when the plan's transform is not served by the one-launch objective (the caller then runs the
 * host-driven loop on the *_dev entry points above). */
typedef struct specinv_lbfgs_opts {
  double lr, tolerance_grad, tolerance_change;
  int32_t max_iter, max_eval, history_size;
  int32_t time_objective;  /* k > 0: bracket every k-th objective evaluation of a step with HIP events (benchmarks:
                              specinv_lbfgs_info.objective_ms / objective_timed; an event pair costs ~10 us of the timeline) */
} specinv_lbfgs_opts;
typedef struct specinv_lbfgs_info {
  double first_loss;      /* what optimizer.step returns: the loss at the entry evaluation */
  double loss, t;
  int32_t total_iters, func_evals, n_iter, history_len, pairs_accepted, pairs_rejected;
  int32_t objective_launches;  /* evaluations this step executed, ... */
  int32_t objective_timed;     /* ... how many of them were bracketed with events (time_objective) ... */
  double objective_ms;         /* ... and the summed duration of those (objective + epilogue launch) */
  int32_t lean_iterations;     /* iterations enqueued so far in the lean form (objective, epilogue, decision + direction: memory empty) */
  int32_t full_iterations;     /* ... in the full form (+ memory products, one-workgroup decision kernel) */
  int32_t suspensions;         /* lean chains that met a non-empty memory and were resumed in the full form */
  int32_t reserved_;
} specinv_lbfgs_info;
/* `n` = elements of the parameter (batch * length); *handle_out identifies the optimiser within the plan */
int specinv_lbfgs_dev_create(specinv_plan* plan, int64_t n, const specinv_lbfgs_opts* opts, int32_t* handle_out);
/* one optimizer.step on x (batch, length), updated in place; target as in specinv_transform_loss_grad */
int specinv_lbfgs_dev_step(specinv_plan* plan, int32_t handle, void* x, int64_t length, const void* target,
                           specinv_lbfgs_info* info_out);
int specinv_lbfgs_dev_destroy(specinv_plan* plan, int32_t handle);

#ifdef __cplusplus
}
#endif
#endif /* SPECINV_H */
