"""Fundamental frequency: `yin`, the estimator of de Cheveigne & Kawahara 2002 in one kernel launch (csrc/kernels_yin.h;
DESIGN 3.28), `yin_cmnd`, the normalised difference function it picks from, and `yin_frames`.  `pitch_shift(...,
preserve_formants=True, formant_order="f0")` reads the envelope order off it (`envelope_order_for_f0`).

`x` is (L,) / (B, L), real.  N = frame_length is one of 256, 512, 1024, 2048, W = N / 2, H = hop_length in 1 ... N, default N / 4;
xz(i) = x[i] for 0 <= i < L, else 0.

    Frames       center=True (default): T = 1 + L // H, s_m = m H - W;  center=False: needs L >= N, T = 1 + (L - N) // H, s_m = m H.
                 f_m[j] = xz(s_m + j), j < N.
    Difference   d(tau) = sum_{j<W} (f[j] - f[j+tau])^2 = E(0) + E(tau) - 2 r(tau), tau = 0 ... W, with
                 E(tau) = sum_{j=tau}^{tau+W-1} f[j]^2 and r(tau) = sum_{j<W} f[j] f[j+tau]: the first W + 1 lags of the circular
                 length-N correlation of the frame with its own first half zero-padded to N; nothing wraps for tau <= N - W.
    Normalised   d'(0) = 1;  c(tau) = sum_{k=1}^{tau} d(k);  d'(tau) = d(tau) tau / c(tau) where c(tau) > 0, else 1.  A silent
                 frame is therefore d' = 1 throughout.
    Pick         over [tau_min, tau_max] = [floor(sample_rate / fmax), ceil(sample_rate / fmin)], which must satisfy
                 1 <= tau_min < tau_max <= W - 1:  tau0 is the smallest tau of the range with d'(tau) < threshold.  If it exists,
                 tau* = tau0, advanced while tau* + 1 <= tau_max and d'(tau* + 1) < d'(tau*); if not, tau* is the first arg-min
                 of d' over the range.
    Refinement   a, b, c = d'(tau* - 1), d'(tau*), d'(tau* + 1), q = a - 2 b + c;  s = (a - c) / (2 q) if q > 0 and |a - c| < q,
                 else 0;  period = tau* + s;  aperiodicity = b;  voiced = b < threshold, exactly the condition that tau0 existed.

Arithmetic: float32 input (float16 and bfloat16 are computed in float32); r goes through the float32 wave-level FFT (the lags
1 ... 8, where d is a small difference of large numbers, take d from the literal sum in float64); E, d and c are kept in float64;
d' is rounded once to float32; the pick runs on those float32 values - the numbers `yin_cmnd` returns - against the float64
threshold; the refinement runs in float64 from the three float32 values and is rounded once.  float64 input is a
NotImplementedError.  NaN input is unspecified.  Not differentiable.

    f0, voiced, aper = si.yin(x, 16000, fmin=60, fmax=1000)                    # (B, T) each, 2048-sample frames every 512
    order = si.envelope_order_for_f0(16000, f0[voiced].median().item())
    dprime = si.yin_cmnd(x)                                                    # (B, T, 1025): where a pYIN or another picker starts

Probabilistic YIN: `pyin` (Mauch & Dixon 2014, in librosa.pyin's formulation) reads that d' in three launches (csrc/kernels_pyin.h;
DESIGN 3.29): `specinv_yin` for d', a frame-parallel kernel for the observation probabilities, and one workgroup per item for the
Viterbi decode.  `pyin_observations` and `pyin_decode` are the two stages, `pyin_bins` the size of the pitch grid.  Frame, hop, W, T,
d', [tau_min, tau_max] and the refinement are those above; K = n_thresholds, (a, b) = beta_parameters, lam = boltzmann_parameter,
s = switch_prob, q = no_trough_prob.

    Prior        s_k = k / K, w_k = I_{s_k}(a, b) - I_{s_{k-1}}(a, b), k = 1 ... K, for integer a, b from the binomial sum
                 I_x = sum_{j=a}^{n} C(n, j) x^j (1 - x)^(n-j), n = a + b - 1, in float64 on the host - formed from its complement
                 sum_{j<a}, so that the small weights near s = 1 keep their digits.  Or `threshold_prior`, K weights used as given.
    Troughs      tau in [tau_min, tau_max] with d'(tau) < d'(tau - 1) and d'(tau) <= d'(tau + 1), on the float32 d' of `yin_cmnd`.
    Candidates   For threshold k the troughs with d'(tau) < s_k (float64) are ranked by rising lag, r_k(tau) = 0, 1, ..., n_k - 1:
                 p(tau) = sum_k w_k [d'(tau) < s_k] (1 - e^-lam) e^(-lam r_k(tau)) / (1 - e^(-lam n_k)).  The first arg-min trough
                 tau_g also gets q sum_{k<=m} w_k, m the number of thresholds with d'(tau_g) >= s_k.
    Observation  bps = ceil(1 / resolution), P = floor(12 bps log2(fmax / fmin)) + 1.  A trough with p > 0 has period tau + shift
                 (the refinement) and bin rint(12 bps log2(sample_rate / period / fmin)); a bin below 0 is bin 0, a bin above P - 1
                 is dropped; of several candidates in a bin the largest lag stands.  o_v[j] is that p, else 0;
                 voiced_prob = clip(sum_j o_v[j], 0, 1); every unvoiced state observes (1 - voiced_prob) / P.
    HMM          2P states: j < P is voiced bin j, P + j unvoiced bin j.  m = round(max_transition_rate 12 H / sample_rate),
                 width = m bps + 1 (odd), half = (width - 1) / 2, tri(k) = 1 - |k| / ((width + 1) / 2);  A[i][j] = tri(j - i) / Z_i for
                 |j - i| <= half with Z_i the sum of tri over the j that exist, else 0;  transition [[1 - s, s], [s, 1 - s]] (x) A;
                 initially 1 / P on the unvoiced states.  Every probability enters as log(p + tiny), tiny the smallest normal
                 float64: a zero is a floor, not -inf.  Viterbi in float64, ties to the lowest state index.
                 f0 = fmin 2^((state mod P) / (12 bps)), voiced_flag = state < P, f0 = fill_na on unvoiced frames.

Where this departs from librosa.pyin: d' is this package's (frames and their centring as above, W lags of a sum over W samples, where
librosa correlates over frame_length - max_period samples); the troughs are taken over [tau_min, tau_max] with the real neighbours
d'(tau_min - 1) and d'(tau_max + 1), where librosa cuts d' to the range first and treats its ends by a rule of their own; a frame
without a trough (silence, d' = 1 throughout) has no candidate and voiced_prob 0, where librosa's arg-min of an empty frame is lag
tau_min; and the observations are rounded to float32 between the two stages.

    f0, voiced, prob = si.pyin(x, 16000, fmin=65, fmax=2093)                  # (B, T) each; f0 is NaN where unvoiced

Not part of the reference's surface.
"""
from __future__ import annotations

import functools
import math

import torch

from . import _lib
from ._ingest import ingest, is_int as _is_int, is_real
from .plan import require_gpu

__all__ = ["yin", "yin_cmnd", "yin_frames", "pyin", "pyin_observations", "pyin_decode", "pyin_bins"]

SUPPORTED_FRAMES = (256, 512, 1024, 2048)
_DTYPES = (torch.float16, torch.bfloat16, torch.float32)
_MAX_BLOCKS = 65535            # workgroups one call of the entry point is given: the wrapper slices the items beyond
_WAVES = 4                     # frames a workgroup takes (kernels_yin.h): an item is ceil(T / 4) workgroups


def _is_real(v):
    return is_real(v) and math.isfinite(v)


def _checked_frame(frame_length, hop_length):
    """(N, H): ValueError for what is no frame or hop at all, NotImplementedError for a frame length the kernel does not cover"""
    if not _is_int(frame_length) or frame_length < 2:
        raise ValueError(f"frame_length must be an int, one of {', '.join(map(str, SUPPORTED_FRAMES))}, got {frame_length!r}")
    if frame_length not in SUPPORTED_FRAMES:
        raise NotImplementedError(f"yin supports frame_length {', '.join(map(str, SUPPORTED_FRAMES))}, got {frame_length}")
    if hop_length is None:
        hop_length = frame_length // 4
    if not _is_int(hop_length) or not 1 <= hop_length <= frame_length:
        raise ValueError(f"hop_length must be an int in 1 ... frame_length = {frame_length}, got {hop_length!r}")
    return frame_length, hop_length


def yin_frames(length, frame_length, hop_length=None, center=True):
    """The number of frames T that `yin` and `yin_cmnd` return for `length` samples (the module's definition): 1 + L // H with
    `center=True`, 1 + (L - N) // H without, which needs L >= N."""
    n, h = _checked_frame(frame_length, hop_length)
    if not _is_int(length) or length < 1:
        raise ValueError(f"length must be an int >= 1, got {length!r}")
    if center:
        return 1 + length // h
    if length < n:
        raise ValueError(f"center=False needs at least frame_length = {n} samples, got {length}")
    return 1 + (length - n) // h


def _lag_range(sample_rate, fmin, fmax, frame_length):
    """(tau_min, tau_max) = (floor(sample_rate / fmax), ceil(sample_rate / fmin)), checked against 1 <= tau_min < tau_max <= W - 1"""
    for name, v in (("sample_rate", sample_rate), ("fmin", fmin), ("fmax", fmax)):
        if not _is_real(v) or not v > 0:
            raise ValueError(f"{name} must be a finite number > 0, got {v!r}")
    if not fmin < fmax:
        raise ValueError(f"fmin must be below fmax, got {fmin!r} and {fmax!r}")
    top = frame_length // 2 - 1
    lowest = sample_rate / top
    if sample_rate / fmax >= 1 << 31 or sample_rate / fmin > top:
        raise ValueError(f"fmin = {fmin!r} needs lags up to {math.ceil(min(sample_rate / fmin, 1e18))}, frame_length {frame_length} "
                         f"holds {top}: the smallest fmin it allows at {sample_rate!r} Hz is {lowest!r}")
    tau_min, tau_max = math.floor(sample_rate / fmax), math.ceil(sample_rate / fmin)
    if tau_min < 1:
        raise ValueError(f"fmax = {fmax!r} is above the sampling rate {sample_rate!r}: the shortest lag would be 0")
    if not tau_min < tau_max <= top:
        raise ValueError(f"fmin = {fmin!r}, fmax = {fmax!r} give the lags {tau_min} ... {tau_max}, which must satisfy "
                         f"tau_min < tau_max <= {top}: the smallest fmin frame_length {frame_length} allows at {sample_rate!r} Hz "
                         f"is {lowest!r}")
    return tau_min, tau_max


def _checked_signal(x, what):
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    if x.dtype == torch.float64:
        raise NotImplementedError(f"{what} is implemented in float32: a {x.dtype} input is not supported")
    if x.dtype not in _DTYPES:
        raise TypeError(f"x must be float16 / bfloat16 / float32, got dtype {x.dtype}")
    if x.dim() not in (1, 2):
        raise ValueError(f"x must be (L,) or (B, L), got shape {tuple(x.shape)}")


def _run(x, what, n, h, center, tau_min, tau_max, threshold, want_tau, want_cmnd):
    """(period, aperiodicity, tau or None, cmnd or None), each with x's leading shape, on x's device"""
    n_frames = yin_frames(x.shape[-1], n, h, center)
    if torch.is_grad_enabled() and x.requires_grad:
        raise NotImplementedError(f"{what} is not differentiable; detach the input")
    lead = tuple(x.shape[:-1])
    batch = x.shape[0] if x.dim() == 2 else 1
    if batch == 0:
        period = torch.zeros(lead + (n_frames,), dtype=torch.float32, device=x.device)
        return (period, period.clone(), torch.zeros(lead + (n_frames,), dtype=torch.int32, device=x.device) if want_tau else None,
                torch.zeros(lead + (n_frames, n // 2 + 1), dtype=torch.float32, device=x.device) if want_cmnd else None)
    device = require_gpu(x.device)
    x2 = ingest(x.reshape(batch, x.shape[-1]), device, torch.float32)
    period = torch.empty((batch, n_frames), dtype=torch.float32, device=device)
    aper = torch.empty_like(period)
    tau = torch.empty((batch, n_frames), dtype=torch.int32, device=device) if want_tau else None
    cmnd = torch.empty((batch, n_frames, n // 2 + 1), dtype=torch.float32, device=device) if want_cmnd else None
    per_call = max(1, _MAX_BLOCKS // -(-n_frames // _WAVES))                         # items whose workgroups fit one call
    for b0 in range(0, batch, per_call):
        nb = min(per_call, batch - b0)
        _lib.call_op("specinv_yin", (x2[b0:], period[b0:], aper[b0:], tau[b0:] if want_tau else None, cmnd[b0:] if want_cmnd else None,
                                     nb, x2.shape[-1], n, h, int(bool(center)), tau_min, tau_max, threshold), False, device)
    return tuple(None if o is None else o.reshape(lead + tuple(o.shape[1:])).to(x.device) for o in (period, aper, tau, cmnd))


def yin(x, sample_rate, fmin, fmax, frame_length=2048, hop_length=None, threshold=0.1, center=True, return_tau=False):
    r"""The fundamental frequency of a waveform (L,) / (B, L) sampled at `sample_rate`, frame by frame: `(f0, voiced,
    aperiodicity)`, each (T,) / (B, T) with T = `yin_frames(L, frame_length, hop_length, center)`, on x's device.  The definition
    is the module's.

    `f0` is float32, in Hz: `(sample_rate / period.double()).float()` with the refined period in samples; it lies within
    `fmin` ... `fmax` up to the rounding of the lags `floor(sample_rate / fmax)` and `ceil(sample_rate / fmin)` and the refinement's
    half sample.  `voiced` is bool: some lag of the range fell below `threshold` (> 0; 0.1 ... 0.15 is the paper's range).
    `aperiodicity` is float32: d' at the chosen lag, about the share of the frame's power that is not periodic.  On an unvoiced
    frame f0 is the best candidate of the range, not a measurement.  `return_tau=True` adds the int32 lags tau* as a fourth value.

    `frame_length` must hold two periods of `fmin` and one sample more: `ceil(sample_rate / fmin) <= frame_length / 2 - 1`,
    otherwise a ValueError names the smallest `fmin` that fits.  frame_length 256, 512, 1024 and 2048; float16 / bfloat16 are
    computed in float32; float64 and other frame lengths are a NotImplementedError.  Any layout torch can express is read as
    torch would read it.  A CPU tensor is computed on the current HIP device and comes back to the CPU.  Any number of items.
    Not differentiable.
    """
    _checked_signal(x, "yin")
    n, h = _checked_frame(frame_length, hop_length)
    tau_min, tau_max = _lag_range(sample_rate, fmin, fmax, n)
    if not _is_real(threshold) or not threshold > 0:
        raise ValueError(f"threshold must be a finite number > 0, got {threshold!r}")
    threshold = float(threshold)
    period, aper, tau, _ = _run(x, "yin", n, h, center, tau_min, tau_max, threshold, bool(return_tau), False)
    f0 = (float(sample_rate) / period.double()).float()
    voiced = aper.double() < threshold
    return (f0, voiced, aper, tau) if return_tau else (f0, voiced, aper)


def yin_cmnd(x, frame_length=2048, hop_length=None, center=True):
    """The cumulative-mean-normalised difference function d' of every frame of a waveform (L,) / (B, L): float32,
    (T, W + 1) / (B, T, W + 1) with W = frame_length / 2, lag 0 ... W along the last axis, on x's device.  These are the numbers
    `yin` picks from, bit for bit: what a probabilistic YIN or a picker of your own starts from.  The limits of `yin` apply."""
    _checked_signal(x, "yin_cmnd")
    n, h = _checked_frame(frame_length, hop_length)
    return _run(x, "yin_cmnd", n, h, center, 1, n // 2 - 1, 0.1, False, True)[3]


# ---- pYIN

PYIN_MAX_BINS = 1024           # P: 2 P <= 2048 states (kernels_pyin.h)
PYIN_MAX_WIDTH = 1025          # the transition band, 2 half + 1
PYIN_MAX_THRESHOLDS = 1024
_TINY = 2.2250738585072014e-308


def _bins_per_semitone(resolution):
    if not _is_real(resolution) or not 0 < resolution <= 1:
        raise ValueError(f"resolution must be a number of semitones in (0, 1], got {resolution!r}")
    return math.ceil(1.0 / resolution)


def pyin_bins(fmin, fmax, resolution=0.1):
    """The number of pitch bins P of `pyin`'s grid: floor(12 bps log2(fmax / fmin)) + 1 with bps = ceil(1 / resolution); bin j is
    fmin 2^(j / (12 bps)) Hz.  The model has 2 P states."""
    for name, v in (("fmin", fmin), ("fmax", fmax)):
        if not _is_real(v) or not v > 0:
            raise ValueError(f"{name} must be a finite number > 0, got {v!r}")
    if not fmin < fmax:
        raise ValueError(f"fmin must be below fmax, got {fmin!r} and {fmax!r}")
    return math.floor(12 * _bins_per_semitone(resolution) * math.log2(fmax / fmin)) + 1


def _checked_bins(fmin, fmax, resolution):
    n_bins = pyin_bins(fmin, fmax, resolution)
    if n_bins > PYIN_MAX_BINS:
        raise NotImplementedError(f"pyin supports at most P = {PYIN_MAX_BINS} pitch bins (2 P = {2 * PYIN_MAX_BINS} states); fmin = "
                                  f"{fmin!r}, fmax = {fmax!r} at resolution {resolution!r} give {n_bins}")
    return n_bins


def _beta_tail(x, a, b):
    n = a + b - 1
    return sum(math.comb(n, j) * x ** j * (1.0 - x) ** (n - j) for j in range(a))


def _threshold_prior(n_thresholds, beta_parameters, threshold_prior):
    """the K weights as a tuple of floats"""
    if not _is_int(n_thresholds) or not 1 <= n_thresholds <= PYIN_MAX_THRESHOLDS:
        raise ValueError(f"n_thresholds must be an int in 1 ... {PYIN_MAX_THRESHOLDS}, got {n_thresholds!r}")
    if threshold_prior is not None:
        w = tuple(float(v) for v in (threshold_prior.tolist() if hasattr(threshold_prior, "tolist") else threshold_prior))
        if len(w) != n_thresholds or not all(math.isfinite(v) and v >= 0 for v in w):
            raise ValueError(f"threshold_prior must hold n_thresholds = {n_thresholds} finite weights >= 0")
        return w
    try:
        a, b = beta_parameters
    except (TypeError, ValueError):
        raise ValueError(f"beta_parameters must be a pair (a, b), got {beta_parameters!r}") from None
    if not (_is_real(a) and _is_real(b) and a > 0 and b > 0):
        raise ValueError(f"beta_parameters must be two finite numbers > 0, got {beta_parameters!r}")
    if a != int(a) or b != int(b):
        raise NotImplementedError(f"the threshold prior is formed for integer beta_parameters, got {beta_parameters!r}: pass "
                                  f"threshold_prior, the n_thresholds weights, for any other distribution")
    return _integer_prior(n_thresholds, int(a), int(b))


@functools.lru_cache(maxsize=32)
def _integer_prior(n_thresholds, a, b):
    q = [_beta_tail(k / n_thresholds, a, b) for k in range(n_thresholds + 1)]
    return tuple(q[k - 1] - q[k] for k in range(1, n_thresholds + 1))


@functools.lru_cache(maxsize=16)
def _obs_tables(w, lam, n_ranks, device):
    """specinv_pyin_obs's `tables` on the device: s_k, w_k, cum[0 ... K], boltz[0 ... n_ranks - 1], inv[0 ... n_ranks]"""
    k_thr = len(w)
    cum = [0.0]
    for v in w:
        cum.append(cum[-1] + v)
    boltz = [(1.0 - math.exp(-lam)) * math.exp(-lam * r) for r in range(n_ranks)]
    inv = [0.0] + [1.0 / (1.0 - math.exp(-lam * c)) for c in range(1, n_ranks + 1)]
    host = [k / k_thr for k in range(1, k_thr + 1)] + list(w) + cum + boltz + inv
    return torch.tensor(host, dtype=torch.float64).to(device)


@functools.lru_cache(maxsize=16)
def _decode_tables(n_bins, half, device):
    """specinv_pyin_viterbi's `tables` on the device: log tri(0 ... half), then -log Z_i"""
    tri = [1.0 - k / (half + 1.0) for k in range(half + 1)]
    prefix = [0.0]
    for v in tri[1:]:
        prefix.append(prefix[-1] + v)                      # tri(1) + ... + tri(k)
    z = [tri[0] + prefix[min(half, i)] + prefix[min(half, n_bins - 1 - i)] for i in range(n_bins)]
    return torch.tensor([math.log(v) for v in tri] + [-math.log(v) for v in z], dtype=torch.float64).to(device)


def _checked_obs_params(boltzmann_parameter, no_trough_prob):
    if not _is_real(boltzmann_parameter) or not boltzmann_parameter > 0:
        raise ValueError(f"boltzmann_parameter must be a finite number > 0, got {boltzmann_parameter!r}")
    if not _is_real(no_trough_prob) or not 0 <= no_trough_prob <= 1:
        raise ValueError(f"no_trough_prob must be in 0 ... 1, got {no_trough_prob!r}")
    return float(boltzmann_parameter), float(no_trough_prob)


def _checked_switch(switch_prob):
    if not _is_real(switch_prob) or not 0 < switch_prob < 1:
        raise ValueError(f"switch_prob must be in (0, 1), got {switch_prob!r}")
    return float(switch_prob)


def _checked_half(half_width):
    if not _is_int(half_width) or half_width < 0:
        raise ValueError(f"half_width must be an int >= 0, got {half_width!r}")
    if 2 * half_width + 1 > PYIN_MAX_WIDTH:
        raise NotImplementedError(f"pyin supports a transition band of at most width = {PYIN_MAX_WIDTH} bins, got "
                                  f"{2 * half_width + 1}")
    return half_width


def _transition_half(sample_rate, hop, bps, max_transition_rate):
    if not _is_real(max_transition_rate) or not max_transition_rate >= 0:
        raise ValueError(f"max_transition_rate must be a finite number of octaves per second >= 0, got {max_transition_rate!r}")
    width = round(max_transition_rate * 12 * hop / sample_rate) * bps + 1
    if width > PYIN_MAX_WIDTH:
        raise NotImplementedError(f"pyin supports a transition band of at most width = {PYIN_MAX_WIDTH} bins; max_transition_rate = "
                                  f"{max_transition_rate!r} at hop {hop} and {bps} bins per semitone gives {width}")
    if width % 2 == 0:
        raise NotImplementedError(f"the transition band must have an odd width; max_transition_rate = {max_transition_rate!r} at hop "
                                  f"{hop} and {bps} bins per semitone gives {width}")
    return (width - 1) // 2


def _observe(xd, n, h, center, tau_min, tau_max, w, lam, q, n_bins, bps, sample_rate, fmin):
    """(obs (B, T, P), voiced_prob (B, T)) on the device from the device signal (B, L): launches 1 and 2"""
    cmnd = _run(xd, "pyin", n, h, center, 1, n // 2 - 1, 0.1, False, True)[3]
    batch, n_frames = cmnd.shape[0], cmnd.shape[1]
    n_ranks = (tau_max - tau_min) // 2 + 1
    tables = _obs_tables(w, lam, n_ranks, xd.device)
    obs = torch.empty((batch, n_frames, n_bins), dtype=torch.float32, device=xd.device)
    vprob = torch.empty((batch, n_frames), dtype=torch.float32, device=xd.device)
    _lib.call_op("specinv_pyin_obs", (cmnd, tables, obs, vprob, batch * n_frames, n, tau_min, tau_max, len(w), n_ranks, n_bins, bps,
                                      float(sample_rate), float(fmin), q), False, xd.device)
    return obs, vprob


def _decode(obs, vprob, half, switch, ticks=None):
    """int32 states (B, T) on the device from device observations: launch 3"""
    batch, n_frames, n_bins = obs.shape
    tables = _decode_tables(n_bins, half, obs.device)
    backptr = torch.empty((batch, n_frames, 2 * n_bins), dtype=torch.int16, device=obs.device)
    states = torch.empty((batch, n_frames), dtype=torch.int32, device=obs.device)
    _lib.call_op("specinv_pyin_viterbi", (obs, vprob, tables, backptr, states, ticks, batch, n_frames, n_bins, half, switch), False,
                 obs.device)
    return states


def _pyin_signal(x, what, n, h, center):
    """(device signal (B, L) or None for no items, lead shape, T): the checks of `_run` that come before the device"""
    n_frames = yin_frames(x.shape[-1], n, h, center)
    if torch.is_grad_enabled() and x.requires_grad:
        raise NotImplementedError(f"{what} is not differentiable; detach the input")
    lead = tuple(x.shape[:-1])
    batch = x.shape[0] if x.dim() == 2 else 1
    if batch == 0:
        return None, lead, n_frames
    device = require_gpu(x.device)
    _lib.load()
    return ingest(x.reshape(batch, x.shape[-1]), device, torch.float32), lead, n_frames


def pyin_observations(x, sample_rate, fmin, fmax, frame_length=2048, hop_length=None, n_thresholds=100, beta_parameters=(2, 18),
                      boltzmann_parameter=2.0, resolution=0.1, no_trough_prob=0.01, center=True, threshold_prior=None):
    """The observation stage of `pyin`: `(obs, voiced_prob)` of a waveform (L,) / (B, L), float32, on x's device.  `obs` is
    (T, P) / (B, T, P) with P = `pyin_bins(fmin, fmax, resolution)`: the probability o_v[j] that the frame is voiced at pitch bin j
    (the module's definition), at most one candidate per bin, zeros elsewhere.  `voiced_prob` is (T,) / (B, T), their sum clipped
    to 0 ... 1; each of the P unvoiced states observes (1 - voiced_prob) / P.  Two launches.  The limits of `pyin` apply."""
    _checked_signal(x, "pyin_observations")
    n, h = _checked_frame(frame_length, hop_length)
    tau_min, tau_max = _lag_range(sample_rate, fmin, fmax, n)
    n_bins = _checked_bins(fmin, fmax, resolution)
    bps = _bins_per_semitone(resolution)
    w = _threshold_prior(n_thresholds, beta_parameters, threshold_prior)
    lam, q = _checked_obs_params(boltzmann_parameter, no_trough_prob)
    xd, lead, n_frames = _pyin_signal(x, "pyin_observations", n, h, center)
    if xd is None:
        return (torch.zeros(lead + (n_frames, n_bins), dtype=torch.float32, device=x.device),
                torch.zeros(lead + (n_frames,), dtype=torch.float32, device=x.device))
    obs, vprob = _observe(xd, n, h, center, tau_min, tau_max, w, lam, q, n_bins, bps, sample_rate, fmin)
    return obs.reshape(lead + (n_frames, n_bins)).to(x.device), vprob.reshape(lead + (n_frames,)).to(x.device)


def pyin_decode(obs, voiced_prob, half_width, bins_per_semitone, switch_prob=0.01):
    """The decode stage of `pyin` alone, for observations of your own: the Viterbi path of the module's 2 P-state model, int32
    (T,) / (B, T) on obs's device.  `obs` is (T, P) / (B, T, P) float32, the voiced observation probabilities, `voiced_prob`
    (T,) / (B, T) float32; state j < P is voiced bin j, state P + j unvoiced bin j, and `state % P` is the bin in both cases.
    `half_width` is the half width of the transition band in bins ((width - 1) / 2 of the module's definition);
    `bins_per_semitone` says what grid the bins are on (bin j is fmin 2^(j / (12 bins_per_semitone))): the path itself does not depend on
    it.  One launch, one workgroup per item; P <= 1024 and 2 half_width + 1 <= 1025."""
    if not isinstance(obs, torch.Tensor) or not isinstance(voiced_prob, torch.Tensor):
        raise TypeError("obs and voiced_prob must be torch.Tensors")
    if obs.dtype != torch.float32 or voiced_prob.dtype != torch.float32:
        raise TypeError(f"obs and voiced_prob must be float32, got {obs.dtype} and {voiced_prob.dtype}")
    if obs.dim() not in (2, 3) or voiced_prob.shape != obs.shape[:-1]:
        raise ValueError(f"obs must be (T, P) or (B, T, P) and voiced_prob (T,) or (B, T), got {tuple(obs.shape)} and "
                         f"{tuple(voiced_prob.shape)}")
    n_frames, n_bins = obs.shape[-2], obs.shape[-1]
    if n_frames < 1 or n_bins < 1:
        raise ValueError(f"obs needs at least one frame and one bin, got shape {tuple(obs.shape)}")
    if n_bins > PYIN_MAX_BINS:
        raise NotImplementedError(f"pyin_decode supports at most P = {PYIN_MAX_BINS} pitch bins, got {n_bins}")
    half = _checked_half(half_width)
    if not _is_int(bins_per_semitone) or bins_per_semitone < 1:
        raise ValueError(f"bins_per_semitone must be an int >= 1, got {bins_per_semitone!r}")
    switch = _checked_switch(switch_prob)
    if torch.is_grad_enabled() and (obs.requires_grad or voiced_prob.requires_grad):
        raise NotImplementedError("pyin_decode is not differentiable; detach the input")
    lead = tuple(obs.shape[:-2])
    batch = obs.shape[0] if obs.dim() == 3 else 1
    if batch == 0:
        return torch.zeros(lead + (n_frames,), dtype=torch.int32, device=obs.device)
    device = require_gpu(obs.device)
    _lib.load()
    od = ingest(obs.reshape(batch, n_frames, n_bins), device, torch.float32)
    vd = ingest(voiced_prob.reshape(batch, n_frames), device, torch.float32)
    return _decode(od, vd, half, switch).reshape(lead + (n_frames,)).to(obs.device)


def pyin(x, sample_rate, fmin, fmax, frame_length=2048, hop_length=None, n_thresholds=100, beta_parameters=(2, 18),
         boltzmann_parameter=2.0, resolution=0.1, max_transition_rate=35.92, switch_prob=0.01, no_trough_prob=0.01,
         fill_na=float("nan"), center=True, threshold_prior=None, return_states=False):
    r"""Probabilistic YIN: the fundamental frequency of a waveform (L,) / (B, L) as one smooth track with a voiced / unvoiced
    decision, `(f0, voiced_flag, voiced_prob)`, each (T,) / (B, T) with T = `yin_frames(L, frame_length, hop_length, center)`, on
    x's device.  The definition is the module's; the parameters and their defaults are librosa.pyin's.

    `f0` is float32, in Hz, on the grid fmin 2^(j / (12 bps)), bps = ceil(1 / resolution) bins per semitone, and `fill_na` (NaN by
    default) on the frames decoded as unvoiced.  `voiced_flag` is bool.  `voiced_prob` is float32: the probability mass the
    frame's candidates carry, before the decode.  `return_states=True` adds the int32 states of the path: state j < P voiced bin
    j, P + j unvoiced bin j, P = `pyin_bins(fmin, fmax, resolution)`.

    `beta_parameters` must be integers - the prior is then a finite sum - unless `threshold_prior`, the n_thresholds weights
    themselves, is given.  Limits, checked before the device is touched: P <= 1024; the transition band
    round(max_transition_rate 12 hop / sample_rate) bps + 1 odd and <= 1025; 1 <= n_thresholds <= 1024; 0 < switch_prob < 1;
    0 <= no_trough_prob <= 1; boltzmann_parameter > 0; resolution in (0, 1]; frame lengths, dtypes and layouts as `yin`.  Any
    number of items; the frames are bounded only by the (B, T, 2 P) int16 scratch of the decode.  Three launches.  Not
    differentiable.
    """
    _checked_signal(x, "pyin")
    n, h = _checked_frame(frame_length, hop_length)
    tau_min, tau_max = _lag_range(sample_rate, fmin, fmax, n)
    n_bins = _checked_bins(fmin, fmax, resolution)
    bps = _bins_per_semitone(resolution)
    w = _threshold_prior(n_thresholds, beta_parameters, threshold_prior)
    lam, q = _checked_obs_params(boltzmann_parameter, no_trough_prob)
    switch = _checked_switch(switch_prob)
    half = _transition_half(sample_rate, h, bps, max_transition_rate)
    if not is_real(fill_na):
        raise ValueError(f"fill_na must be a number, got {fill_na!r}")
    xd, lead, n_frames = _pyin_signal(x, "pyin", n, h, center)
    if xd is None:
        f0 = torch.zeros(lead + (n_frames,), dtype=torch.float32, device=x.device)
        out = (f0, f0.bool(), f0.clone())
        return out + (f0.int(),) if return_states else out
    obs, vprob = _observe(xd, n, h, center, tau_min, tau_max, w, lam, q, n_bins, bps, sample_rate, fmin)
    states = _decode(obs, vprob, half, switch)
    voiced = states < n_bins
    f0 = (float(fmin) * torch.exp2((states % n_bins).double() / (12 * bps))).float()
    f0 = torch.where(voiced, f0, torch.full_like(f0, float(fill_na)))
    out = tuple(o.reshape(lead + (n_frames,)).to(x.device) for o in (f0, voiced, vprob, states))
    return out if return_states else out[:3]
