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

Not part of the reference's surface.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers

import torch

from . import _lib
from ._ingest import ingest
from .plan import require_gpu

__all__ = ["yin", "yin_cmnd", "yin_frames"]

SUPPORTED_FRAMES = (256, 512, 1024, 2048)
_DTYPES = (torch.float16, torch.bfloat16, torch.float32)
_MAX_BLOCKS = 65535            # workgroups one call of the entry point is given: the wrapper slices the items beyond
_WAVES = 4                     # frames a workgroup takes (kernels_yin.h): an item is ceil(T / 4) workgroups


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _is_real(v):
    return isinstance(v, numbers.Real) and not isinstance(v, bool) and math.isfinite(v)


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
    lib = _lib.load()
    x2 = ingest(x.reshape(batch, x.shape[-1]), device, torch.float32)
    period = torch.empty((batch, n_frames), dtype=torch.float32, device=device)
    aper = torch.empty_like(period)
    tau = torch.empty((batch, n_frames), dtype=torch.int32, device=device) if want_tau else None
    cmnd = torch.empty((batch, n_frames, n // 2 + 1), dtype=torch.float32, device=device) if want_cmnd else None
    stream = torch.cuda.current_stream(device)
    per_call = max(1, _MAX_BLOCKS // -(-n_frames // _WAVES))                         # items whose workgroups fit one call
    for b0 in range(0, batch, per_call):
        nb = min(per_call, batch - b0)
        _lib.check(lib.specinv_yin(x2[b0:].data_ptr(), period[b0:].data_ptr(), aper[b0:].data_ptr(),
                                   tau[b0:].data_ptr() if want_tau else None, cmnd[b0:].data_ptr() if want_cmnd else None, nb,
                                   x2.shape[-1], n, h, int(bool(center)), tau_min, tau_max, threshold, _lib.F32,
                                   stream.device.index, C.c_void_p(stream.cuda_stream)))
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
