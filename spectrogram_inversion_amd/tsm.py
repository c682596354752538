"""Time-domain time-scale modification: `wsola` (waveform-similarity overlap-add, Verhelst & Roelands 1993), `ola` (plain
overlap-add with short frames) and `time_stretch_hpss` (Driedger, Mueller & Ewert 2014: the harmonic part by the phase-locked
vocoder, the percussive part by OLA), two kernel launches (csrc/kernels_wsola.h).  It is what `pytsmod`, `audiotsm`
and the TSM toolbox ship; a phase vocoder, locked or not, smears a click over a whole analysis frame, and a time-domain method
does not.

Inputs

  - `x` is (L,) or (B, L), real.
  - N = `frame_length` is even, 2 <= N <= 2048.
  - Hs = `hop_length` is the synthesis hop, 1 <= Hs <= N, default N // 2.
  - D = `tolerance`, 0 <= D <= 1024, default N // 2.
  - w is a real window of N entries, default `torch.hann_window(N)` (periodic).
  - `rate` > 0 is finite.  `rate` > 1 shortens, as in `time_stretch`.
  - n_out = `length` if given, else ceil(L / rate) (the quotient a float64 quotient).
  - xz(i) = x[i] for 0 <= i < L, else 0.

Frame count.  M = (n_out - 1 + N/2) // Hs + 1 is the number of frames.  These are exactly the frames whose support
[m Hs - N/2, m Hs + N/2) meets [0, n_out).

Analysis centres.  a_m = floor(m Hs rate + 0.5) for m = 0 ... M - 1, made once with NumPy in float64,
`np.floor(np.arange(M) * Hs * rate + 0.5).astype(np.int64)`, and handed to the library as an int64 device array.  The kernels never
evaluate this expression: hipcc contracts a * b + c into an fma by default, and the result would then differ in rare cases.  A
centre array as an input is also what a time-varying rate will need: the C ABI takes any non-decreasing int64 centres, this
module exposes `rate` only.

Lag chain.  del_0 = 0.  For m = 0 ... M - 2, with u_m = a_m + del_m - N/2:

    p[n]      = xz(u_m + Hs + n),  n < N                        (the natural continuation of frame m)
    c[d]      = sum_n xz(a_{m+1} - N/2 + d + n) * p[n],  |d| <= D   (float64 products and sums for both dtypes)
    del_{m+1} = the d with the largest c[d]; among equals the smallest |d|; of +-d the negative one

Overlap-add.  For 0 <= j < n_out, over the frames m in [0, M) with 0 <= n = j - m Hs + N/2 < N, in ascending m, in float64:

    acc[j] = sum_m w[n] * xz(u_m + n)        ow[j] = sum_m w[n]
    y[j]   = acc[j] / (ow[j] if ow[j] >= 1e-3 else 1), rounded once to x's dtype

D = 0 is plain OLA: all lags are 0 and the chain is not run.  ow does not depend on the data.  NaN input is unspecified.  float16
and bfloat16 are computed as float32 and rounded back, as in `hpss`.

    y = si.wsola(x, 0.8)                                                    # 25 % longer, speech and general material
    y, lags = si.wsola(x, 0.8, 1024, 512, 512, return_lags=True)
    y = si.time_stretch_hpss(x, 0.8, n_fft=1024, hop_length=256, window=w)  # tones by the vocoder, clicks by OLA

Not part of the reference's surface.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from ._ingest import ingest, is_int
from .plan import require_gpu
from .timescale import _METHODS, _checked_lock_tol, _checked_rate

__all__ = ["wsola", "ola", "time_stretch_hpss", "wsola_frames", "wsola_centres"]

_MAX_FRAME = 2048
_MAX_TOL = 1024
_REAL = {torch.float16: torch.float32, torch.bfloat16: torch.float32, torch.float32: torch.float32, torch.float64: torch.float64}


def _int_in(value, name, lo, hi, what):
    if not is_int(value):
        raise ValueError(f"{name} must be an int, got {value!r}")
    if value < lo or value > hi:
        raise ValueError(f"{name} must be {what}, got {value}")
    return value


def _checked_frame(frame_length, hop_length, name="frame_length", hop_name="hop_length"):
    n = _int_in(frame_length, name, 2, _MAX_FRAME, f"even, from 2 to {_MAX_FRAME}")
    if n % 2:
        raise ValueError(f"{name} must be even, from 2 to {_MAX_FRAME}, got {n}")
    hop = n // 2 if hop_length is None else _int_in(hop_length, hop_name, 1, n, f"from 1 to {name} = {n}")
    return n, hop


def _checked_window(window, n):
    if window is None:
        return None
    if not isinstance(window, torch.Tensor):
        raise TypeError("window must be a torch.Tensor or None")
    if window.dtype not in _REAL:
        raise TypeError(f"window must be real floating point, got dtype {window.dtype}")
    if window.dim() != 1 or window.shape[0] != n:
        raise ValueError(f"window must hold frame_length = {n} entries, got shape {tuple(window.shape)}")
    return window


def wsola_frames(n_out, frame_length, hop_length):
    """M, the number of frames of `n_out` output samples: (n_out - 1 + N/2) // Hs + 1."""
    return (n_out - 1 + frame_length // 2) // hop_length + 1


def wsola_centres(n_frames, hop_length, rate):
    """The analysis centres a_m = floor(m Hs rate + 0.5), m < n_frames, as the module defines them: an int64 array."""
    a = np.floor(np.arange(n_frames) * hop_length * rate + 0.5)
    return np.clip(a, -2.0 ** 62, 2.0 ** 62).astype(np.int64)         # (beyond either bound every read is outside the row anyway)


def _checked_wave(x, what):
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    if x.dtype not in _REAL:
        raise TypeError(f"x must be float16, bfloat16, float32 or float64, got dtype {x.dtype}")
    if x.dim() not in (1, 2):
        raise ValueError(f"x must be (L,) or (B, L), got shape {tuple(x.shape)}")
    if x.shape[-1] < 1:
        raise ValueError(f"x of shape {tuple(x.shape)} holds no samples")
    if torch.is_grad_enabled() and x.requires_grad:
        raise NotImplementedError(f"{what} is not differentiable; detach the input")


def _run(x, rate, n, hop, tol, window, length, return_lags, what):
    _checked_wave(x, what)
    rate = _checked_rate(rate)
    window = _checked_window(window, n)
    n_in = x.shape[-1]
    if length is None:
        if not n_in / rate < 1 << 62:
            raise ValueError(f"{n_in} samples at rate {rate} stretch beyond 2^62 samples")
        n_out = max(1, math.ceil(n_in / rate))
    else:
        n_out = _int_in(length, "length", 1, (1 << 62) - 1, "from 1 to 2^62 - 1")
    n_frames = wsola_frames(n_out, n, hop)
    if n_frames >= 1 << 31:
        raise ValueError(f"{n_out} samples at hop_length {hop} take {n_frames} frames, beyond 2^31 - 1")
    if x.numel() == 0:
        y = x.new_zeros(x.shape[:-1] + (n_out,))
        return (y, torch.zeros(x.shape[:-1] + (n_frames,), dtype=torch.int32, device=x.device)) if return_lags else y
    device = require_gpu(x.device)
    dtype = _REAL[x.dtype]
    x2 = ingest(x.reshape(-1, n_in), device, dtype)
    # (the default window is made on the CPU: the same bits on every device, and those a caller's own hann_window(N) has)
    w = ingest(torch.hann_window(n, dtype=dtype) if window is None else window, device, dtype)
    centres = torch.from_numpy(wsola_centres(n_frames, hop, rate)).to(device)
    y = torch.empty((x2.shape[0], n_out), dtype=dtype, device=device)
    lags = torch.empty((x2.shape[0], n_frames), dtype=torch.int32, device=device)
    _lib.call_op("specinv_wsola", (x2, centres, w, lags, y, x2.shape[0], n_in, n_out, n_frames, n, hop, tol), dtype != torch.float32,
                 device)
    y = y.reshape(x.shape[:-1] + (n_out,)).to(device=x.device, dtype=x.dtype)
    if not return_lags:
        return y
    return y, lags.reshape(x.shape[:-1] + (n_frames,)).to(x.device)


def wsola(x, rate, frame_length=1024, hop_length=None, tolerance=None, window=None, length=None, return_lags=False):
    r"""A waveform (L,) / (B, L) played `rate` times as fast at the same pitch by waveform-similarity overlap-add: (n_out,) /
    (B, n_out) of `x`'s dtype and device, `n_out = length` if given, else ceil(L / rate).  With `return_lags=True` it returns
    `(y, lags)`, `lags` (..., M) int32: the offset del_m the search gave frame m.  The definition is the module's.

    `frame_length` is even, from 2 to 2048; `hop_length` (default `frame_length // 2`) is the synthesis hop, from 1 to
    `frame_length`; `tolerance` (default `frame_length // 2`, from 0 to 1024) is how far a frame may move from its nominal
    position to line up with the one before it, and 0 is plain overlap-add; `window` is a real tensor of `frame_length` entries
    (default the periodic Hann window).

    Products and sums are float64 for every dtype and the result is rounded once; float16 / bfloat16 are computed as float32 and
    rounded back.  A CPU tensor is computed on the current HIP device and comes back to the CPU.  Any number of items; an empty
    batch returns an empty result.  Not differentiable.
    """
    n, hop = _checked_frame(frame_length, hop_length)
    tol = n // 2 if tolerance is None else tolerance
    tol = _int_in(tol, "tolerance", 0, _MAX_TOL, f"from 0 to {_MAX_TOL}")
    return _run(x, rate, n, hop, tol, window, length, bool(return_lags), "wsola")


def ola(x, rate, frame_length=256, hop_length=None, window=None, length=None):
    """Plain overlap-add: `wsola` with `tolerance=0`, every frame at its nominal position.  With short frames (the default is
    256) it keeps transients sharp and is what percussive material wants; on tonal material it is rough."""
    n, hop = _checked_frame(frame_length, hop_length)
    return _run(x, rate, n, hop, 0, window, length, False, "ola")


def time_stretch_hpss(x, rate, n_fft=None, kernel_size=31, power=2.0, hpss_iter=0, perc_frame=256, perc_hop=None, max_iter=32,
                      method="accelerated_griffin_lim", phase_lock="identity", lock_tol=1e-6, **kwargs):
    r"""A waveform (L,) / (B, L) played `rate` times as fast with its transients kept (Driedger, Mueller & Ewert 2014): the
    harmonic part by the phase-locked vocoder, the percussive part by overlap-add with short frames.  It is exactly

        x_h, x_p = hpss_audio(x, n_fft, kernel_size, power, 1.0, hpss_iter, **kwargs)
        y_h = time_stretch(x_h, rate, n_fft, max_iter, method, phase_lock=phase_lock, lock_tol=lock_tol, **kwargs)
        y_p = ola(x_p, rate, perc_frame, perc_hop, length=y_h.shape[-1])
        return y_h + y_p

    with `phase_lock` "identity" (the default) or "pghi" - the harmonic branch is always locked, `None` is a ValueError - and has `time_stretch`'s length.  `hpss_iter` is `hpss_audio`'s `max_iter` (MISI iterations that make x_h + x_p = x);
    `perc_frame` / `perc_hop` are `ola`'s frame and hop.  `**kwargs` holds the STFT arguments and whatever else `time_stretch`'s
    method takes.  Both branches map output time s to input time s * rate from 0, which holds for centred frames only:
    `center=False` is a ValueError.
    """
    from .hpss import hpss_audio
    from .timescale import time_stretch
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    if x.dtype not in _REAL:
        raise TypeError(f"x must be float16, bfloat16, float32 or float64, got dtype {x.dtype}")
    rate = _checked_rate(rate)
    if method not in _METHODS:
        raise ValueError(f"method must be one of {', '.join(_METHODS)}, got {method!r}")
    if not is_int(max_iter) or max_iter < 0:
        raise ValueError(f"max_iter must be an int >= 0, got {max_iter!r}")
    _checked_frame(perc_frame, perc_hop, "perc_frame", "perc_hop")
    if not kwargs.get("center", True):
        raise ValueError("time_stretch_hpss needs centred frames: with center=False the vocoder's output time 0 is not the input's")
    if not (isinstance(phase_lock, str) and phase_lock in ("identity", "pghi")):
        raise ValueError(f"time_stretch_hpss locks the phase of its harmonic branch: phase_lock must be 'identity' or 'pghi', "
                         f"got {phase_lock!r}")
    lock_tol = _checked_lock_tol(lock_tol)
    if torch.is_grad_enabled() and x.requires_grad:
        raise NotImplementedError("time_stretch_hpss is not differentiable; detach the input")
    x_h, x_p = hpss_audio(x, n_fft, kernel_size, power, 1.0, hpss_iter, **kwargs)
    y_h = time_stretch(x_h, rate, n_fft, max_iter, method, phase_lock=phase_lock, lock_tol=lock_tol, **kwargs)
    y_p = ola(x_p, rate, perc_frame, perc_hop, length=y_h.shape[-1])
    return y_h + y_p
