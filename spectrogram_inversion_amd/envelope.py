"""Spectral envelopes: `spectral_envelope`, the true-envelope estimator of Roebel & Rodet 2005 in one kernel launch
(csrc/kernels_envelope.h), `impose_envelope`, which makes one waveform carry another's envelope, and
`default_envelope_order` and `envelope_order_for_f0`.  `pitch_shift(..., preserve_formants=True)` is built from them.

`S` is a one-sided spectrogram (F, T) / (B, F, T), real non-negative magnitudes or complex, F = N / 2 + 1 with N = n_fft.  Per
item and frame:

    amin   = floor * max |S| over the item          (an all-zero item: V = 0 everywhere, E = 1)
    a0[k]  = log(max(|S[k]|, amin))
    C(a)   = Re rfft(irfft(a, N) * l),   l[q] = 1 if min(q, N - q) <= order else 0
    V_0    = C(a0);   V_i = C(max(a0, V_{i-1})),  i = 1 ... n_iter
    E      = exp(V_{n_iter})

`a` is real and read as an even sequence of length N, so its cepstrum is real and even: C keeps the `order` lowest quefrencies of
the log-magnitude.  `n_iter = 0` is plain cepstral smoothing, which runs through the middle of the harmonics' peaks and the gaps
between them; every further pass lifts what lies under the envelope up to it and smooths again, so that the envelope climbs onto
the peaks.  `n_iter` is a fixed count, not a stop rule.  `order >= N / 2` is the identity; `order = 0`, `n_iter = 0` is the
constant `(a0[0] + a0[N/2] + 2 sum a0[1 ... N/2-1]) / N`.  NaN input is unspecified.

    E = si.spectral_envelope(si.stft(x, 1024, hop_length=256, window=w), order=si.default_envelope_order(44100))
    y = si.impose_envelope(y, x, 1024, order=73, hop_length=256, window=w)        # y with x's formants
    y = si.pitch_shift(x, 44100, 4, n_fft=1024, hop_length=256, window=w, preserve_formants=True)

Not part of the reference's surface.
"""
from __future__ import annotations

import math
import numbers

import torch

from . import _lib
from ._ingest import ingest
from .plan import _RECOGNISED, require_gpu

__all__ = ["spectral_envelope", "impose_envelope", "default_envelope_order", "envelope_order_for_f0"]

SUPPORTED_N_FFT = (256, 512, 1024, 2048)
MAX_ITER = 256
# dtype -> (the real dtype returned, complex?); float64 / complex128 are not implemented
_KINDS = {torch.float16: (torch.float16, False), torch.bfloat16: (torch.bfloat16, False), torch.float32: (torch.float32, False),
          torch.complex32: (torch.float16, True), torch.complex64: (torch.float32, True)}
_MAX_BLOCKS = 65535            # workgroups one call of the entry point is given: the wrapper slices the items beyond


def envelope_order_for_f0(sample_rate, f0):
    """`max(1, round(sample_rate / (2 f0)))`: the cepstral order whose cut-off quefrency is half the period of a voice at `f0` Hz,
    the true-envelope order of Roebel & Rodet - the envelope then follows the formants and not the harmonics.  `yin` measures
    `f0`; `default_envelope_order(sample_rate)` is this at 300 Hz.  ValueError for an argument that is not a finite number > 0."""
    for name, v in (("sample_rate", sample_rate), ("f0", f0)):
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or not (v > 0 and math.isfinite(v)):
            raise ValueError(f"{name} must be a finite number > 0, got {v!r}")
    return max(1, round(sample_rate / (2 * f0)))


def default_envelope_order(sample_rate):
    """`max(1, round(sample_rate / 600))`, which is `envelope_order_for_f0(sample_rate, 300)`: the cepstral order whose cut-off
    quefrency is half the period of a 300 Hz voice, so that the envelope follows the formants and not the harmonics of voices up
    to about there.  A default, not a tuned value: a higher voice wants a lower order, a bass a higher one - where the pitch can
    be measured, `envelope_order_for_f0` with `yin`'s f0 (or `pitch_shift(..., formant_order="f0")`) gives that order."""
    return envelope_order_for_f0(sample_rate, 300)


def _checked_iter(n_iter, name="n_iter"):
    if isinstance(n_iter, bool) or not isinstance(n_iter, int) or not 0 <= n_iter <= MAX_ITER:
        raise ValueError(f"{name} must be an int in 0 ... {MAX_ITER}, got {n_iter!r}")
    return n_iter


def _checked_order(order, n_fft, name="order"):
    """an int in 0 ... n_fft / 2 (`n_fft=None`: only what can be said without it)"""
    top = "n_fft / 2" if n_fft is None else str(n_fft // 2)
    if isinstance(order, bool) or not isinstance(order, int) or order < 0 or (n_fft is not None and order > n_fft // 2):
        raise ValueError(f"{name} must be an int in 0 ... {top}, got {order!r}")
    return order


def _checked_floor(floor):
    if isinstance(floor, bool) or not isinstance(floor, numbers.Real) or not (floor > 0 and math.isfinite(floor)):
        raise ValueError(f"floor must be a finite number > 0, got {floor!r}")
    return float(floor)


def _checked_gain(max_gain_db):
    if isinstance(max_gain_db, bool) or not isinstance(max_gain_db, numbers.Real) or not (max_gain_db >= 0 and math.isfinite(max_gain_db)):
        raise ValueError(f"max_gain_db must be a finite number >= 0, got {max_gain_db!r}")
    return float(max_gain_db)


def _checked_n_fft(n_freq, dtype, what):
    """NotImplementedError for what the kernel does not cover; the n_fft of `n_freq` one-sided bins otherwise"""
    if dtype in (torch.float64, torch.complex128):
        raise NotImplementedError(f"{what} is implemented in float32: a {dtype} input is not supported")
    if n_freq in SUPPORTED_N_FFT:
        raise NotImplementedError(f"{what} takes a one-sided spectrogram: {n_freq} bins look like a two-sided one of n_fft {n_freq}, "
                                  "which is not supported")
    n_fft = 2 * (n_freq - 1)
    if n_fft not in SUPPORTED_N_FFT:
        raise NotImplementedError(f"{what} supports n_fft {', '.join(map(str, SUPPORTED_N_FFT))} ({n_freq} bins are n_fft {n_fft})")
    return n_fft


def spectral_envelope(spec, order, n_iter=16, floor=1e-6, log=False, frame_major=False):
    r"""The spectral envelope `E` of a one-sided spectrogram (F, T) / (B, F, T), real magnitudes or complex: a real array of its
    shape, real dtype and device, or with `log=True` its logarithm `V`.  The definition is the module's.

    `order` (an int in 0 ... n_fft / 2) is the number of quefrencies kept, `default_envelope_order(sample_rate)` where nothing
    better is known; `n_iter` (0 ... 256) the number of true-envelope passes after the first smoothing; `floor` (> 0) what the
    magnitudes are held above, relative to the item's largest.  With `frame_major=True` the array is (T, F) / (B, T, F), as
    `gla_projection` takes it, and so is the result; the kernel then skips a transpose on either side.

    n_fft 256, 512, 1024 and 2048.  float16 / bfloat16 / complex32 are computed in float32 and rounded back; float64 / complex128,
    two-sided spectrograms and other sizes are a NotImplementedError.  Any layout torch can express is read as torch would read it.
    A CPU tensor is computed on the current HIP device and comes back to the CPU.  Any number of items.  Not differentiable.
    """
    if not isinstance(spec, torch.Tensor):
        raise TypeError("spec must be a torch.Tensor")
    if spec.dtype not in _KINDS and spec.dtype not in (torch.float64, torch.complex128):
        raise TypeError(f"spec must be float16 / bfloat16 / float32 or complex, got dtype {spec.dtype}")
    if spec.dim() not in (2, 3):
        raise ValueError(f"spec must be (F, T) or (B, F, T), got shape {tuple(spec.shape)}")
    n_freq, n_frames = (spec.shape[-1], spec.shape[-2]) if frame_major else (spec.shape[-2], spec.shape[-1])
    if n_freq < 2 or n_frames < 1:
        raise ValueError(f"spec of shape {tuple(spec.shape)} holds no frames")
    if n_frames >= 1 << 31:
        raise ValueError(f"spec of shape {tuple(spec.shape)}: T must be below 2^31")
    _checked_order(order, 2 * (n_freq - 1))
    n_iter, floor = _checked_iter(n_iter), _checked_floor(floor)
    n_fft = _checked_n_fft(n_freq, spec.dtype, "spectral_envelope")
    if torch.is_grad_enabled() and spec.requires_grad:
        raise NotImplementedError("spectral_envelope is not differentiable; detach the input")
    out_dtype, cplx = _KINDS[spec.dtype]
    if spec.numel() == 0:
        return spec.new_zeros(spec.shape, dtype=out_dtype)
    device = require_gpu(spec.device)
    s3 = ingest(spec.reshape((-1,) + tuple(spec.shape[-2:])), device, torch.complex64 if cplx else torch.float32)
    amin = (s3.abs().amax(dim=(1, 2)) * floor).to(torch.float32).contiguous()       # a one-off pass, not the hot path
    out = torch.empty(s3.shape, dtype=torch.float32, device=device)
    tile = 32 if n_fft <= 512 else 16 if n_fft == 1024 else 8                        # frames per workgroup (kernels_envelope.h)
    per_call = max(1, _MAX_BLOCKS // -(-n_frames // tile))                           # items whose workgroups fit one call
    for b0 in range(0, s3.shape[0], per_call):
        nb = min(per_call, s3.shape[0] - b0)
        _lib.call_op("specinv_spectral_envelope", (s3[b0:], out[b0:], amin[b0:], nb, n_freq, n_frames, order, n_iter, int(bool(log)),
                                                   int(cplx), int(bool(frame_major))), False, device)
    return out.reshape(spec.shape).to(device=spec.device, dtype=out_dtype)


def impose_envelope(y, x, n_fft=None, order=None, n_iter=16, floor=1e-6, max_gain_db=40.0, **stft_kwargs):
    r"""Two waveforms of equal shape (L,) / (B, L): `y` carrying the spectral envelope of `x`, a waveform of that shape.  It is
    exactly

        Y, X = stft(y, n_fft, **stft_kwargs), stft(x, n_fft, **stft_kwargs)
        V_y, V_x = spectral_envelope(Y, order, n_iter, floor, log=True), spectral_envelope(X, order, n_iter, floor, log=True)
        G = exp(clamp(V_x - V_y, -g, g)),   g = max_gain_db * ln(10) / 20
        istft(Y * G, **stft_kwargs)

    cropped or zero-padded on the right to L.  The clamp keeps a band that `y` left empty - above the old Nyquist frequency of a
    signal shifted down, say - from being amplified into noise.  `order=None` is `n_fft // 16`, a default for where the
    sampling rate is not known; pass `default_envelope_order(sample_rate)` where it is.  `**stft_kwargs` are `stft`'s
    (`hop_length`, `window`, ...; `n_fft` defaults as there).  The limits of `spectral_envelope` apply.  Not differentiable.
    """
    from . import istft, stft
    if not isinstance(y, torch.Tensor) or not isinstance(x, torch.Tensor):
        raise TypeError("y and x must be torch.Tensors")
    if y.shape != x.shape:
        raise ValueError(f"y and x must have one shape, got {tuple(y.shape)} and {tuple(x.shape)}")
    if y.dtype == torch.float64 or x.dtype == torch.float64:
        raise NotImplementedError("impose_envelope is implemented in float32: a float64 waveform is not supported")
    if order is not None:
        _checked_order(order, None)
    n_iter, floor, max_gain_db = _checked_iter(n_iter), _checked_floor(floor), _checked_gain(max_gain_db)
    if torch.is_grad_enabled() and (y.requires_grad or x.requires_grad):
        raise NotImplementedError("impose_envelope is not differentiable; detach the inputs")
    kw = {k: v for k, v in stft_kwargs.items() if k in _RECOGNISED}
    Y, X = stft(y, n_fft, **kw), stft(x, n_fft, **kw)
    n = _checked_n_fft(Y.shape[-2], Y.dtype, "impose_envelope")
    order = _checked_order(n // 16 if order is None else order, n)
    V = spectral_envelope(torch.stack([Y, X.to(Y.device)]).reshape((-1,) + tuple(Y.shape[-2:])), order, n_iter, floor, log=True)
    V_y, V_x = V.reshape((2,) + tuple(Y.shape)).unbind(0)
    g = max_gain_db * math.log(10.0) / 20.0
    out = istft(Y * torch.exp(torch.clamp(V_x - V_y, -g, g)), **kw)
    length = y.shape[-1]
    if out.shape[-1] >= length:
        return out[..., :length]
    return torch.nn.functional.pad(out, (0, length - out.shape[-1]))
