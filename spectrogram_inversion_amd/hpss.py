"""Harmonic-percussive source separation: `hpss`, the median-filter separation of Fitzgerald 2010 with the margins of Driedger,
Mueller & Disch 2014 (`librosa.decompose.hpss`, `librosa.effects.hpss` / `harmonic` / `percussive`), one kernel launch
(csrc/kernels_hpss.h).

`S` is (F, T) or (B, F, T), real non-negative magnitudes or complex.  Nothing about an STFT is read: the array is filtered as it
stands.

    A = S for a real input, sqrt(re^2 + im^2) evaluated in float64 for a complex one
    refl(i, n) = j if j < n else 2 n - 1 - j,  j = i mod 2 n            (Python's mod)
    harm[f, t] = median{ A[f, refl(t + d, T)] : |d| <= k_h // 2 }       (a sustained tone is a horizontal line: kept)
    perc[f, t] = median{ A[refl(f + d, F), t] : |d| <= k_p // 2 }       (a click is a vertical line: kept)

The sizes are odd, so a median is an element of its window; for a real input `harm` and `perc` hold input elements bit for bit.
With margins m_h, m_p >= 1, a power p > 0 and split = (m_h == 1 and m_p == 1),

    soft(X, R):  Z = max(X, R);  Z < tiny: 0.5 if split else 0;  otherwise a = (X / Z)^p, r = (R / Z)^p and a / (a + r)
                 p = inf: 1 if X > R else 0, whatever Z is
    M_h = soft(harm, m_h * perc),   M_p = soft(perc, m_p * harm),   H = S * M_h,   P = S * M_p

`tiny` is the smallest normal number of the input's real dtype (float32's for the halves).  From Z on everything is float64 for
every dtype and the result is rounded once; p = 1 and p = 2 are products, not pow.  With both margins 1 the masks sum to 1 and
H + P = S.  NaN input is unspecified.

This is `librosa.decompose.hpss` with `librosa.util.softmask`, with three deviations: an even kernel size is a ValueError (scipy
moves the window off centre for those), sizes above 127 are a ValueError, and the reflection is continued periodically, so a window
wider than twice its axis is defined (scipy's own extension is not: `median_filter([1., 2.], size=17, mode='reflect')` is zeros).

    H, P = si.hpss(si.stft(x, 1024, hop_length=256, window=w))                       # two spectrograms, H + P = S
    x_h, x_p = si.hpss_audio(x, 1024, hop_length=256, window=w)                      # two waveforms
    x_h, x_p = si.hpss_audio(x, 1024, max_iter=8, hop_length=256, window=w)          # ... made consistent by MISI: x_h + x_p = x

Not part of the reference's surface.
"""
from __future__ import annotations

import math
import numbers

import torch

from . import _lib
from ._ingest import ingest
from .plan import _RECOGNISED, require_gpu

__all__ = ["hpss", "hpss_medians", "hpss_audio", "harmonic", "percussive"]

_MAX_SIZE = 127
# dtype -> (the real dtype computed in, complex?)
_KINDS = {torch.float16: (torch.float32, False), torch.bfloat16: (torch.float32, False), torch.float32: (torch.float32, False),
          torch.float64: (torch.float64, False), torch.complex32: (torch.float32, True), torch.complex64: (torch.float32, True),
          torch.complex128: (torch.float64, True)}
_REAL_OF = {torch.complex32: torch.float16, torch.complex64: torch.float32, torch.complex128: torch.float64}


def _pair(value, name):
    if isinstance(value, (tuple, list)):
        if len(value) != 2:
            raise ValueError(f"{name} must be a scalar or a (harmonic, percussive) pair, got {value!r}")
        return value[0], value[1]
    return value, value


def _checked_sizes(kernel_size):
    sizes = _pair(kernel_size, "kernel_size")
    for k in sizes:
        if isinstance(k, bool) or not isinstance(k, int):
            raise ValueError(f"kernel_size must be an int or a pair of ints, got {kernel_size!r}")
        if k < 1 or k > _MAX_SIZE or k % 2 == 0:
            raise ValueError(f"a kernel size must be odd, from 1 to {_MAX_SIZE}, got {k}")
    return sizes


def _checked_margins(margin):
    margins = _pair(margin, "margin")
    for m in margins:
        if isinstance(m, bool) or not isinstance(m, numbers.Real) or not (m >= 1 and math.isfinite(m)):
            raise ValueError(f"a margin must be a finite number >= 1, got {m!r}")
    return float(margins[0]), float(margins[1])


def _checked_power(power):
    if isinstance(power, bool) or not isinstance(power, numbers.Real) or not power > 0:
        raise ValueError(f"power must be a number > 0 (inf is allowed), got {power!r}")
    return float(power)


def _checked_spec(spec, what):
    if not isinstance(spec, torch.Tensor):
        raise TypeError("spec must be a torch.Tensor")
    if spec.dtype not in _KINDS:
        raise TypeError(f"spec must be float16 / bfloat16 / float32 / float64 or complex, got dtype {spec.dtype}")
    if spec.dim() not in (2, 3):
        raise ValueError(f"spec must be (F, T) or (B, F, T), got shape {tuple(spec.shape)}")
    if spec.shape[-1] < 1 or spec.shape[-2] < 1:
        raise ValueError(f"spec of shape {tuple(spec.shape)} holds no bins")
    if spec.shape[-1] >= 1 << 31 or spec.shape[-2] >= 1 << 31:
        raise ValueError(f"spec of shape {tuple(spec.shape)}: F and T must be below 2^31")
    if torch.is_grad_enabled() and spec.requires_grad:
        raise NotImplementedError(f"{what} is not differentiable; detach the input")


def _run(spec, sizes, power, margins, mode):
    """One launch: the two outputs of `mode` in the caller's shape and device, real (float16 / bfloat16 for those inputs) unless
    the mode is the components of a complex input."""
    rdtype, cplx = _KINDS[spec.dtype]
    out_cplx = cplx and mode == _lib.HPSS_COMPONENTS
    out_dtype = spec.dtype if out_cplx or not cplx else _REAL_OF[spec.dtype]
    if spec.numel() == 0:
        return spec.new_zeros(spec.shape, dtype=out_dtype), spec.new_zeros(spec.shape, dtype=out_dtype)
    device = require_gpu(spec.device)
    work = (torch.complex64 if rdtype == torch.float32 else torch.complex128) if cplx else rdtype
    s3 = ingest(spec.reshape((-1,) + tuple(spec.shape[-2:])), device, work)
    out_work = work if out_cplx else rdtype
    out_a = torch.empty(s3.shape, dtype=out_work, device=device)
    out_b = torch.empty(s3.shape, dtype=out_work, device=device)
    _lib.call_op("specinv_hpss", (s3, out_a, out_b, s3.shape[0], s3.shape[1], s3.shape[2], sizes[0], sizes[1], power, margins[0],
                                  margins[1], mode, int(cplx)), rdtype != torch.float32, device)
    return tuple(o.reshape(spec.shape).to(device=spec.device, dtype=out_dtype) for o in (out_a, out_b))


def hpss(spec, kernel_size=31, power=2.0, mask=False, margin=1.0):
    r"""The harmonic and the percussive component `(H, P)` of a spectrogram (F, T) / (B, F, T), each of its shape, dtype and device:
    `H = S * M_h`, `P = S * M_p` (real components for real magnitudes, complex for a complex input), or with `mask=True` the masks
    `(M_h, M_p)` themselves in the real dtype.  The definition is the module's.

    `kernel_size` is the width of the two median filters, an odd int from 1 to 127 or a `(harmonic, percussive)` pair: the first
    runs along time, the second along frequency.  `margin` (>= 1, a scalar or such a pair) is what a component has to exceed the
    other by; with a margin above 1 the components no longer sum to the input, and what neither claims is the residual.  `power` > 0
    is the exponent of the soft mask; `float('inf')` gives binary masks.

    float16 / bfloat16 / complex32 are computed as float32 / complex64 and rounded back.  A CPU tensor is computed on the current HIP
    device and comes back to the CPU.  Any number of items.  Not differentiable.
    """
    _checked_spec(spec, "hpss")
    sizes, power, margins = _checked_sizes(kernel_size), _checked_power(power), _checked_margins(margin)
    return _run(spec, sizes, power, margins, _lib.HPSS_MASKS if mask else _lib.HPSS_COMPONENTS)


def hpss_medians(spec, kernel_size=31):
    r"""`(harm, perc)`: the spectrogram's magnitude median-filtered along time and along frequency, the two enhanced spectrograms the
    masks of `hpss` are made from, in the real dtype.  Every value is an element of its window: for a real input the result holds
    input elements bit for bit, for a complex one the float64 magnitude rounded once.  Arguments and rules are those of `hpss`."""
    _checked_spec(spec, "hpss_medians")
    return _run(spec, _checked_sizes(kernel_size), 1.0, (1.0, 1.0), _lib.HPSS_MEDIANS)


def hpss_audio(x, n_fft=None, kernel_size=31, power=2.0, margin=1.0, max_iter=0, **kwargs):
    r"""A waveform (L,) / (B, L) split into its harmonic and its percussive part `(x_h, x_p)`, waveforms of the length `istft` gives
    the frame count of `x`.

    With `max_iter=0` it is exactly

        H, P = hpss(stft(x, n_fft, **stft_kwargs), kernel_size, power, False, margin)
        istft(H, **stft_kwargs), istft(P, **stft_kwargs)

    and with `max_iter > 0` exactly `misi(torch.stack([H, P], -3), x, max_iter=max_iter, **kwargs)` unbound along the source axis:
    MISI starts from the two masked spectrograms, makes each a consistent spectrogram and keeps `x_h + x_p = x[..., :L]`.  That needs
    both margins equal to 1 - otherwise H + P is not the input's spectrogram and the constraint would be wrong: a ValueError.
    `**kwargs` holds the STFT arguments (`hop_length`, `window`, ...; `n_fft` defaults as in `stft`) and, with `max_iter > 0`, whatever
    else `misi` takes (`tol`, `verbose`, `eva_iter`, `metric`).  Not differentiable.
    """
    from . import istft, misi, stft
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    sizes, power, margins = _checked_sizes(kernel_size), _checked_power(power), _checked_margins(margin)
    if isinstance(max_iter, bool) or not isinstance(max_iter, int) or max_iter < 0:
        raise ValueError(f"max_iter must be an int >= 0, got {max_iter!r}")
    if max_iter > 0 and margins != (1.0, 1.0):
        raise ValueError(f"max_iter > 0 needs both margins equal to 1, got {margins}: with a larger margin the two components do "
                         "not sum to the input and MISI's mixture constraint would be wrong")
    if torch.is_grad_enabled() and x.requires_grad:
        raise NotImplementedError("hpss_audio is not differentiable; detach the input")
    stft_kwargs = {k: v for k, v in kwargs.items() if k in _RECOGNISED}
    H, P = hpss(stft(x, n_fft, **stft_kwargs), sizes, power, False, margins)
    if max_iter == 0:
        return istft(H, **stft_kwargs), istft(P, **stft_kwargs)
    y = misi(torch.stack([H, P], -3), x, max_iter=max_iter, **kwargs)
    return y.unbind(-2)


def harmonic(x, n_fft=None, kernel_size=31, power=2.0, margin=1.0, max_iter=0, **kwargs):
    """The harmonic part of a waveform: the first of `hpss_audio`'s pair, with its arguments."""
    return hpss_audio(x, n_fft, kernel_size, power, margin, max_iter, **kwargs)[0]


def percussive(x, n_fft=None, kernel_size=31, power=2.0, margin=1.0, max_iter=0, **kwargs):
    """The percussive part of a waveform: the second of `hpss_audio`'s pair, with its arguments."""
    return hpss_audio(x, n_fft, kernel_size, power, margin, max_iter, **kwargs)[1]
