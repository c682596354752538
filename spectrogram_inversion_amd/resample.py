"""Sample-rate conversion: `resample`, the windowed-sinc interpolation of `torchaudio.functional.resample` (its default
`sinc_interp_hann`), one kernel launch (csrc/kernels_resample.h).

With o : n the ratio orig_freq : new_freq reduced by its greatest common divisor, base = min(o, n) * rolloff,
W = lowpass_filter_width and x read as zero outside 0 ... L - 1, output m of L_out = ceil(n L / o) is

    y[m] = (base / o) * sum over s with |tau| < W of  sinc(tau) * cos^2(pi tau / (2 W)) * x[s],
    tau = base * (s n - m o) / (o n),   sinc(t) = sin(pi t) / (pi t).

An output reads at most 2 ceil(W o / base) + 1 samples.  The weights are generated on the fly, in float64 for every dtype: there is
no filter bank to build, and nothing depends on how the ratio reduces (27781 : 22050, four semitones at 22.05 kHz, costs what 5 : 4
costs).  `timescale.pitch_shift` is `time_stretch` followed by this.

    y = si.resample(x, 48000, 44100)

Not part of the reference's surface.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from ._ingest import ingest, is_int
from .plan import require_gpu

__all__ = ["resample"]

_REAL = {torch.float16: torch.float32, torch.float32: torch.float32, torch.float64: torch.float64}
_MAX_INDEX = 1 << 62          # the kernel forms m * o for every output m in 64 bits
_MAX_HALF_WIDTH = 1 << 30


def _checked_int(value, name):
    if not is_int(value):
        raise ValueError(f"{name} must be an int, got {type(value).__name__}")
    if value < 1:
        raise ValueError(f"{name} must be >= 1, got {value}")
    return value


def _checked_filter(lowpass_filter_width, rolloff):
    _checked_int(lowpass_filter_width, "lowpass_filter_width")
    if lowpass_filter_width >= 1 << 31:
        raise ValueError(f"lowpass_filter_width must be below 2^31, got {lowpass_filter_width}")
    if isinstance(rolloff, bool) or not isinstance(rolloff, (int, float)) or not 0 < rolloff <= 1:
        raise ValueError(f"rolloff must be a number in (0, 1], got {rolloff!r}")
    return lowpass_filter_width, float(rolloff)


def resample(x, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    r"""A waveform (L,) / (B, L) sampled at `orig_freq` converted to `new_freq`: (L_out,) / (B, L_out) of the same dtype and
    device, `L_out = ceil(n L / o)` in integer arithmetic.  The definition is the module's; `lowpass_filter_width` (an int
    >= 1) is the filter's half-width in zero crossings and `rolloff` in (0, 1] the cut-off as a share of the lower Nyquist frequency,
    both torchaudio's, with its defaults.

    Weights and sum are float64 for every dtype and the result is rounded once; float16 is computed as float32 and rounded back.
    A CPU tensor is computed on the current HIP device and comes back to the CPU.  Equal rates return a copy.  Any number of
    items.  Not differentiable.
    """
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    if x.dtype not in _REAL:
        raise TypeError(f"x must be float16, float32 or float64, got dtype {x.dtype}")
    o, n = _checked_int(orig_freq, "orig_freq"), _checked_int(new_freq, "new_freq")
    width, rolloff = _checked_filter(lowpass_filter_width, rolloff)
    if x.dim() not in (1, 2):
        raise ValueError(f"x must be (L,) or (B, L), got shape {tuple(x.shape)}")
    if torch.is_grad_enabled() and x.requires_grad:
        raise NotImplementedError("resample is not differentiable; detach the input")
    g = math.gcd(o, n)
    o, n = o // g, n // g
    n_in = x.shape[-1]
    n_out = -((-n * n_in) // o)
    if n_out * o >= _MAX_INDEX:
        raise ValueError(f"{n_in} samples at {o}:{n} index beyond 62 bits")
    if math.ceil(width * o / (min(o, n) * rolloff)) >= _MAX_HALF_WIDTH:
        raise ValueError(f"{o}:{n} at lowpass_filter_width {width} reads more than 2^31 samples per output")
    if o == n:
        return x.detach().clone()
    if x.numel() == 0 or n_out == 0:
        return x.new_zeros(x.shape[:-1] + (n_out,))
    device = require_gpu(x.device)
    dtype = _REAL[x.dtype]
    x2 = ingest(x.reshape(-1, n_in), device, dtype)
    out = torch.empty((x2.shape[0], n_out), dtype=dtype, device=device)
    _lib.call_op("specinv_resample", (x2, out, x2.shape[0], n_in, n_out, o, n, width, rolloff), dtype != torch.float32, device)
    return out.reshape(x.shape[:-1] + (n_out,)).to(device=x.device, dtype=x.dtype)
