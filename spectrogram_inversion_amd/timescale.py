"""Time-scale modification: the phase vocoder, and `time_stretch`, which refines the vocoder's phase with the package's own
iteration.

Griffin & Lim 1984 and RTISI-LA (Zhu, Beauregard & Wyse 2007) were published for this: a spectrogram is resampled along time and
a signal is estimated from the modified spectrogram.  `phase_vocoder` is the resampling (`librosa.phase_vocoder`,
`torchaudio.functional.phase_vocoder`), one kernel launch (csrc/kernels_pvoc.h).  For output frame j of `T_out`, with
t_j = j * rate, i = floor(t_j), a = t_j - i and the frames at and beyond T read as zeros,

    |P[j]| = a |S[i+1]| + (1 - a) |S[i]| ;   arg P[0] = arg S[0] ;   arg P[j+1] = arg P[j] + wrap(arg S[i+1] - arg S[i] - adv) + adv

with adv = 2 pi k hop / n_fft the advance bin k expects over one hop (k signed above n_fft / 2) and wrap(x) = x - 2 pi round(x / 2 pi).
Everything after the two angles, the running sum included, is float64 whatever the input's dtype.

The vocoder's output is far from a consistent spectrogram (|STFT(ISTFT(P))| misses |P| by 0.4 in relative L2), which is why
`time_stretch` does not stop there: it starts `accelerated_griffin_lim` (or `griffin_lim`, `ADMM`) from P.

    y = si.time_stretch(x, 0.8, n_fft=1024, hop_length=256, window=w)                  # 25 % longer
    P = si.phase_vocoder(si.stft(x, 1024, hop_length=256, window=w), 0.8, hop_length=256, window=w)

`pitch_shift` is the other half of the pair (`librosa.effects.pitch_shift`, `torchaudio.functional.pitch_shift`): `time_stretch` by
2^(-n_steps / bins_per_octave), then `resample` (resample.py) back to the original rate and length.

    z = si.pitch_shift(x, 22050, 4, n_fft=1024, hop_length=256, window=w)              # four semitones up, as long as x

Not part of the reference's surface.
"""
from __future__ import annotations

import dataclasses
import math
import numbers

import torch

from . import methods as _m
from .plan import _RECOGNISED, args_helper, get_plan, require_gpu, trim_plan_cache
from .projection import _COMPLEX, _check_items

__all__ = ["phase_vocoder", "time_stretch", "stretched_frames", "pitch_shift"]

_METHODS = ("accelerated_griffin_lim", "griffin_lim", "ADMM")
_MAX_FRAMES = 2147483000


def _checked_rate(rate):
    if isinstance(rate, bool) or not isinstance(rate, numbers.Real):
        raise ValueError(f"rate must be a float, got {type(rate).__name__}")
    rate = float(rate)
    if not (rate > 0 and math.isfinite(rate)):
        raise ValueError(f"rate must be finite and > 0, got {rate}")
    return rate


def stretched_frames(n_frames, rate):
    """The frame count `phase_vocoder` gives `n_frames` frames at `rate`: the smallest n >= 1 with float(n) * rate >= n_frames,
    the product a float64 product (what `specinv_phase_vocoder` checks its plan against)."""
    rate = _checked_rate(rate)
    n_frames = int(n_frames)
    if n_frames < 1:
        raise ValueError(f"n_frames must be >= 1, got {n_frames}")
    if not n_frames / rate < _MAX_FRAMES:
        raise ValueError(f"{n_frames} frames at rate {rate} stretch beyond {_MAX_FRAMES} frames")
    n = max(1, math.ceil(n_frames / rate))
    while n > 1 and float(n - 1) * rate >= n_frames:
        n -= 1
    while float(n) * rate < n_frames:
        n += 1
    return n


def _checked_lock(phase_lock):
    if phase_lock is not None and not (isinstance(phase_lock, str) and phase_lock == "identity"):
        raise ValueError(f"phase_lock must be None or 'identity', got {phase_lock!r}")
    return phase_lock


def phase_vocoder(spec, rate, phase_lock=None, **stft_kwargs):
    r"""A complex spectrogram (F, T) / (B, F, T) resampled along time by the phase vocoder: (F, T_out) / (B, F, T_out) complex of
    the same dtype and device, `T_out = stretched_frames(T, rate)`.  `rate > 1` shortens, `rate < 1` lengthens.

    `**stft_kwargs` are those the spectrogram was computed with, as everywhere (`hop_length` and `onesided` are what is read).
    The phase is accumulated in float64 for every dtype and the result rounded once; complex32 is computed as complex64 and
    rounded back.  A CPU tensor is computed on the current HIP device and comes back to the CPU.  Frames beyond the last read as
    zeros, as in librosa and torchaudio.  Not differentiable.  At most 65535 items.

    `phase_lock=None` moves every bin's phase on its own.  `phase_lock="identity"` is identity phase locking (Laroche & Dolson
    1999; csrc/kernels_pvoc_lock.h): a bin is a peak of its frame when its squared magnitude exceeds that of its
    four neighbours, every bin follows the nearest peak, and around a peak the phase differences of the analysis frame are kept.
    The magnitude is the same.  On tonal input the locked result is two to seven times closer to a consistent spectrogram before
    any iteration; on noise it gains little and can lose.  One more launch, and batch * F * T_out doubles held by the plan.
    """
    _checked_lock(phase_lock)
    if not isinstance(spec, torch.Tensor):
        raise TypeError("spec must be a torch.Tensor")
    if spec.dtype not in _COMPLEX:
        raise TypeError(f"spec must be complex, got dtype {spec.dtype} (the phase vocoder reads the phase)")
    rate = _checked_rate(rate)
    if spec.dim() not in (2, 3):
        raise ValueError(f"spec must be (F, T) or (B, F, T), got shape {tuple(spec.shape)}")
    if torch.is_grad_enabled() and spec.requires_grad:
        raise NotImplementedError("phase_vocoder is not differentiable; detach the input")
    spec3 = spec.unsqueeze(0) if spec.dim() == 2 else spec
    if spec3.shape[1] < 1 or spec3.shape[2] < 1:
        raise ValueError(f"spec of shape {tuple(spec.shape)} holds no frames")
    _check_items(spec3.shape[0], "phase_vocoder", f"spec of shape {tuple(spec.shape)}")
    n_out = stretched_frames(spec3.shape[2], rate)
    spec3, stft_kwargs, half = _m._widen(spec3, stft_kwargs)
    args = args_helper(spec3, **stft_kwargs)
    if spec3.shape[0] == 0:
        return spec.new_zeros((0, spec3.shape[1], n_out))
    device = require_gpu(spec3.device)
    if args.signal_length(n_out) < 1:
        # one centred frame (rate >= T) stands for no sample, and no plan can be made for that; the vocoder reads neither the
        # centring nor the window, so its plan is the uncentred one of the same shape (nothing can invert such a result anyway)
        args = dataclasses.replace(args, center=False)
    plan = get_plan(args, spec3.shape[0], n_out, spec3.real.dtype, device)
    out = plan.phase_vocoder(spec3.detach().to(device), rate, phase_lock)
    trim_plan_cache()
    if spec.dim() == 2:
        out = out.squeeze(0)
    out = out.to(spec.device)
    return out.to(torch.complex32) if half else out


def time_stretch(x, rate, n_fft=None, max_iter=32, method="accelerated_griffin_lim", phase_lock=None, **kwargs):
    r"""A waveform (L,) / (B, L) played `rate` times as fast at the same pitch: a waveform of about L / rate samples.

    It is exactly

        method(phase_vocoder(stft(x, n_fft, **stft_kwargs), rate, phase_lock, **stft_kwargs), max_iter=max_iter, **kwargs)

    with `method` one of "accelerated_griffin_lim" (the default: Fast Griffin-Lim at its default parameters), "griffin_lim" and
    "ADMM", started from the vocoder's phase with the vocoder's magnitude as the target.  `**kwargs` holds the STFT arguments
    (`hop_length`, `window`, `win_length`, `center`, ...; `n_fft` defaults as in `stft`) and whatever else the method takes
    (`tol`, `verbose`, `eva_iter`, `alpha`, ...), each with the method's own default.  `max_iter=0` is `istft` of the vocoder's
    output, the classic phase vocoder; with `phase_lock="identity"` (see `phase_vocoder`) that is usable on tonal material.  Locking
    is worth the first few iterations there; after five or more the two starts end within 13 % of each other.

    The result holds the samples `istft` gives `stretched_frames(T, rate)` frames, (T_out - 1) * hop_length with `center=True`: it
    is not padded or trimmed to round(L / rate).  dtype and device rules are those of `stft` and the method.
    """
    from . import ADMM, accelerated_griffin_lim, griffin_lim, istft, stft
    if method not in _METHODS:
        raise ValueError(f"method must be one of {', '.join(_METHODS)}, got {method!r}")
    rate = _checked_rate(rate)
    _checked_lock(phase_lock)
    if isinstance(max_iter, bool) or not isinstance(max_iter, int) or max_iter < 0:
        raise ValueError(f"max_iter must be an int >= 0, got {max_iter!r}")
    stft_kwargs = {k: v for k, v in kwargs.items() if k in _RECOGNISED}
    P = phase_vocoder(stft(x, n_fft, **stft_kwargs), rate, phase_lock, **stft_kwargs)
    if max_iter == 0:
        return istft(P, **stft_kwargs)
    run = {"accelerated_griffin_lim": accelerated_griffin_lim, "griffin_lim": griffin_lim, "ADMM": ADMM}[method]
    return run(P, max_iter=max_iter, **kwargs)


def shift_rate(sample_rate, n_steps, bins_per_octave=12):
    """(rate, orig) of `pitch_shift`: the rate `time_stretch` runs at, 2^(-n_steps / bins_per_octave), and the sampling rate
    int(sample_rate / rate) its result is read at, which `resample` then converts back to `sample_rate` (torchaudio's two lines)."""
    if isinstance(sample_rate, bool) or not isinstance(sample_rate, int) or sample_rate < 1:
        raise ValueError(f"sample_rate must be an int >= 1, got {sample_rate!r}")
    if isinstance(n_steps, bool) or not isinstance(n_steps, numbers.Real) or not math.isfinite(n_steps):
        raise ValueError(f"n_steps must be a finite number, got {n_steps!r}")
    if isinstance(bins_per_octave, bool) or not isinstance(bins_per_octave, int) or bins_per_octave < 1:
        raise ValueError(f"bins_per_octave must be an int >= 1, got {bins_per_octave!r}")
    try:
        rate = 2.0 ** (-float(n_steps) / bins_per_octave)
        orig = int(sample_rate / rate)
    except (OverflowError, ZeroDivisionError):
        rate, orig = 0.0, 0
    if not (rate > 0 and math.isfinite(rate) and orig >= 1):
        raise ValueError(f"{n_steps} steps of {bins_per_octave} per octave at {sample_rate} Hz leave no sampling rate to convert from")
    return rate, orig


def pitch_shift(x, sample_rate, n_steps, bins_per_octave=12, n_fft=None, max_iter=32, method="accelerated_griffin_lim",
                lowpass_filter_width=6, rolloff=0.99, phase_lock=None, **kwargs):
    r"""A waveform (L,) / (B, L) sampled at `sample_rate` raised by `n_steps` steps of `bins_per_octave` to the octave (a real
    number: fractional and negative steps are valid) at the same duration: a waveform of the same shape.

    It is exactly, with (rate, orig) = shift_rate(sample_rate, n_steps, bins_per_octave),

        y = time_stretch(x, rate, n_fft=n_fft, max_iter=max_iter, method=method, phase_lock=phase_lock, **kwargs)
        if orig != sample_rate:
            y = resample(y, orig, sample_rate, lowpass_filter_width, rolloff)

    and then y[..., :L], zero-padded on the right to L where it is shorter - torchaudio's definition, its phase vocoder refined by
    `method`.  `**kwargs` are `time_stretch`'s; dtype and device rules are `time_stretch`'s and `resample`'s.
    """
    from .resample import resample
    rate, orig = shift_rate(sample_rate, n_steps, bins_per_octave)
    _checked_lock(phase_lock)
    y = time_stretch(x, rate, n_fft=n_fft, max_iter=max_iter, method=method, phase_lock=phase_lock, **kwargs)
    if orig != sample_rate:
        y = resample(y, orig, sample_rate, lowpass_filter_width, rolloff)
    n = x.shape[-1]
    if y.shape[-1] >= n:
        return y[..., :n]
    return torch.nn.functional.pad(y, (0, n - y.shape[-1]))
