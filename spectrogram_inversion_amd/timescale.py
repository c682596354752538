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

`phase_lock="identity"` (csrc/kernels_pvoc_lock.h) and `phase_lock="pghi"` (csrc/kernels_pvoc_pghi.h) keep the
phase coherent across the bins of a frame: around the nearest spectral peak, or along the magnitude-ordered heap of "phase vocoder
done right" (Prusa & Holighaus 2017), which also helps on noisy and transient input.

`pitch_shift` is the other half of the pair (`librosa.effects.pitch_shift`, `torchaudio.functional.pitch_shift`): `time_stretch` by
2^(-n_steps / bins_per_octave), then `resample` (resample.py) back to the original rate and length.

    z = si.pitch_shift(x, 22050, 4, n_fft=1024, hop_length=256, window=w)              # four semitones up, as long as x
    z = si.pitch_shift(x, 22050, 4, n_fft=1024, hop_length=256, window=w, preserve_formants=True)   # ... with x's formants (envelope.py)

Not part of the reference's surface.
"""
from __future__ import annotations

import dataclasses
import math
import numbers

import torch

from . import _lib
from . import methods as _m
from ._ingest import ingest
from .plan import _RECOGNISED, args_helper, get_plan, require_gpu, trim_plan_cache
from .projection import _COMPLEX, _check_items

__all__ = ["phase_vocoder", "time_stretch", "stretched_frames", "pitch_shift"]

_METHODS = ("accelerated_griffin_lim", "griffin_lim", "ADMM")
_MAX_FRAMES = 2147483000
_LOCKS = ("identity", "pghi")
_PGHI_MAX_FREQ = 2915         # the bins a workgroup of the "pghi" kernel holds: rtpghi's bound


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
    if phase_lock is not None and not (isinstance(phase_lock, str) and phase_lock in _LOCKS):
        raise ValueError(f"phase_lock must be None, 'identity' or 'pghi', got {phase_lock!r}")
    return phase_lock


def _checked_lock_tol(lock_tol):
    if isinstance(lock_tol, bool) or not isinstance(lock_tol, numbers.Real) or not 0 < lock_tol < 1:
        raise ValueError(f"lock_tol must be a finite number in (0, 1), got {lock_tol!r}")
    return float(lock_tol)


def _pvoc_pghi(spec3, rate, n_out, lock_tol, return_parents, stft_kwargs):
    """`phase_lock="pghi"` on (B, F, T), B >= 1: `specinv_pvoc_pghi`, stateless - no plan is made."""
    args = args_helper(spec3, **stft_kwargs)
    if not args.onesided:
        raise NotImplementedError("phase_lock='pghi' takes one-sided spectrograms only")
    if spec3.shape[1] > _PGHI_MAX_FREQ:
        raise NotImplementedError(f"phase_lock='pghi': {spec3.shape[1]} bins are beyond the kernel's limit of {_PGHI_MAX_FREQ}")
    device = require_gpu(spec3.device)
    real = spec3.real.dtype
    s = ingest(spec3, device, spec3.dtype)
    out = torch.empty((s.shape[0], s.shape[1], n_out), dtype=s.dtype, device=device)
    parents = torch.empty(out.shape, dtype=torch.int8, device=device) if return_parents else None
    _lib.call_op("specinv_pvoc_pghi", (s, out, parents, s.shape[0], s.shape[1], s.shape[2], n_out, args.n_fft, args.hop_length, rate,
                                       lock_tol), real != torch.float32, device)
    return out, parents


def phase_vocoder(spec, rate, phase_lock=None, lock_tol=1e-6, return_parents=False, **stft_kwargs):
    r"""A complex spectrogram (F, T) / (B, F, T) resampled along time by the phase vocoder: (F, T_out) / (B, F, T_out) complex of
    the same dtype and device, `T_out = stretched_frames(T, rate)`.  `rate > 1` shortens, `rate < 1` lengthens.

    `**stft_kwargs` are those the spectrogram was computed with, as everywhere (`hop_length` and `onesided` are what is read).
    The phase is accumulated in float64 for every dtype and the result rounded once; complex32 is computed as complex64 and
    rounded back.  A CPU tensor is computed on the current HIP device and comes back to the CPU.  Frames beyond the last read as
    zeros, as in librosa and torchaudio.  Not differentiable.  At most 65535 items (any number with `phase_lock="pghi"`).

    `phase_lock=None` moves every bin's phase on its own.  `phase_lock="identity"` is identity phase locking (Laroche & Dolson
    1999; csrc/kernels_pvoc_lock.h): a bin is a peak of its frame when its squared magnitude exceeds that of its
    four neighbours, every bin follows the nearest peak, and around a peak the phase differences of the analysis frame are kept.
    The magnitude is the same.  On tonal input the locked result is two to seven times closer to a consistent spectrogram before
    any iteration; on noise it gains little and can lose.  One more launch, and batch * F * T_out doubles held by the plan.

    `phase_lock="pghi"` is the phase vocoder with heap-integrated phase (Prusa & Holighaus 2017, "phase vocoder done right";
    csrc/kernels_pvoc_pghi.h): identity locking in which a bin follows the root of its magnitude-ordered heap chain
    - a bin is a root when its own magnitude in the previous output frame beats the widest path from its neighbours - and a root
    continues from the locked phase of the previous output frame.  It helps on noisy and transient input too, where identity
    locking does not.  Bins below `lock_tol` (finite, 0 < lock_tol < 1; read by this mode only) times the item's largest input
    magnitude keep their own phase and own no other bin.  One launch, no plan, any number of items; one-sided spectrograms of
    at most 2915 bins; the magnitude is formed as sqrt(re^2 + im^2) and may differ from the other modes' by one rounding.
    `return_parents=True` (this mode only) returns `(P, parents)`, `parents` int8 of P's shape: 0 the bin's own previous frame,
    1 from bin k - 1, 2 from bin k + 1, 3 below the floor.
    """
    _checked_lock(phase_lock)
    lock_tol = _checked_lock_tol(lock_tol)
    if return_parents and phase_lock != "pghi":
        raise ValueError("return_parents is valid only with phase_lock='pghi'")
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
    if phase_lock != "pghi":                                   # (no plan there: the grid loops over any number of items)
        _check_items(spec3.shape[0], "phase_vocoder", f"spec of shape {tuple(spec.shape)}")
    n_out = stretched_frames(spec3.shape[2], rate)
    spec3, stft_kwargs, half = _m._widen(spec3, stft_kwargs)
    if phase_lock == "pghi":
        if spec3.shape[0] == 0:
            out, parents = spec.new_zeros((0, spec3.shape[1], n_out)), spec.new_zeros((0, spec3.shape[1], n_out), dtype=torch.int8)
        else:
            out, parents = _pvoc_pghi(spec3.detach(), rate, n_out, lock_tol, bool(return_parents), stft_kwargs)
            if spec.dim() == 2:
                out = out.squeeze(0)
                parents = parents.squeeze(0) if return_parents else None
            out = out.to(spec.device)
            out = out.to(torch.complex32) if half else out
        return (out, parents.to(spec.device)) if return_parents else out
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


def time_stretch(x, rate, n_fft=None, max_iter=32, method="accelerated_griffin_lim", phase_lock=None, lock_tol=1e-6, **kwargs):
    r"""A waveform (L,) / (B, L) played `rate` times as fast at the same pitch: a waveform of about L / rate samples.

    It is exactly

        method(phase_vocoder(stft(x, n_fft, **stft_kwargs), rate, phase_lock, lock_tol, **stft_kwargs), max_iter=max_iter, **kwargs)

    with `method` one of "accelerated_griffin_lim" (the default: Fast Griffin-Lim at its default parameters), "griffin_lim" and
    "ADMM", started from the vocoder's phase with the vocoder's magnitude as the target.  `**kwargs` holds the STFT arguments
    (`hop_length`, `window`, `win_length`, `center`, ...; `n_fft` defaults as in `stft`) and whatever else the method takes
    (`tol`, `verbose`, `eva_iter`, `alpha`, ...), each with the method's own default.  `max_iter=0` is `istft` of the vocoder's
    output, the classic phase vocoder; with `phase_lock="identity"` (see `phase_vocoder`) that is usable on tonal material.  Locking
    is worth the first few iterations there; after five or more the two starts end within 13 % of each other.  `phase_lock="pghi"`
    with its `lock_tol` is the heap-integrated vocoder, which gives the better start on noisy and transient material as well.

    The result holds the samples `istft` gives `stretched_frames(T, rate)` frames, (T_out - 1) * hop_length with `center=True`: it
    is not padded or trimmed to round(L / rate).  dtype and device rules are those of `stft` and the method.
    """
    from . import ADMM, accelerated_griffin_lim, griffin_lim, istft, stft
    if method not in _METHODS:
        raise ValueError(f"method must be one of {', '.join(_METHODS)}, got {method!r}")
    rate = _checked_rate(rate)
    _checked_lock(phase_lock)
    lock_tol = _checked_lock_tol(lock_tol)
    if isinstance(max_iter, bool) or not isinstance(max_iter, int) or max_iter < 0:
        raise ValueError(f"max_iter must be an int >= 0, got {max_iter!r}")
    stft_kwargs = {k: v for k, v in kwargs.items() if k in _RECOGNISED}
    P = phase_vocoder(stft(x, n_fft, **stft_kwargs), rate, phase_lock, lock_tol, **stft_kwargs)
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
                lowpass_filter_width=6, rolloff=0.99, phase_lock=None, lock_tol=1e-6, preserve_formants=False, formant_order=None,
                formant_iter=16, **kwargs):
    r"""A waveform (L,) / (B, L) sampled at `sample_rate` raised by `n_steps` steps of `bins_per_octave` to the octave (a real
    number: fractional and negative steps are valid) at the same duration: a waveform of the same shape.

    It is exactly, with (rate, orig) = shift_rate(sample_rate, n_steps, bins_per_octave),

        y = time_stretch(x, rate, n_fft=n_fft, max_iter=max_iter, method=method, phase_lock=phase_lock, lock_tol=lock_tol, **kwargs)
        if orig != sample_rate:
            y = resample(y, orig, sample_rate, lowpass_filter_width, rolloff)

    and then y[..., :L], zero-padded on the right to L where it is shorter - torchaudio's definition, its phase vocoder refined by
    `method`.  `**kwargs` are `time_stretch`'s; dtype and device rules are `time_stretch`'s and `resample`'s.

    That moves the formants with the pitch: a voice raised by four steps is a smaller head.  With `preserve_formants=True` the
    result z of the above keeps the spectral envelope of `x`; it is exactly

        impose_envelope(z, x, n_fft, formant_order or default_envelope_order(sample_rate), formant_iter, **stft_kwargs)

    (envelope.py) with the STFT arguments among `**kwargs`: `formant_order` is the cepstral order of the envelope (an int in
    0 ... n_fft / 2; None or 0: the default for the sampling rate, a guess for a 300 Hz voice) and `formant_iter` the number of
    true-envelope passes (0 ... 256).  `formant_order="f0"` measures the pitch instead: with

        f0, voiced, _ = yin(x, sample_rate, fmin=sample_rate / 1000, fmax=sample_rate / 20, frame_length=2048)

    (pitch.py) the order is `min(n_fft // 2, envelope_order_for_f0(sample_rate, median of f0[voiced]))` over the whole batch - one
    more launch and one read-back - and the default where no frame is voiced; with `preserve_formants=False` nothing is computed.
    Preserving costs two more STFTs, two envelopes and an inverse STFT, and `spectral_envelope`'s limits apply (float32,
    n_fft 256 ... 2048, one-sided).  With the default `False` nothing changes.
    """
    from .envelope import _checked_iter, _checked_order, default_envelope_order, impose_envelope
    from .resample import resample
    rate, orig = shift_rate(sample_rate, n_steps, bins_per_octave)
    _checked_lock(phase_lock)
    lock_tol = _checked_lock_tol(lock_tol)
    if isinstance(formant_order, str):
        if formant_order != "f0":
            raise ValueError(f'formant_order must be an int, None or "f0", got {formant_order!r}')
    elif formant_order is not None:
        w = kwargs.get("window")
        n = n_fft or kwargs.get("win_length") or (w.numel() if isinstance(w, torch.Tensor) else None)      # (as stft reads them)
        _checked_order(formant_order, n if isinstance(n, int) and not isinstance(n, bool) else None, "formant_order")
    _checked_iter(formant_iter, "formant_iter")
    y = time_stretch(x, rate, n_fft=n_fft, max_iter=max_iter, method=method, phase_lock=phase_lock, lock_tol=lock_tol, **kwargs)
    if orig != sample_rate:
        y = resample(y, orig, sample_rate, lowpass_filter_width, rolloff)
    n = x.shape[-1]
    y = y[..., :n] if y.shape[-1] >= n else torch.nn.functional.pad(y, (0, n - y.shape[-1]))
    if not preserve_formants:
        return y
    stft_kwargs = {k: v for k, v in kwargs.items() if k in _RECOGNISED}
    if formant_order == "f0":
        formant_order = _order_from_f0(x, sample_rate, n_fft, stft_kwargs)
    return impose_envelope(y, x, n_fft, formant_order or default_envelope_order(sample_rate), formant_iter, **stft_kwargs)


def _order_from_f0(x, sample_rate, n_fft, stft_kwargs):
    """`formant_order="f0"`: the envelope order for the median f0 of the voiced frames of the whole batch (one read-back), at most
    n_fft // 2; the default order where no frame is voiced"""
    from .envelope import default_envelope_order, envelope_order_for_f0
    from .pitch import yin
    f0, voiced, _ = yin(x, sample_rate, fmin=sample_rate / 1000, fmax=sample_rate / 20, frame_length=2048)
    # (the median of f0[voiced] without the read-back a boolean index costs: one .item() in all; NaN where nothing is voiced)
    median = torch.where(voiced, f0, torch.full_like(f0, math.nan)).nanmedian().item() if f0.numel() else math.nan
    if math.isnan(median):
        return default_envelope_order(sample_rate)
    w = stft_kwargs.get("window")
    n = n_fft or stft_kwargs.get("win_length") or (w.numel() if isinstance(w, torch.Tensor) else None)      # (as stft reads them)
    order = envelope_order_for_f0(sample_rate, median)
    return min(n // 2, order) if isinstance(n, int) and not isinstance(n, bool) else order
