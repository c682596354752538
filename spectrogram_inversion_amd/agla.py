"""Accelerated Griffin-Lim (AGLA; Peer, Welker & Gerkmann 2022), with gamma = 1 the Fast Griffin-Lim of Perraudin, Balazs &
Soendergaard 2013 that librosa and torchaudio implement: the extrapolation acts on successive *projected* estimates.

With P(x) = ISTFT(S m / (|S| + 1e-16)), S = STFT(x) - one Griffin-Lim iteration without momentum - and c_0 = ISTFT(start):

    n = 1:   t_1 = c_1 = d_1 = P(c_0)
    n > 1:   y = P(c_{n-1}) ;  t_n = (1 - gamma) d_{n-1} + gamma y ;  c_n = t_n + alpha (t_n - t_{n-1}) ;  d_n = t_n + beta (t_n - t_{n-1})

All three sequences are consistent spectrograms, so the library carries them as signals and an iteration is the projection
launch plus one launch over (B, L) samples (`specinv_agla_*`, csrc/kernels_agla.h).  `griffin_lim` keeps the reference's own
recursion (a filter on the spectrum), which is a different method.  Not part of the reference's surface.
"""
from __future__ import annotations

import torch

from . import _lib
from . import methods as _m
from .plan import args_helper, get_plan, require_gpu, trim_plan_cache

__all__ = ["accelerated_griffin_lim"]

# A plan takes at most this many batch items (methods._MAX_PLAN_BATCH); larger batches run as slices (methods._iterative_sliced)
_MAX_PLAN_BATCH = _m._MAX_PLAN_BATCH


def accelerated_griffin_lim(spec, max_iter=200, tol=1e-6, alpha=0.99, beta=None, gamma=1.0, verbose=True, eva_iter=10,
                            metric="sc", **stft_kwargs):
    r"""Waveform (L,) / (B, L) from a spectrogram by Accelerated Griffin-Lim.

    `spec` is a magnitude (F, T) / (B, F, T) tensor - the iteration then starts from `phase_init(spec)` - or a complex one to
    start from (its modulus is the target).  `alpha >= 0`, `beta >= 0` (None: `alpha`) and `gamma > 0` are the method's three
    parameters; the defaults, gamma = 1 at the reference's default momentum, are Fast Griffin-Lim (beta has no effect then),
    alpha = 0 with gamma = 1 is Griffin-Lim without momentum.  `max_iter`, `tol`, `eva_iter`, `metric`, `verbose` and
    `**stft_kwargs` are those of `griffin_lim`.  CPU tensors are computed on the current HIP device and come back to the CPU;
    float16 / bfloat16 are computed in float32 and rounded back.  Not differentiable.
    """
    if not isinstance(spec, torch.Tensor):
        raise TypeError("spec must be a torch.Tensor")
    if spec.dim() not in (2, 3):
        raise ValueError(f"spec must be (F, T) or (B, F, T), got shape {tuple(spec.shape)}")
    if beta is None:
        beta = alpha
    if not alpha >= 0 or not beta >= 0:
        raise ValueError(f"alpha and beta must be >= 0, got {alpha} and {beta}")
    if not gamma > 0:
        raise ValueError(f"gamma must be > 0, got {gamma}")
    assert eva_iter > 0 and max_iter > 0 and tol >= 0
    assert isinstance(metric, str) and metric.upper() in _lib.METRICS
    if torch.is_grad_enabled() and spec.requires_grad:
        raise NotImplementedError("accelerated_griffin_lim is not differentiable; detach the input")
    half = None
    if spec.dtype == torch.bfloat16:
        w = stft_kwargs.get("window")
        if isinstance(w, torch.Tensor) and w.dtype == torch.bfloat16:
            stft_kwargs = dict(stft_kwargs, window=w.float())
        spec, half = spec.float(), torch.bfloat16
    else:
        spec, stft_kwargs, half = _m._widen(spec, stft_kwargs)
    rdtype = spec.real.dtype if spec.is_complex() else spec.dtype
    if rdtype not in (torch.float32, torch.float64):
        raise TypeError(f"spec of dtype {spec.dtype} is not supported (float16 / bfloat16 / float32 / float64 or complex)")
    spec3 = _m._format_spec(spec)
    if spec3.shape[0] < 1 or spec3.shape[2] < 1:
        raise ValueError(f"spec of shape {tuple(spec.shape)} holds no items")
    args = args_helper(spec3, **stft_kwargs)
    _m._no_complex_window(args)
    device = require_gpu(spec3.device)
    if spec3.shape[0] > _MAX_PLAN_BATCH:
        x = _m._iterative_sliced("agla", spec3.to(device), args, device, rdtype, (alpha, beta, gamma), max_iter, tol, verbose,
                                 eva_iter, metric, per=_MAX_PLAN_BATCH)
    else:
        plan = get_plan(args, spec3.shape[0], spec3.shape[2], rdtype, device)
        if spec3.is_complex():
            plan.agla_init(spec3, None, alpha, beta, gamma)        # target = |spec|
        else:
            plan.agla_init(None, spec3, alpha, beta, gamma)        # phase_init on the device
        _m._run_loop(plan, max_iter, tol, verbose, eva_iter, metric)
        x = plan.wave()
    trim_plan_cache()
    if not (spec.shape[0] == 1 and spec.dim() == 3):
        x = x.squeeze(0)                                       # (as griffin_lim: squeeze unless the input was exactly (1, F, T))
    x = x.to(spec.device)
    return x.to(half) if half else x
