"""Accelerated Griffin-Lim (AGLA; Peer, Welker & Gerkmann 2022), with gamma = 1 the Fast Griffin-Lim of Perraudin, Balazs &
Soendergaard 2013 that librosa and torchaudio implement: the extrapolation acts on successive *projected* estimates.

With P(x) = ISTFT(S m / (|S| + 1e-16)), S = STFT(x) - one Griffin-Lim iteration without momentum - and c_0 = ISTFT(start):

    n = 1:   t_1 = c_1 = d_1 = P(c_0)
    n > 1:   y = P(c_{n-1}) ;  t_n = (1 - gamma) d_{n-1} + gamma y ;  c_n = t_n + alpha (t_n - t_{n-1}) ;  d_n = t_n + beta (t_n - t_{n-1})

All three sequences are consistent spectrograms, so the library carries them as signals and an iteration is the projection
launch plus one launch over (B, L) samples (`specinv_agla_*`, csrc/kernels_agla.h).  `griffin_lim` keeps the reference's own
recursion (a filter on the spectrum), which is a different method.  `agla_unfolded` is a fixed number of these iterations as a
differentiable layer whose alpha, beta, gamma may differ per iteration and be learned (csrc/kernels_agla_adjoint.h).  Not part of
the reference's surface.
"""
from __future__ import annotations

import torch

from . import _lib
from ._ingest import ingest
from . import methods as _m
from .autograd import _input_grad
from .plan import args_helper, get_plan, require_gpu, trim_plan_cache

__all__ = ["accelerated_griffin_lim", "agla_unfolded"]

# A plan takes at most this many batch items (methods._MAX_PLAN_BATCH); larger batches run as slices (methods._iterative_sliced)
_MAX_PLAN_BATCH = _m._MAX_PLAN_BATCH

def _prepare(spec, stft_kwargs):
    """The checked spectrogram in the form the plan takes, all that needs no device: (spec3 (B, F, T), args, rdtype, half) -
    float16 / bfloat16 widened to float32 (`half`: the dtype to return), a batch axis added where absent."""
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
    return spec3, args, rdtype, half


def _finish(x, spec, half):
    """(B, L) on the device -> the caller's shape, device and dtype."""
    if not (spec.shape[0] == 1 and spec.dim() == 3):
        x = x.squeeze(0)                                       # (as griffin_lim: squeeze unless the input was exactly (1, F, T))
    x = x.to(spec.device)
    return x.to(half) if half else x


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
    spec3, args, rdtype, half = _prepare(spec, stft_kwargs)
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
    return _finish(x, spec, half)


def _schedule(name, value, n_iter):
    """One of alpha, beta, gamma as a (n_iter,) float64 CPU tensor, the graph to a tensor that requires grad kept."""
    if isinstance(value, torch.Tensor):
        if value.is_complex() or value.dtype == torch.bool:
            raise TypeError(f"{name} must be real, got dtype {value.dtype}")
        if value.numel() not in (1, n_iter):
            raise ValueError(f"{name} must hold 1 or n_iter = {n_iter} elements, got shape {tuple(value.shape)}")
        t = value.reshape(-1).to(device="cpu", dtype=torch.float64)
    elif isinstance(value, (int, float)) and not isinstance(value, bool):
        t = torch.tensor([float(value)], dtype=torch.float64)
    else:
        raise TypeError(f"{name} must be a float or a tensor, got {type(value).__name__}")
    return t.expand(n_iter)


def _schedules(n_iter, alpha, beta, gamma):
    """The checked `n_iter` and parameters of an unfolded layer: alpha, beta (None: alpha), gamma as (n_iter,) float64 CPU tensors
    and their values as three lists."""
    if isinstance(n_iter, bool) or not isinstance(n_iter, int) or n_iter < 1:
        raise ValueError(f"n_iter must be an integer >= 1, got {n_iter!r}")
    al = _schedule("alpha", alpha, n_iter)
    be = al if beta is None else _schedule("beta", beta, n_iter)
    ga = _schedule("gamma", gamma, n_iter)
    sched = [t.detach().tolist() for t in (al, be, ga)]
    if not all(v >= 0 for v in sched[0] + sched[1]):
        raise ValueError(f"alpha and beta must be >= 0, got {sched[0]} and {sched[1]}")
    if not all(v > 0 for v in sched[2]):
        raise ValueError(f"gamma must be > 0, got {sched[2]}")
    return al, be, ga, sched


def _sweep(plan, t, sched, g_y, mag_fm, fixed_mask=None, goff=None):
    """The backward sweep of an unfolded layer over the recorded signals t[0] = c_0, t[n] = t_n: one `specinv_agla_step_adjoint`
    for n = N ... 2, the closing step and the ISTFT's adjoint.  With `goff` (batch, length), which gains the cotangent of the
    constraint's offset, the constrained sweep (`specinv_cgla_*`) under the bool mask `fixed_mask` of known samples, or None.
    Returns the cotangent of the start's spectrogram, of the frame-major magnitudes `mag_fm` and the (N, 3) gradients of alpha_n,
    beta_n, gamma_n on the device."""
    al, be, ga = sched
    n_iter = len(al)
    gm_fm = torch.zeros_like(mag_fm)
    a = g_y.detach().to(plan.dtype).clone(memory_format=torch.contiguous_format)   # (the sweep works in place)
    gc = torch.zeros_like(a)
    gd = torch.zeros_like(a) if any(g != 1.0 for g in ga) else None                # (every gamma = 1: gd stays 0)
    c_prev = torch.empty_like(a)
    dots = torch.zeros((n_iter, 3), dtype=torch.float64, device=plan.device)       # row 0: iteration 1 does not extrapolate
    w8 = None if fixed_mask is None else fixed_mask.to(torch.uint8)                # (the kernel's form of the mask, once)
    for n in range(n_iter, 1, -1):
        step = (t[n], t[n - 1], t[n - 2] if n > 2 else None, (al[n - 1], be[n - 1], ga[n - 1], al[n - 2], be[n - 2]))
        if goff is None:
            plan.agla_step_adjoint(*step, a, gc, gd, c_prev, dots[n - 1], mag_fm, gm_fm)
        else:
            plan.cgla_step_adjoint(*step, w8, a, gc, gd, goff, c_prev, dots[n - 1], mag_fm, gm_fm)
    if goff is None:
        plan.agla_first_adjoint(t[0], a, gc, gd, mag_fm, gm_fm)
    else:
        plan.cgla_first_adjoint(t[0], w8, a, gc, gd, goff, mag_fm, gm_fm)
    return plan.istft_adjoint(gc), gm_fm, dots


class _AglaUnfoldedFn(torch.autograd.Function):
    """`n_iter` AGLA iterations as one differentiable layer.  The forward pass is the inference kernels with c_0 = ISTFT(start) and
    t_1 ... t_N recorded, (N + 1) B L reals; the backward sweep recomputes c_{n-1} and d_{n-1} from the t's and runs one
    `specinv_agla_step_adjoint` per iteration (csrc/kernels_agla_adjoint.h), which also leaves the gradients of alpha_n, beta_n,
    gamma_n in a row of a device tensor that is read once."""

    @staticmethod
    def forward(ctx, spec3, alpha, beta, gamma, plan, n_iter):
        ctx.real_in = not spec3.is_complex()
        start = ingest(spec3, plan.device, plan.dtype if ctx.real_in else plan.cdtype)
        sched = [t.detach().tolist() for t in (alpha, beta, gamma)]
        if ctx.real_in:
            plan.agla_init_sched(None, start, *sched)              # phase_init on the device
        else:
            plan.agla_init_sched(start, None, *sched)              # target = |spec|
        waves = []
        for _ in range(n_iter):
            waves.append(plan.wave())                              # c_0 = ISTFT(start), then t_1 ... t_{N-1}
            plan.agla_iterate(1)
        y = plan.wave()
        ctx.plan, ctx.sched = plan, sched
        ctx.save_for_backward(start, y, *waves)
        return y

    @staticmethod
    def backward(ctx, g_y):
        plan = ctx.plan
        start, y, *t = ctx.saved_tensors
        t.append(y)                                                # t[0] = c_0, t[n] = t_n
        mag = start if ctx.real_in else start.abs()
        mag_fm = mag.transpose(1, 2).contiguous()                  # frame-major once, not once per iteration
        g_c0, gm_fm, dots = _sweep(plan, t, ctx.sched, g_y, mag_fm)
        g_spec = _input_grad(ctx, plan, mag, start, g_c0, gm_fm.transpose(1, 2).contiguous())
        g_par = dots.cpu() if any(ctx.needs_input_grad[1:4]) else None
        return (g_spec, *(g_par[:, k] if ctx.needs_input_grad[1 + k] else None for k in range(3)), None, None)


def agla_unfolded(spec, n_iter=5, alpha=0.99, beta=None, gamma=1.0, **stft_kwargs):
    r"""`n_iter` iterations of Accelerated Griffin-Lim as a layer to train through, its three parameters learnable per iteration.

    `spec`, `**stft_kwargs`, the start, shapes, dtypes and devices are those of `accelerated_griffin_lim`; there is no stop rule,
    the result is t_N.  `alpha`, `beta` (None: `alpha`, whose gradient then also takes beta's) and `gamma` are each a float, a
    tensor with one element or a real tensor with `n_iter` elements, on any device; element n - 1 belongs to iteration n.  Iteration
    1 does not extrapolate: element 0 has no effect and receives a zero gradient.  Every alpha and beta must be >= 0, every gamma
    > 0.  Without a gradient to compute and with constant parameters the result is `accelerated_griffin_lim(spec,
    max_iter=n_iter, tol=0, verbose=False, alpha=..., beta=..., gamma=...)`.  With grad mode on and `spec` or a parameter requiring
    grad, the same kernels run and the result carries gradients to `spec` (magnitudes: through the target and through
    `phase_init`; a complex start: through the start and its modulus, the target) and to each parameter tensor, in its dtype and on
    its device.  With every gamma = 1 (Fast Griffin-Lim) beta has no effect and its gradient is exactly 0.  At most 65535 items.
    """
    if not isinstance(spec, torch.Tensor):
        raise TypeError("spec must be a torch.Tensor")
    if spec.dim() not in (2, 3):
        raise ValueError(f"spec must be (F, T) or (B, F, T), got shape {tuple(spec.shape)}")
    al, be, ga, sched = _schedules(n_iter, alpha, beta, gamma)
    spec3, args, rdtype, half = _prepare(spec, stft_kwargs)
    if spec3.shape[0] > _MAX_PLAN_BATCH:
        raise ValueError(f"spec of shape {tuple(spec.shape)} holds {spec3.shape[0]} items, agla_unfolded takes at most {_MAX_PLAN_BATCH}")
    grad = torch.is_grad_enabled() and (spec.requires_grad or al.requires_grad or be.requires_grad or ga.requires_grad)
    if not grad and all(len(set(v)) == 1 for v in sched):
        return accelerated_griffin_lim(spec, max_iter=n_iter, tol=0, verbose=False, alpha=sched[0][0], beta=sched[1][0],
                                       gamma=sched[2][0], **stft_kwargs)
    device = require_gpu(spec3.device)
    plan = get_plan(args, spec3.shape[0], spec3.shape[2], rdtype, device)
    if grad:
        x = _AglaUnfoldedFn.apply(spec3.to(device), al, be, ga, plan, n_iter)
    else:
        start = spec3.detach().to(device)
        plan.agla_init_sched(*((start, None) if start.is_complex() else (None, start)), *sched)
        plan.agla_iterate(n_iter)
        x = plan.wave()
    trim_plan_cache()
    return _finish(x, spec, half)
