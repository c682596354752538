"""Accelerated Griffin-Lim for a target that is only partly unknown: the complex value of some bins is given (bandwidth extension,
packet-loss concealment, spectrogram inpainting, a noisy phase kept where it is reliable), and so may be some samples of the
signal (time-domain inpainting).

With M the mask of known bins, K their values and m the magnitude target, the constrained amplitude projection
Y = where(M, K, S m / (|S| + 1e-16)) followed by the ISTFT is, the STFT being linear,

    ISTFT(S m' / (|S| + 1e-16)) + k,    m' = where(M, 0, m),  k = ISTFT(where(M, K, 0)):

the projection launch of `accelerated_griffin_lim` with zeros in its magnitude operand, plus a constant signal made once.  A known
sample is one more select on the same (B, L) signal.  An iteration stays the projection launch plus one launch over the samples
(`specinv_agla_constrain`, csrc/kernels_agla.h); no state of the spectrogram's size exists.  `constrained_unfolded` is a fixed
number of these iterations as a differentiable layer (csrc/kernels_agla_adjoint.h).  Not part of the reference's surface.
"""
from __future__ import annotations

import torch
from tqdm import tqdm

from . import _lib
from ._ingest import ingest
from . import methods as _m
from .agla import _finish, _prepare, _schedules, _sweep, accelerated_griffin_lim, agla_unfolded
from .autograd import _input_grad
from .metrics import _from_sums
from .plan import get_plan, require_gpu, trim_plan_cache

__all__ = ["constrained_griffin_lim", "constrained_unfolded"]

_MAX_PLAN_BATCH = _m._MAX_PLAN_BATCH


def _together(name_v, v, name_m, mask):
    """The two members of a (values, mask) pair come together, as tensors, the mask bool; True when the pair is given."""
    if v is None and mask is None:
        return False
    if v is None or mask is None:
        raise ValueError(f"{name_v} and {name_m} come together, got only {name_m if v is None else name_v}")
    if not isinstance(v, torch.Tensor) or not isinstance(mask, torch.Tensor):
        raise TypeError(f"{name_v} and {name_m} must be torch.Tensors")
    if mask.dtype != torch.bool:
        raise TypeError(f"{name_m} must be a bool tensor, got dtype {mask.dtype}")
    return True


def _expanded(name_v, v, name_m, mask, shape):
    """`mask` expanded to `shape`, which `v` must have."""
    if tuple(v.shape) != tuple(shape):
        raise ValueError(f"{name_v} must have shape {tuple(shape)}, got {tuple(v.shape)}")
    try:
        return torch.broadcast_to(mask, tuple(shape))
    except RuntimeError:
        raise ValueError(f"{name_m} of shape {tuple(mask.shape)} does not broadcast to {tuple(shape)}") from None


def _begin(plan, spec3, known_spec, spec_mask, known_wave, wave_mask, alpha, beta, gamma):
    """The plan in the AGLA state under the constraint, before the first iteration: the start with the known bins put in, zeros in
    the magnitude operand under the mask, offset = where(W, xk, ISTFT(where(M, K, 0))) handed to the plan.  Either pair may be None;
    the masks are bool and of their values' shapes.  `alpha`, `beta`, `gamma` are floats or, a schedule, sequences of one length
    (`Plan.agla_init_sched`).  Returns m_full (B, F, T), the target of the evaluation."""
    dev, shape = plan.device, (plan.batch, plan.length)
    init = plan.agla_init_sched if isinstance(alpha, (list, tuple)) else plan.agla_init
    spec3 = spec3.detach().to(dev)
    m = spec3.abs() if spec3.is_complex() else spec3
    if known_spec is not None:
        M = spec_mask.to(dev).reshape(spec3.shape)
        K = known_spec.detach().to(device=dev, dtype=plan.cdtype).reshape(spec3.shape)
        m_full = torch.where(M, K.abs(), m)
        start = torch.where(M, K, spec3 if spec3.is_complex() else plan.phase_init(m_full))
        offset = plan.istft(torch.where(M, K, torch.zeros_like(K)))
        init(start, torch.where(M, torch.zeros_like(m), m), alpha, beta, gamma)
    else:
        m_full = m
        offset = torch.zeros(shape, dtype=plan.dtype, device=dev)
        init(spec3 if spec3.is_complex() else None, m, alpha, beta, gamma)
    W = None
    if known_wave is not None:
        W = wave_mask.to(dev).reshape(shape)
        offset = torch.where(W, known_wave.detach().to(device=dev, dtype=plan.dtype).reshape(shape), offset)
    plan.agla_constrain(offset, W)
    return m_full


def _evaluate(plan, m_full, name):
    """(metric, mse) of |STFT(t_n)| against the full target: one STFT."""
    s = plan.metric_sums(plan.stft(plan.wave()).abs(), m_full)
    return _from_sums(name, s), s[0] / s[3]


def _loop(plan, m_full, max_iter, tol, verbose, eva_iter, metric):
    """The reference's `_training_loop` (torch_specinv/methods.py:153-190) on `_evaluate`, with the bar of `methods._run_loop`.
    Returns (iterations done, [(iteration, metric, loss), ...])."""
    name = metric.upper()
    done, init_loss, previous, evals = 0, None, None, []
    with tqdm(total=max_iter, disable=not verbose) as pbar:
        while done < max_iter:
            until = eva_iter - (done % eva_iter)
            if done + until > max_iter:
                plan.agla_iterate(max_iter - done)
                done = max_iter
                break
            plan.agla_iterate(until)
            done += until
            m, loss = _evaluate(plan, m_full, name)
            evals.append((done - 1, m, loss))
            pbar.set_postfix(**{name: m}, loss=loss)
            pbar.update(eva_iter)
            if not init_loss:
                init_loss = loss
            elif (previous - loss) / init_loss < tol and previous > loss:
                break
            previous = loss
    return done, evals


def constrained_griffin_lim(spec, known_spec=None, spec_mask=None, known_wave=None, wave_mask=None, max_iter=200, tol=1e-6,
                            alpha=0.99, beta=None, gamma=1.0, verbose=True, eva_iter=10, metric="sc", **stft_kwargs):
    r"""Waveform (L,) / (B, L) by Accelerated Griffin-Lim with the complex value of some bins and / or some samples given.

    `spec`, `alpha`, `beta`, `gamma`, `max_iter`, `tol`, `eva_iter`, `metric`, `verbose` and `**stft_kwargs` are those of
    `accelerated_griffin_lim`; a complex `spec` is the start.  `known_spec` is complex and of `spec`'s shape, `spec_mask` bool and
    broadcastable to it, true where the bin's complex value is given: the values of `spec` there are ignored, the target is
    `|known_spec|`, and every iteration's amplitude projection puts `known_spec` in.  `known_wave` is real, (L,) / (B, L) with L
    the signal length of `spec`'s frames, `wave_mask` bool and broadcastable to it, true where the sample is given: the result
    holds `known_wave` there bit for bit.  Each pair is optional, its two members come together; with neither this is
    `accelerated_griffin_lim`.  Two-sided spectra are accepted; a mask that is not Hermitian-symmetric gives what `istft` gives
    for such a spectrum (the real part of its inverse transform).

    With P the momentum-free projection onto m' = where(M, 0, m), k = ISTFT(where(M, K, 0)) and xk the known wave:

        n = 1:  t_1 = where(W, xk, P(c_0) + k) ;  c_1 = d_1 = t_1           (c_0 = ISTFT(start), the known bins put in)
        n > 1:  u = P(c_{n-1}) + k ;  t_n = where(W, xk, (1 - gamma) d_{n-1} + gamma u)
                c_n = t_n + alpha (t_n - t_{n-1}) ;  d_n = t_n + beta (t_n - t_{n-1})

    The result is t_n.  The stop rule and the bar are `griffin_lim`'s, on |STFT(t_n)| against the full target every `eva_iter`
    iterations: that costs one STFT per `eva_iter` iterations beside them.  CPU tensors are computed on the current HIP device
    and come back to the CPU; float16 / bfloat16 are computed in float32 and rounded back.  Not differentiable; at most 65535
    items.
    """
    if not isinstance(spec, torch.Tensor):
        raise TypeError("spec must be a torch.Tensor")
    if spec.dim() not in (2, 3):
        raise ValueError(f"spec must be (F, T) or (B, F, T), got shape {tuple(spec.shape)}")
    has_spec = _together("known_spec", known_spec, "spec_mask", spec_mask)
    has_wave = _together("known_wave", known_wave, "wave_mask", wave_mask)
    if has_spec and not known_spec.is_complex():
        raise TypeError(f"known_spec must be complex, got dtype {known_spec.dtype}")
    if has_wave and (known_wave.is_complex() or known_wave.dtype == torch.bool):
        raise TypeError(f"known_wave must be real, got dtype {known_wave.dtype}")
    if has_spec:
        spec_mask = _expanded("known_spec", known_spec, "spec_mask", spec_mask, spec.shape)
    if not has_spec and not has_wave:
        return accelerated_griffin_lim(spec, max_iter=max_iter, tol=tol, alpha=alpha, beta=beta, gamma=gamma, verbose=verbose,
                                       eva_iter=eva_iter, metric=metric, **stft_kwargs)
    if beta is None:
        beta = alpha
    if not alpha >= 0 or not beta >= 0:
        raise ValueError(f"alpha and beta must be >= 0, got {alpha} and {beta}")
    if not gamma > 0:
        raise ValueError(f"gamma must be > 0, got {gamma}")
    assert eva_iter > 0 and max_iter > 0 and tol >= 0
    assert isinstance(metric, str) and metric.upper() in _lib.METRICS
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (spec, known_spec, known_wave)):
        raise NotImplementedError("constrained_griffin_lim is not differentiable; detach the inputs")
    spec3, args, rdtype, half = _prepare(spec, stft_kwargs)
    batch, _, n_frames = spec3.shape
    length = args.signal_length(n_frames)
    if has_wave:
        wave_mask = _expanded("known_wave", known_wave, "wave_mask", wave_mask, (length,) if spec.dim() == 2 else (batch, length))
    if batch > _MAX_PLAN_BATCH:
        raise ValueError(f"spec of shape {tuple(spec.shape)} holds {batch} items, constrained_griffin_lim takes at most {_MAX_PLAN_BATCH}")
    device = require_gpu(spec3.device)
    plan = get_plan(args, batch, n_frames, rdtype, device)
    m_full = _begin(plan, spec3, known_spec if has_spec else None, spec_mask, known_wave if has_wave else None, wave_mask,
                    alpha, beta, gamma)
    _loop(plan, m_full, max_iter, tol, verbose, eva_iter, metric)
    x = plan.wave()
    plan.agla_constrain(None)                                  # (the cached plan gives the constraint's memory back)
    trim_plan_cache()
    return _finish(x, spec, half)


class _CglaUnfoldedFn(torch.autograd.Function):
    """`n_iter` constrained AGLA iterations as one differentiable layer, `_AglaUnfoldedFn` under the constraint.  The forward pass is
    the inference kernels with c_0 = ISTFT(start) and t_1 ... t_N recorded, (N + 1) B L reals; the backward sweep runs one
    `specinv_cgla_step_adjoint` per iteration (csrc/kernels_agla_adjoint.h), which also accumulates the cotangent of the constant
    signal where(W, xk, k), and splits that and the start's between `spec`, `known_spec` and `known_wave` once at the end."""

    @staticmethod
    def forward(ctx, spec3, K, xk, alpha, beta, gamma, M, W, plan, n_iter):
        ctx.real_in = not spec3.is_complex()
        start = ingest(spec3, plan.device, plan.dtype if ctx.real_in else plan.cdtype)
        if K is not None:
            K = ingest(K, plan.device, plan.cdtype)
        sched = [t.detach().tolist() for t in (alpha, beta, gamma)]
        _begin(plan, start, K, M, xk, W, *sched)
        waves = []
        for _ in range(n_iter):
            waves.append(plan.wave())                              # c_0 = ISTFT(start), then t_1 ... t_{N-1}
            plan.agla_iterate(1)
        y = plan.wave()
        plan.agla_constrain(None)
        ctx.plan, ctx.sched, ctx.M, ctx.W = plan, sched, M, W
        ctx.has_K = K is not None
        ctx.save_for_backward(start, y, *waves, *(() if K is None else (K,)))
        return y

    @staticmethod
    def backward(ctx, g_y):
        plan, M, W = ctx.plan, ctx.M, ctx.W
        start, y, *t = ctx.saved_tensors
        K = t.pop() if ctx.has_K else None
        t.append(y)                                                # t[0] = c_0, t[n] = t_n
        m = start if ctx.real_in else start.abs()
        m_full, m_free = m, m
        if K is not None:
            absK = K.abs()
            m_full, m_free = torch.where(M, absK, m), torch.where(M, torch.zeros_like(m), m)
        mag_fm = m_free.transpose(1, 2).contiguous()               # frame-major once, not once per iteration
        goff = torch.zeros((plan.batch, plan.length), dtype=plan.dtype, device=plan.device)
        g_start, gm_fm, dots = _sweep(plan, t, ctx.sched, g_y, mag_fm, W, goff)
        gm = gm_fm.transpose(1, 2).contiguous()
        g_xk = None if W is None else torch.where(W, goff, torch.zeros_like(goff))
        g_K = None
        if K is not None:
            zero = torch.zeros_like(g_start)
            g_k = goff if W is None else torch.where(W, torch.zeros_like(goff), goff)
            g_K = torch.where(M, plan.istft_adjoint(g_k) + g_start, zero)             # k and the start under M
            g_start = torch.where(M, zero, g_start)
            gm = torch.where(M, torch.zeros_like(gm), gm)                              # (the operand holds zeros there)
        g_spec = _input_grad(ctx, plan, m_full, start, g_start, gm)
        if K is not None and ctx.real_in:                          # phase_init(m_full) reads |K| under M
            unit = torch.where(absK > 0, K / absK, torch.zeros_like(K))
            g_K = g_K + torch.where(M, g_spec, torch.zeros_like(g_spec)) * unit
            g_spec = torch.where(M, torch.zeros_like(g_spec), g_spec)
        need = ctx.needs_input_grad
        g_par = dots.cpu() if any(need[3:6]) else None
        return (g_spec if need[0] else None, g_K if need[1] else None, g_xk if need[2] else None,
                *(g_par[:, k] if need[3 + k] else None for k in range(3)), None, None, None, None)


def constrained_unfolded(spec, known_spec=None, spec_mask=None, known_wave=None, wave_mask=None, n_iter=5, alpha=0.99, beta=None,
                         gamma=1.0, **stft_kwargs):
    r"""`n_iter` iterations of `constrained_griffin_lim` as a layer to train through: waveform (L,) / (B, L).

    `spec`, the two (values, mask) pairs, their shapes, broadcasting, dtypes and devices are those of `constrained_griffin_lim`;
    `n_iter`, `alpha`, `beta`, `gamma` those of `agla_unfolded` (each a float or a tensor of 1 or `n_iter` elements on any device,
    element n - 1 for iteration n, element 0 without effect; `beta=None` is `alpha`).  There is no stop rule and no evaluation: the
    result is t_N of the recursion in `constrained_griffin_lim`'s docstring with alpha_n, beta_n, gamma_n.  With neither pair this
    is `agla_unfolded`; without a gradient to compute and with constant parameters it is `constrained_griffin_lim(...,
    max_iter=n_iter, tol=0, verbose=False)`.  With grad mode on and `spec`, `known_spec`, `known_wave` or a parameter tensor
    requiring grad, the same kernels run and the result carries gradients to `spec` (magnitudes: through the target off the mask
    and through `phase_init`; a complex start: through the start and its modulus off the mask; exactly 0 under `spec_mask`), to
    `known_spec` (through the known bins' signal at every iteration, through the start and, for a magnitude `spec`, through
    `|known_spec|` inside `phase_init`; exactly 0 outside `spec_mask`), to `known_wave` (exactly 0 outside `wave_mask`) and to each
    parameter tensor, in its dtype, shape and device.  The masks are constants.  First derivatives only; at most 65535 items.
    """
    if not isinstance(spec, torch.Tensor):
        raise TypeError("spec must be a torch.Tensor")
    if spec.dim() not in (2, 3):
        raise ValueError(f"spec must be (F, T) or (B, F, T), got shape {tuple(spec.shape)}")
    has_spec = _together("known_spec", known_spec, "spec_mask", spec_mask)
    has_wave = _together("known_wave", known_wave, "wave_mask", wave_mask)
    if has_spec and not known_spec.is_complex():
        raise TypeError(f"known_spec must be complex, got dtype {known_spec.dtype}")
    if has_wave and (known_wave.is_complex() or known_wave.dtype == torch.bool):
        raise TypeError(f"known_wave must be real, got dtype {known_wave.dtype}")
    if has_spec:
        spec_mask = _expanded("known_spec", known_spec, "spec_mask", spec_mask, spec.shape)
    if not has_spec and not has_wave:
        return agla_unfolded(spec, n_iter=n_iter, alpha=alpha, beta=beta, gamma=gamma, **stft_kwargs)
    al, be, ga, sched = _schedules(n_iter, alpha, beta, gamma)
    spec3, args, rdtype, half = _prepare(spec, stft_kwargs)
    batch, _, n_frames = spec3.shape
    length = args.signal_length(n_frames)
    if has_wave:
        wave_mask = _expanded("known_wave", known_wave, "wave_mask", wave_mask, (length,) if spec.dim() == 2 else (batch, length))
    if batch > _MAX_PLAN_BATCH:
        raise ValueError(f"spec of shape {tuple(spec.shape)} holds {batch} items, constrained_unfolded takes at most {_MAX_PLAN_BATCH}")
    K, xk = (known_spec if has_spec else None), (known_wave if has_wave else None)
    grad = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (spec, K, xk, al, be, ga))
    if not grad and all(len(set(v)) == 1 for v in sched):
        return constrained_griffin_lim(spec, known_spec, spec_mask, known_wave, wave_mask, max_iter=n_iter, tol=0, alpha=sched[0][0],
                                       beta=sched[1][0], gamma=sched[2][0], verbose=False, **stft_kwargs)
    device = require_gpu(spec3.device)
    plan = get_plan(args, batch, n_frames, rdtype, device)
    if grad:
        shape = (batch, length)
        x = _CglaUnfoldedFn.apply(spec3.to(device),
                                  None if K is None else K.to(device=device, dtype=plan.cdtype).reshape(spec3.shape),
                                  None if xk is None else xk.to(device=device, dtype=plan.dtype).reshape(shape), al, be, ga,
                                  None if K is None else spec_mask.to(device).reshape(spec3.shape),
                                  None if xk is None else wave_mask.to(device).reshape(shape), plan, n_iter)
    else:
        _begin(plan, spec3, K, spec_mask, xk, wave_mask, *sched)
        plan.agla_iterate(n_iter)
        x = plan.wave()
        plan.agla_constrain(None)                                  # (the cached plan gives the constraint's memory back)
    trim_plan_cache()
    return _finish(x, spec, half)
