"""Multiple Input Spectrogram Inversion (MISI; Gunawan & Sen 2010, the layer Wang, Le Roux & Hershey 2018 unfold): phase
retrieval for the K magnitude estimates of a source separator, done jointly so that the K waveforms add up to the mixture.

One iteration is the Griffin-Lim projection without momentum on the B * K items, followed by the coupling step

    e = (mix - sum_k y_k) / K ;   x_k = y_k + e

on the plan's own signal state (`specinv_misi_*`, csrc/kernels_misi.h).  `misi_unfolded` is a fixed number of these iterations as a
differentiable layer (csrc/kernels_misi_adjoint.h).  Not part of the reference's surface.
"""
from __future__ import annotations

import torch

from . import _lib
from ._ingest import ingest
from .methods import _MAX_PLAN_BATCH, _no_complex_window, _run_loop
from .plan import Plan, args_helper, get_plan, require_gpu, trim_plan_cache

__all__ = ["misi", "misi_unfolded"]

_NARROW = {torch.float16: torch.float32, torch.bfloat16: torch.float32, torch.complex32: torch.complex64}
_REAL_OF = {torch.complex64: torch.float32, torch.complex128: torch.float64}


def _start(plan: Plan, specs3, mix2, n_src):
    """The starting spectrogram of one plan's items: a complex input as it is; magnitudes with the mixture's phase,
    C = polar(mag, angle(STFT(mix))) - the mixture's spectrogram from the plan itself, on the mixture repeated n_src times; where
    it is exactly 0 the angle is 0."""
    if specs3.is_complex():
        return specs3, None
    phase = torch.angle(plan.stft(mix2[:, :plan.length].repeat_interleave(n_src, dim=0).contiguous()))
    return torch.polar(specs3, phase), specs3


def _run_sliced(specs4, mix2, args, device, rdtype, per, max_iter, tol, verbose, eva_iter, metric):
    """More than one plan's worth of items: slices of whole mixtures, one plan each, stepped in lockstep; the stop rule of
    `_training_loop` sees the sums of all slices (what methods._iterative_sliced does for griffin_lim)."""
    from tqdm import tqdm

    from .metrics import _from_sums
    assert eva_iter > 0 and max_iter > 0 and tol >= 0
    assert isinstance(metric, str) and metric.upper() in _lib.METRICS
    name = metric.upper()
    B, K, F, T = specs4.shape
    plans = []
    for lo in range(0, B, per):
        hi = min(B, lo + per)
        p = Plan(args, (hi - lo) * K, T, rdtype, device)
        part = specs4[lo:hi].reshape((hi - lo) * K, F, T)
        init, mag = _start(p, part, mix2[lo:hi], K)
        p.misi_init(init, mag, mix2[lo:hi], K)
        plans.append(p)
    done, init_loss, previous = 0, None, None
    with tqdm(total=max_iter, disable=not verbose) as pbar:
        while done < max_iter:
            until = eva_iter - (done % eva_iter)
            if done + until > max_iter:
                for p in plans:
                    p.misi_iterate(max_iter - done)
                break
            sums = [p.misi_iterate(until, eval_last=True) for p in plans]
            s = [sum(v[k] for v in sums) for k in range(4)]
            done += until
            m, loss = _from_sums(name, s), s[0] / s[3]
            pbar.set_postfix(**{name: m}, loss=loss)
            pbar.update(eva_iter)
            if not init_loss:
                init_loss = loss
            elif (previous - loss) / init_loss < tol and previous > loss:
                break
            previous = loss
    return torch.cat([p.wave() for p in plans], 0)


def _check_tensors(specs, mixture):
    if not isinstance(specs, torch.Tensor) or not isinstance(mixture, torch.Tensor):
        raise TypeError("specs and mixture must be torch.Tensors")
    if mixture.is_complex():
        raise TypeError(f"mixture must be a real waveform, got dtype {mixture.dtype}")
    if specs.dim() not in (3, 4):
        raise ValueError(f"specs must be (K, F, T) or (B, K, F, T), got shape {tuple(specs.shape)}")
    if mixture.dim() != specs.dim() - 2:
        raise ValueError(f"mixture must be {'(L,)' if specs.dim() == 3 else '(B, L)'} for specs of shape {tuple(specs.shape)}, "
                         f"got shape {tuple(mixture.shape)}")


def _prepare(specs, mixture, stft_kwargs):
    """The checked arguments in the form the plan takes, all that needs no device: (specs4 (B, K, F, T), mix2 (B, L_m), args,
    rdtype, L, half) - float16 / bfloat16 widened to float32 (`half`: the dtype to return), a batch axis added where absent."""
    half = specs.dtype if specs.dtype in _NARROW else None
    if half is not None:
        specs = specs.to(_NARROW[specs.dtype])
        w = stft_kwargs.get("window")
        if isinstance(w, torch.Tensor) and w.dtype in _NARROW:
            stft_kwargs = dict(stft_kwargs, window=w.float())
    if mixture.dtype in _NARROW:
        mixture = mixture.to(_NARROW[mixture.dtype])
    rdtype = _REAL_OF.get(specs.dtype, specs.dtype)
    if rdtype not in (torch.float32, torch.float64):
        raise TypeError(f"specs of dtype {specs.dtype} are not supported (float16 / bfloat16 / float32 / float64 or complex)")
    if mixture.dtype != rdtype:
        raise TypeError(f"mixture is {mixture.dtype}, specs compute in {rdtype}")
    specs4 = specs.unsqueeze(0) if specs.dim() == 3 else specs
    mix2 = mixture.unsqueeze(0) if mixture.dim() == 1 else mixture
    B, K, F, T = specs4.shape
    if B < 1 or K < 1 or T < 1:
        raise ValueError(f"specs of shape {tuple(specs.shape)} hold no items")
    if mix2.shape[0] != B:
        raise ValueError(f"mixture of shape {tuple(mixture.shape)} has {mix2.shape[0]} rows, specs of shape {tuple(specs.shape)} "
                         f"hold {B} mixtures")
    if K > _MAX_PLAN_BATCH:
        raise ValueError(f"specs of shape {tuple(specs.shape)}: {K} sources per mixture, a plan takes at most {_MAX_PLAN_BATCH} items")
    args = args_helper(specs4.reshape(B * K, F, T), **stft_kwargs)
    _no_complex_window(args)
    L = args.signal_length(T)
    if mix2.shape[1] < L:
        raise ValueError(f"mixture of shape {tuple(mixture.shape)} is shorter than the {L} samples specs of shape "
                         f"{tuple(specs.shape)} invert to")
    return specs4, mix2, args, rdtype, L, half


def _finish(x, specs, half):
    """(B * K, L) on the device -> the caller's shape, device and dtype."""
    B, K = (1, specs.shape[0]) if specs.dim() == 3 else specs.shape[:2]
    x = x.reshape(B, K, -1)
    if specs.dim() == 3:
        x = x.squeeze(0)
    x = x.to(specs.device)
    if half is None:
        return x
    return x.to(torch.float16 if half == torch.complex32 else half)


def misi(specs, mixture, max_iter=200, tol=1e-6, verbose=True, eva_iter=10, metric="sc", **stft_kwargs):
    r"""Waveforms (K, L) / (B, K, L) of K sources whose sum is the mixture, from their spectrograms.

    `specs` is (K, F, T) or (B, K, F, T): magnitudes - the iteration then starts from the mixture's phase - or a complex
    spectrogram to start from (its modulus is the target).  `mixture` is (L_m,) or (B, L_m) with L_m >= L, the length the
    spectrograms invert to; samples beyond L are ignored.  `max_iter`, `tol`, `eva_iter`, `metric`, `verbose` and
    `**stft_kwargs` are those of `griffin_lim`; there is no momentum.  The sum of the result over its source axis equals
    `mixture[..., :L]` to rounding.  CPU tensors are computed on the current HIP device and come back to the CPU; float16 /
    bfloat16 are computed in float32.  Not differentiable: `misi_unfolded` is the form to train through.
    """
    _check_tensors(specs, mixture)
    if torch.is_grad_enabled() and (specs.requires_grad or mixture.requires_grad):
        raise NotImplementedError("misi is not differentiable; detach the inputs")
    specs4, mix2, args, rdtype, L, half = _prepare(specs, mixture, stft_kwargs)
    B, K, F, T = specs4.shape
    device = require_gpu(specs.device)
    specs4, mix2 = specs4.to(device), mix2.to(device)
    if B * K > _MAX_PLAN_BATCH:
        x = _run_sliced(specs4, mix2, args, device, rdtype, _MAX_PLAN_BATCH // K, max_iter, tol, verbose, eva_iter, metric)
    else:
        plan = get_plan(args, B * K, T, rdtype, device)
        init, mag = _start(plan, specs4.reshape(B * K, F, T), mix2, K)
        plan.misi_init(init, mag, mix2, K)
        _run_loop(plan, max_iter, tol, verbose, eva_iter, metric)
        x = plan.wave()
    trim_plan_cache()
    return _finish(x, specs, half)


class _MisiUnfoldedFn(torch.autograd.Function):
    """`n_iter` MISI iterations as one differentiable layer.  The forward pass is the inference kernels with the iterates recorded
    as signals, x_0 ... x_{N-1} (N B K L reals where recorded spectra would be N B K F T complex); the backward sweep recomputes
    each spectrum from its signal and runs one `specinv_misi_step_adjoint` per iteration (csrc/kernels_misi_adjoint.h)."""

    @staticmethod
    def forward(ctx, specs4, mix2, plan, n_iter):
        B, K, F, T = specs4.shape
        specs3 = ingest(specs4.reshape(B * K, F, T), plan.device, plan.cdtype if specs4.is_complex() else plan.dtype)
        mix = ingest(mix2, plan.device, plan.dtype)
        init, mag = _start(plan, specs3, mix, K)
        plan.misi_init(init, mag, mix, K)
        waves = []
        for _ in range(n_iter):
            waves.append(plan.wave())                                  # x_{n-1}: what the next projection launch reads
            plan.misi_iterate(1)
        ctx.plan, ctx.n_src = plan, K
        ctx.save_for_backward(specs3, mix, *waves)
        return plan.wave()

    @staticmethod
    def backward(ctx, g_y):
        plan, K = ctx.plan, ctx.n_src
        specs3, mix, *waves = ctx.saved_tensors
        n_mix, L = plan.batch // K, plan.length
        real_in = not specs3.is_complex()
        mag = specs3 if real_in else specs3.abs()
        g = g_y.detach().to(plan.dtype).clone(memory_format=torch.contiguous_format)   # (the sweep works in place)
        gmix = torch.zeros((n_mix, L), dtype=plan.dtype, device=plan.device)
        mag_fm = mag.transpose(1, 2).contiguous()                      # frame-major once, not once per iteration
        gm_fm = torch.zeros_like(mag_fm)
        for x_prev in reversed(waves):
            plan.misi_step_adjoint(K, x_prev, mag_fm, g, gmix, gm_fm)
        plan.misi_mix_adjoint(K, g, gmix)                              # x_0 = M(ISTFT(C0))
        gc = plan.istft_adjoint(g)
        gm = gm_fm.transpose(1, 2)
        if real_in:
            # C0 = specs U, U = R / |R| the phase of R = STFT(mixture[:L]) (1, with no gradient, where R = 0)
            r = plan.stft(mix[:, :L].repeat_interleave(K, dim=0).contiguous())
            a = r.abs()
            zero = a == 0
            u = torch.where(zero, torch.ones_like(r), r / a)
            g_specs = gm + (gc.real * u.real + gc.imag * u.imag)
            if ctx.needs_input_grad[1]:
                gu = gc * mag
                g_r = torch.where(zero, torch.zeros_like(r), (gu - u * (gu.real * u.real + gu.imag * u.imag)) / a)
                gmix += plan.stft_adjoint(g_r, L).reshape(n_mix, K, L).sum(1)
        else:
            unit = torch.where(mag > 0, specs3 / mag, torch.zeros_like(specs3))
            g_specs = gc + gm * unit                                   # target = |C0| (autograd._input_grad)
        g_mix = None
        if ctx.needs_input_grad[1]:
            g_mix = torch.zeros_like(mix)                              # samples beyond L never enter
            g_mix[:, :L] = gmix
        return g_specs.reshape(n_mix, K, *specs3.shape[1:]), g_mix, None, None


def misi_unfolded(specs, mixture, n_iter=5, **stft_kwargs):
    r"""`n_iter` MISI iterations as a layer to train through (Wang, Le Roux & Hershey 2018): `misi` with a fixed iteration count
    and gradients.

    `specs`, `mixture`, `**stft_kwargs`, the start, shapes, dtypes and devices are those of `misi`; there is no stop rule.  Without
    a gradient to compute the result is `misi(specs, mixture, max_iter=n_iter, tol=0, verbose=False, **stft_kwargs)`.  With grad
    mode on and `specs` or `mixture` requiring grad, the same kernels run and the result carries gradients to `specs` (magnitudes:
    directly and through the start; a complex start: through the start and its modulus, the target) and to `mixture` (through
    every coupling step and, for magnitudes, through the start's phase; samples beyond L get zero).  At most 65535 items (B * K).
    """
    _check_tensors(specs, mixture)
    if isinstance(n_iter, bool) or not isinstance(n_iter, int) or n_iter < 1:
        raise ValueError(f"n_iter must be an integer >= 1, got {n_iter!r}")
    specs4, mix2, args, rdtype, L, half = _prepare(specs, mixture, stft_kwargs)
    B, K, F, T = specs4.shape
    if B * K > _MAX_PLAN_BATCH:
        raise ValueError(f"specs of shape {tuple(specs.shape)} hold {B * K} items, misi_unfolded takes at most {_MAX_PLAN_BATCH}")
    if not (torch.is_grad_enabled() and (specs.requires_grad or mixture.requires_grad)):
        return misi(specs, mixture, max_iter=n_iter, tol=0, verbose=False, **stft_kwargs)
    device = require_gpu(specs.device)
    plan = get_plan(args, B * K, T, rdtype, device)
    x = _MisiUnfoldedFn.apply(specs4.to(device), mix2.to(device), plan, n_iter)
    trim_plan_cache()
    return _finish(x, specs, half)
