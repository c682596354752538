"""Drop-in host layer: the public functions of the reference's
`torch_specinv/methods.py` (exported at torch_specinv/__init__.py:6) with the same
names, argument meaning, defaults and error behaviour, running on libspecinv's
HIP kernels.

Differences that are deliberate:
  * compute always happens on the HIP device.  Tensors that live on the CPU are
    staged to the current HIP device and the result is returned on the input's
    device; without a GPU the functions raise (there is no CPU fallback).
  * `griffin_lim`, `ADMM` and `RTISI_LA` are differentiable w.r.t. `spec` (recorded forward + hand-written
    adjoint kernels, see autograd.py).
"""
from __future__ import annotations

import inspect
import os
import sys

import torch
from tqdm import tqdm

from . import _lib
from .lbfgs import LBFGS as _LBFGS
from .plan import args_helper, get_plan, require_gpu, trim_plan_cache
from .transforms import DeviceTransform

__all__ = ["griffin_lim", "RTISI_LA", "ADMM", "L_BFGS", "phase_init"]


def _format_spec(spec):
    """methods.py:99-111 shape rules (2-D -> (1, F, T); rank must be 2 or 3)."""
    assert 4 > spec.dim() > 1
    return spec.unsqueeze(0) if spec.dim() == 2 else spec


_HALF = {torch.float16: torch.float32, torch.complex32: torch.complex64}


def _widen(spec, stft_kwargs):
    """float16 / complex32 spectrograms (methods.py:52-53 names them) are inverted in float32 and the result is rounded back to
    float16: the kernels are float32 / float64.  (The reference would compute in half precision itself - where torch.stft can -
    so its result is the noisier of the two.)  Returns (spec, stft_kwargs, dtype to cast the result to or None)."""
    if spec.dtype not in _HALF:
        return spec, stft_kwargs, None
    kw = dict(stft_kwargs)
    w = kw.get("window")
    if isinstance(w, torch.Tensor) and w.dtype == torch.float16:
        kw["window"] = w.float()
    return spec.to(_HALF[spec.dtype]), kw, torch.float16


def _finish(x, spec, out_device):
    """methods.py:267-270: squeeze unless the input was exactly (1, F, T)."""
    trim_plan_cache()
    if not (spec.shape[0] == 1 and spec.dim() == 3):
        x = x.squeeze(0)
    return x.to(out_device)


def _no_complex_window(args):
    """The reference gets as far as its first overlap-add with a complex window and fails there: conv_transpose1d of
    the real frames with the complex `diag(window)` weight (methods.py:95,127), `asym_window1 += window` in RTISI_LA
    (:327).  Same exception type here, before any work is queued.  (`phase_init` never reads the window: it accepts one.)"""
    if args.complex_window:
        raise RuntimeError("complex windows are not supported: the reference's overlap-add (F.conv_transpose1d of real "
                           "frames with a complex diag(window) weight, torch_specinv/methods.py:127) raises on them too")


def _run_loop(plan, max_iter, tol, verbose, eva_iter, metric):
    """Drives the library's `_training_loop` (methods.py:153-190) and mirrors its tqdm bar."""
    assert eva_iter > 0
    assert max_iter > 0
    assert tol >= 0
    assert isinstance(metric, str) and metric.upper() in _lib.METRICS
    name = metric.upper()
    with tqdm(total=max_iter, disable=not verbose) as pbar:
        def on_eval(_it, m, loss):
            pbar.set_postfix(**{name: m}, loss=loss)
            pbar.update(eva_iter)
            return 0
        return plan.run(max_iter, eva_iter, tol, metric, callback=on_eval if verbose else None)


# A plan takes at most this many batch items (the batch is a y / z extent of its launch grids: specinv_plan_create refuses more).
# The reference has no such bound (every op is batched by torch): the drop-in functions split larger batches into slices.
_MAX_PLAN_BATCH = 65535


def _slices(n_items, per=None):
    per = per or _MAX_PLAN_BATCH
    return [(lo, min(n_items, lo + per)) for lo in range(0, n_items, per)]


def _iterative_sliced(which, spec3, args, device, rdtype, coef, max_iter, tol, verbose, eva_iter, metric, per=None):
    """griffin_lim / ADMM / accelerated_griffin_lim (`which` = "gla", "admm", "agla"; `coef` the parameters of `Plan.<which>_init`
    after the two spectrogram arguments, a tuple where there are several) on a batch beyond one plan's 65 535 items (`per`): one
    plan per slice, stepped in lockstep; the metric and the stop rule of `_training_loop` (torch_specinv/methods.py:181-190) are
    whole-batch quantities, so every evaluation adds the slices' sums before the decision - what `distributed.run_loop_global`
    does across ranks, here across slices."""
    from .metrics import _from_sums
    from .plan import Plan
    assert eva_iter > 0 and max_iter > 0 and tol >= 0
    assert isinstance(metric, str) and metric.upper() in _lib.METRICS
    name = metric.upper()
    coefs = coef if isinstance(coef, tuple) else (coef,)
    plans = []
    for lo, hi in _slices(spec3.shape[0], per):
        p = Plan(args, hi - lo, spec3.shape[2], rdtype, device)
        part = spec3[lo:hi]
        init = getattr(p, which + "_init")
        if part.is_complex():
            init(part, None, *coefs)
        else:
            init(None, part, *coefs)
        plans.append(p)
    done, init_loss, previous = 0, None, None
    with tqdm(total=max_iter, disable=not verbose) as pbar:
        while done < max_iter:
            until = eva_iter - (done % eva_iter)
            if done + until > max_iter:
                for p in plans:
                    p.iterate(max_iter - done)
                break
            sums = [p.iterate(until, eval_last=True) for p in plans]
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


def _iterative(which, spec, coef, max_iter, tol, verbose, eva_iter, metric, stft_kwargs):
    spec3 = _format_spec(spec)
    real_in = not spec3.is_complex()
    args = args_helper(spec3, **stft_kwargs)
    _no_complex_window(args)
    device = require_gpu(spec3.device)
    rdtype = spec3.real.dtype if spec3.is_complex() else spec3.dtype
    if spec3.shape[0] > _MAX_PLAN_BATCH and not (torch.is_grad_enabled() and spec.requires_grad):
        x = _iterative_sliced(which, spec3.to(device), args, device, rdtype, coef, max_iter, tol, verbose, eva_iter, metric)
        return _finish(x, spec, spec.device)
    plan = get_plan(args, spec3.shape[0], spec3.shape[2], rdtype, device)
    if torch.is_grad_enabled() and spec.requires_grad:
        # a gradient w.r.t. the spectrogram is wanted: recorded forward + hand-written adjoints (autograd.py)
        from .autograd import admm_differentiable, griffin_lim_differentiable
        run = griffin_lim_differentiable if which == "gla" else admm_differentiable
        assert eva_iter > 0 and max_iter > 0 and tol >= 0
        name = metric.upper()
        with tqdm(total=max_iter, disable=not verbose) as pbar:
            def on_eval(_it, m, loss):
                pbar.set_postfix(**{name: m}, loss=loss)
                pbar.update(eva_iter)
            x = run(spec3.to(device), plan, coef, max_iter, tol, eva_iter, metric, on_eval if verbose else None)
        return _finish(x, spec, spec.device)
    init = getattr(plan, which + "_init")
    if real_in:
        init(None, spec3, coef)        # phase_init on the device (methods.py:106)
    else:
        init(spec3, None, coef)        # target = |spec| (methods.py:110)
    _run_loop(plan, max_iter, tol, verbose, eva_iter, metric)
    return _finish(plan.wave(), spec, spec.device)


def griffin_lim(spec, max_iter=200, tol=1e-6, alpha=0.99, verbose=True, eva_iter=10, metric="sc", **stft_kwargs):
    r"""Griffin-Lim / Fast Griffin-Lim phase reconstruction (reference: methods.py:193-270).

    Args and return value are those of `torch_specinv.methods.griffin_lim`: `spec` is a
    magnitude (F, T) / (B, F, T) tensor, or a complex one to warm-start from; `alpha` is the
    Fast-Griffin-Lim momentum (default 0.99, methods.py:196); `**stft_kwargs` are the
    `torch.stft` arguments the spectrogram was computed with.  Returns (L,) / (B, L).
    """
    assert alpha >= 0
    spec, stft_kwargs, half = _widen(spec, stft_kwargs)
    y = _iterative("gla", spec, alpha, max_iter, tol, verbose, eva_iter, metric, stft_kwargs)
    return y.to(half) if half else y


def ADMM(spec, max_iter=1000, tol=1e-6, rho=0.1, verbose=1, eva_iter=10, metric="sc", **stft_kwargs):
    r"""Griffin-Lim-like phase recovery via ADMM (reference: methods.py:415-506)."""
    assert eva_iter > 0
    assert max_iter > 0
    assert tol >= 0
    assert isinstance(metric, str) and metric.upper() in _lib.METRICS
    spec, stft_kwargs, half = _widen(spec, stft_kwargs)
    y = _iterative("admm", spec, rho, max_iter, tol, verbose, eva_iter, metric, stft_kwargs)
    return y.to(half) if half else y


_STFT_KWARGS = tuple(p for p in inspect.signature(torch.stft).parameters if p not in ("input", "n_fft"))


def RTISI_LA(spec, look_ahead=-1, asymmetric_window=False, max_iter=25, alpha=0.99, verbose=1, **stft_kwargs):
    r"""Real-Time Iterative Spectrogram Inversion with Look-Ahead (reference: methods.py:273-412).

    The whole frame-serial recursion runs inside one kernel launch per batch (one workgroup per batch item).  With
    `verbose` the frames are fed in blocks through the resumable form of the same kernel (`specinv_rtisi_stream_push`,
    the same samples bit for bit) and the bar advances per block; the reference's bar counts the same
    `frames + look_ahead` steps (:362,400).
    """
    assert max_iter > 0
    assert alpha >= 0
    assert not spec.is_complex()
    spec, stft_kwargs, half = _widen(spec, stft_kwargs)
    spec3 = _format_spec(spec)
    args = args_helper(spec3, **stft_kwargs)
    if not asymmetric_window:
        # this branch of the reference hands the caller's kwargs to torch.stft as they are (:308-310,385): a name
        # torch.stft does not know is a TypeError there, not a silently dropped one
        for key in stft_kwargs:
            if key not in _STFT_KWARGS:
                raise TypeError(f"stft() got an unexpected keyword argument '{key}'")
    _no_complex_window(args)
    device = require_gpu(spec3.device)
    if torch.is_grad_enabled() and spec.requires_grad:
        from .autograd import rtisi_differentiable
        plan = get_plan(args, spec3.shape[0], spec3.shape[2], spec3.dtype, device)
        x = rtisi_differentiable(spec3.to(device), plan, look_ahead, asymmetric_window, max_iter, alpha)
    elif verbose and spec3.shape[2] >= 32 and _live_progress():
        x = _rtisi_with_progress(spec3.to(device), look_ahead, asymmetric_window, max_iter, alpha, stft_kwargs)
    elif spec3.shape[0] > _MAX_PLAN_BATCH:
        # (items are independent, methods.py:363-404: slices of the batch, one plan each)
        from .plan import Plan
        x = torch.cat([Plan(args, hi - lo, spec3.shape[2], spec3.dtype, device).rtisi(spec3[lo:hi], look_ahead, asymmetric_window,
                                                                                       max_iter, alpha)
                       for lo, hi in _slices(spec3.shape[0])], 0)
    else:
        # one persistent launch (what the benchmark measures); a bar nobody watches live is completed at the end
        plan = get_plan(args, spec3.shape[0], spec3.shape[2], spec3.dtype, device)
        keep = ((stft_kwargs.get("win_length") or args.n_fft) - 1) // args.hop_length      # num_keep, methods.py:322-324
        with tqdm(total=spec3.shape[2] + (keep if look_ahead < 0 else look_ahead), disable=not verbose) as pbar:   # methods.py:362
            x = plan.rtisi(spec3, look_ahead, asymmetric_window, max_iter, alpha)
            if verbose:
                torch.cuda.synchronize(device)
            pbar.update(pbar.total)
    x = _finish(x, spec, spec.device)
    return x.to(half) if half else x


def _live_progress():
    """A bar that advances while the recursion runs costs a launch (and a host round trip) per block of frames instead of
    the one persistent launch: only worth it when somebody is watching it move - stderr is a terminal - or on request
    (SPECINV_RTISI_PROGRESS=blocks; =end forces the single launch)."""
    mode = os.environ.get("SPECINV_RTISI_PROGRESS", "")
    if mode in ("blocks", "end"):
        return mode == "blocks"
    try:
        return sys.stderr.isatty()
    except (AttributeError, ValueError):
        return False


def _rtisi_with_progress(spec3, look_ahead, asymmetric_window, max_iter, alpha, stft_kwargs):
    from .streaming import RTISIStream
    frames = spec3.shape[2]
    block = min(256, max(16, frames // 8))            # about eight updates of the bar, eight launches
    stream = RTISIStream(spec3.shape[1], spec3.shape[0], look_ahead, asymmetric_window, max_iter, alpha, max_push=block,
                         dtype=spec3.dtype, device=spec3.device, **stft_kwargs)
    pieces = []
    with tqdm(total=frames + stream.look_ahead) as pbar:                  # methods.py:362
        for j in range(0, frames, block):
            pieces.append(stream.push(spec3[:, :, j:j + block]))
            pbar.update(min(block, frames - j))
        pieces.append(stream.flush())
        pbar.update(stream.look_ahead)
    return torch.cat(pieces, 1)


def phase_init(spec, **stft_kwargs):
    r"""Single-pass phase initialisation (reference: methods.py:572-615).  Returns a complex
    tensor of the input's shape."""
    assert not spec.is_complex()
    spec, stft_kwargs, half = _widen(spec, stft_kwargs)
    shape = spec.shape
    spec3 = spec.unsqueeze(0) if spec.dim() == 2 else spec
    assert spec3.dim() == 3
    args = args_helper(spec3, **stft_kwargs)
    device = require_gpu(spec3.device)
    if spec3.shape[0] > _MAX_PLAN_BATCH:
        from .plan import Plan
        out = torch.cat([Plan(args, hi - lo, spec3.shape[2], spec3.dtype, device).phase_init(spec3[lo:hi])
                         for lo, hi in _slices(spec3.shape[0])], 0).view(shape).to(spec.device)
        return out.to(torch.complex32) if half else out
    plan = get_plan(args, spec3.shape[0], spec3.shape[2], spec3.dtype, device)
    out = plan.phase_init(spec3).view(shape).to(spec.device)
    return out.to(torch.complex32) if half else out


def L_BFGS(spec, transform_fn, samples=None, init_x0=None, outer_max_iter=1000, tol=1e-6, verbose=1, eva_iter=10,
           metric="sc", **kwargs):
    r"""Waveform optimisation with L-BFGS (reference: methods.py:509-569).

    `transform_fn` is either a `spectrogram_inversion_amd.transforms.DeviceTransform`
    (`MagSTFT`, `LogMelSTFT`: fused HIP forward + analytic backward) or any differentiable
    callable like in the reference (then torch autograd evaluates it and only the optimiser's
    vector arithmetic runs on libspecinv's kernels).  `**kwargs` go to the optimiser with
    `torch.optim.LBFGS`'s names and defaults.
    """
    assert eva_iter > 0
    assert outer_max_iter > 0
    assert tol >= 0
    assert isinstance(metric, str) and metric.upper() in _lib.METRICS
    device = require_gpu(spec.device)
    if init_x0 is None:
        init_x0 = spec.new_empty(*samples).normal_(std=1e-6)             # methods.py:538
    # the reference optimises `nn.Parameter(init_x0)` (methods.py:539), i.e. the caller's tensor in place, and returns
    # a view of it (:569): same here - straight on its storage when it already lives on the device, through a
    # staging copy otherwise
    x0 = init_x0.detach()
    in_place = x0.device == device and x0.is_contiguous() and x0.dtype in (torch.float32, torch.float64)
    x = x0 if in_place else x0.to(device=device).clone().contiguous()
    target = spec.detach().to(device)

    if isinstance(transform_fn, DeviceTransform):
        fwd, fg = transform_fn.bind(x, target)
    else:
        def fwd(v):
            with torch.no_grad():
                return transform_fn(v)

        def fg(v):
            p = v.detach().clone().requires_grad_(True)
            with torch.enable_grad():
                loss = torch.nn.functional.mse_loss(transform_fn(p), target)   # methods.py:547-549
            (g,) = torch.autograd.grad(loss, p)
            return float(loss.detach()), g.contiguous()

    opt = _LBFGS(x, device=device, **kwargs)
    name = metric.upper()
    from .metrics import _sums, _from_sums
    init_loss = None
    previous_loss = None
    with tqdm(total=outer_max_iter, disable=not verbose) as pbar:
        for i in range(outer_max_iter):                                   # _training_loop, :178
            opt.step(fg)                                                  # :553
            if i % eva_iter == eva_iter - 1:
                v = fwd(x)                                                # :554-556
                s = _sums(v, target.reshape(v.shape))
                m, l2 = _from_sums(name, s), s[0] / s[3]
                pbar.set_postfix(**{name: m}, loss=l2)
                pbar.update(eva_iter)
                if not init_loss:
                    init_loss = l2
                elif (previous_loss - l2) / init_loss < tol and previous_loss > l2:
                    break
                previous_loss = l2
    if not in_place:
        x0.copy_(x)
    del opt                      # (a device-resident optimiser hands its vectors back to the plan's bounded pool)
    trim_plan_cache()
    return x0
