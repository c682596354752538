"""One Griffin-Lim projection as a differentiable layer, and the two transforms it sits between.

    P(x; m) = ISTFT(m S / (|S| + 1e-16)) ,  S = STFT(x)

is one iteration of `griffin_lim` without momentum (torch_specinv/methods.py:241-248) written on signals: what `misi_unfolded`
and `agla_unfolded` fix a coupling or an extrapolation around, and what every unfolded phase-retrieval model puts something
learned behind.  `gla_projection` is that piece alone; `stft` / `istft` are the library's transforms (envelope division, signal
length, padding and scaling as everywhere else) to get into and out of the signal domain:

    x = si.istft(si.phase_init(mag), hop_length=hop, window=w)
    for n in range(N):
        x = net[n](si.gla_projection(x, mag, hop_length=hop, window=w))

The backward pass of `gla_projection` recomputes S from x and is one fused launch where the plan has it
(csrc/kernels_proj_adjoint.h).  Not part of the reference's surface.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import methods as _m
from ._ingest import ingest
from .plan import args_helper, get_plan, require_gpu, trim_plan_cache

__all__ = ["gla_projection", "stft", "istft"]

_MAX_PLAN_BATCH = _m._MAX_PLAN_BATCH
_REAL = (torch.float16, torch.bfloat16, torch.float32, torch.float64)
_COMPLEX = {torch.complex32: torch.float16, torch.complex64: torch.float32, torch.complex128: torch.float64}


def _compute_dtype(dtype):
    """float16 / bfloat16 are computed in float32 (and returned in the input's dtype)"""
    return torch.float32 if dtype in (torch.float16, torch.bfloat16) else dtype


def _args(n_freq, rdtype, stft_kwargs):
    """The plan's arguments for `n_freq` bins: `args_helper` reads the bin count and the dtype off a spectrogram."""
    w = stft_kwargs.get("window")
    onesided = stft_kwargs.get("onesided")
    if onesided is None:
        onesided = not (isinstance(w, torch.Tensor) and w.is_complex())
    n_fft = (n_freq - 1) * 2 if onesided else n_freq
    win_length = stft_kwargs.get("win_length") or (w.numel() if isinstance(w, torch.Tensor) else n_fft)
    if n_fft < 2 or win_length > n_fft:
        raise ValueError(f"{n_freq} bins mean n_fft = {n_fft}, which does not hold a window of {win_length} samples")
    args = args_helper(torch.empty((n_freq, 1), dtype=rdtype, device="meta"), **stft_kwargs)
    _m._no_complex_window(args)
    return args


def _batched(t, what, dims):
    """(..., ) -> with a batch axis; `dims` is the rank without one"""
    if t.dim() not in (dims, dims + 1):
        raise ValueError(f"{what} must have {dims} or {dims + 1} dimensions, got shape {tuple(t.shape)}")
    return t.unsqueeze(0) if t.dim() == dims else t


def _check_items(n, name, what):
    if n > _MAX_PLAN_BATCH:
        raise ValueError(f"{what} holds {n} items, {name} takes at most {_MAX_PLAN_BATCH}")


class _ProjectionFn(torch.autograd.Function):
    """y = P(x; m) on a plan: x (B, L), m frame-major (B, T, F), both on the plan's device in its dtype.  Only x and m are saved;
    the backward pass recomputes S (`specinv_project_adjoint`)."""

    @staticmethod
    def forward(ctx, x, mag_fm, plan):
        x, mag_fm = ingest(x, plan.device, plan.dtype), ingest(mag_fm, plan.device, plan.dtype)
        ctx.plan = plan
        ctx.save_for_backward(x, mag_fm)
        return plan.project(x, mag_fm)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_y):
        x, mag_fm = ctx.saved_tensors
        g_x, g_mag = ctx.plan.project_adjoint(x, mag_fm, g_y)
        return g_x, g_mag, None


class _StftFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, plan):
        ctx.plan, ctx.length = plan, x.shape[1]
        return plan.stft(x.detach())

    @staticmethod
    @once_differentiable
    def backward(ctx, g_spec):
        return ctx.plan.stft_adjoint(g_spec, ctx.length), None


class _IstftFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, spec, plan):
        ctx.plan = plan
        return plan.istft(spec.detach())

    @staticmethod
    @once_differentiable
    def backward(ctx, g_x):
        return ctx.plan.istft_adjoint(g_x), None


def gla_projection(x, mag, frame_major=False, **stft_kwargs):
    r"""One projection of Griffin-Lim, y = ISTFT(mag * S / (|S| + 1e-16)) with S = STFT(x), as a layer to build unfolded models
    from.

    `x` is a real waveform (L,) / (B, L), `mag` a real target (F, T) / (B, F, T) - with `frame_major=True` (T, F) / (B, T, F), the
    layout the kernels use: a loop that calls the layer many times with one target then pays no transposes, and `mag.grad` comes
    back in that layout.  L must be the length `**stft_kwargs` (those of `griffin_lim`) give T frames.  The result has the shape
    of `x`.  Differentiable in `x` and `mag` (first derivatives); where |S| = 0 the derivative of S / |S| is taken as 0.
    float16 / bfloat16 are computed in float32 and returned in the dtype of `x`; CPU tensors are computed on the current HIP
    device and come back to the CPU; gradients arrive in the inputs' shape, dtype and device.  At most 65535 items.
    """
    if not isinstance(x, torch.Tensor) or not isinstance(mag, torch.Tensor):
        raise TypeError("x and mag must be torch.Tensors")
    if mag.is_complex():
        raise TypeError(f"mag must be real, got dtype {mag.dtype} (pass spec.abs())")
    if x.dtype not in _REAL or mag.dtype not in _REAL:
        raise TypeError(f"x and mag must be float16 / bfloat16 / float32 / float64, got {x.dtype} and {mag.dtype}")
    x2, mag3 = _batched(x, "x", 1), _batched(mag, "mag", 2)
    if x2.shape[0] != mag3.shape[0]:
        raise ValueError(f"x holds {x2.shape[0]} items and mag {mag3.shape[0]}")
    n_frames, n_freq = (mag3.shape[1], mag3.shape[2]) if frame_major else (mag3.shape[2], mag3.shape[1])
    if n_frames < 1 or n_freq < 1:
        raise ValueError(f"mag of shape {tuple(mag.shape)} holds no frames")
    rdtype = _compute_dtype(x.dtype)
    args = _args(n_freq, rdtype, stft_kwargs)
    length = args.signal_length(n_frames)
    if x2.shape[1] != length:
        raise ValueError(f"x holds {x2.shape[1]} samples, {n_frames} frames need L = {length}")
    _check_items(x2.shape[0], "gla_projection", f"x of shape {tuple(x.shape)}")
    if x2.shape[0] == 0:
        return x * 0 + mag.sum().to(x.dtype) * 0                   # (nothing to compute: zeros that carry a zero gradient)
    device = require_gpu(x.device)
    plan = get_plan(args, x2.shape[0], n_frames, rdtype, device)
    xd = x2.to(device=device, dtype=rdtype)
    md = mag3.to(device=device, dtype=rdtype)
    y = _ProjectionFn.apply(xd, md if frame_major else md.transpose(1, 2), plan)
    trim_plan_cache()
    return y.reshape(x.shape).to(device=x.device, dtype=x.dtype)


def stft(x, n_fft=None, **stft_kwargs):
    """The library's STFT of a real waveform (L,) / (B, L): complex (F, T) / (B, F, T), `torch.stft` with `return_complex=True`.
    `n_fft` defaults to `win_length` or the window's length; the other `**stft_kwargs` are those of `griffin_lim`.  Differentiable
    (first derivatives); dtype, device and batch rules as `gla_projection`."""
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    if x.dtype not in _REAL:
        raise TypeError(f"x must be float16 / bfloat16 / float32 / float64, got {x.dtype}")
    x2 = _batched(x, "x", 1)
    w = stft_kwargs.get("window")
    if n_fft is None:
        n_fft = stft_kwargs.get("win_length") or (w.numel() if isinstance(w, torch.Tensor) else None)
    if not n_fft:
        raise ValueError("stft needs n_fft, win_length or a window")
    onesided = stft_kwargs.get("onesided")
    if onesided is None:
        onesided = not (isinstance(w, torch.Tensor) and w.is_complex())
    rdtype = _compute_dtype(x.dtype)
    args = _args(int(n_fft) // 2 + 1 if onesided else int(n_fft), rdtype, stft_kwargs)
    n_frames = args.frame_count(x2.shape[1]) if x2.shape[1] + 2 * args.padding >= args.n_fft else 0
    if n_frames < 1:
        raise ValueError(f"x holds {x2.shape[1]} samples, fewer than one frame of n_fft = {args.n_fft}")
    _check_items(x2.shape[0], "stft", f"x of shape {tuple(x.shape)}")
    cdtype = torch.complex128 if rdtype == torch.float64 else torch.complex64
    if x2.shape[0] == 0:
        return (x2 * 0).sum(1).to(cdtype)[:, None, None].expand(0, args.n_freq, n_frames)
    device = require_gpu(x.device)
    plan = get_plan(args, x2.shape[0], n_frames, rdtype, device)
    spec = _StftFn.apply(x2.to(device=device, dtype=rdtype).contiguous(), plan)
    trim_plan_cache()
    if x.dim() == 1:
        spec = spec.squeeze(0)
    spec = spec.to(x.device)
    return spec.to(torch.complex32) if x.dtype == torch.float16 else spec


def istft(spec, **stft_kwargs):
    """The library's inverse STFT of a complex spectrogram (F, T) / (B, F, T): the waveform (L,) / (B, L) a `griffin_lim` with
    these `**stft_kwargs` starts from - overlap-add of the windowed inverse frames divided by the window-square envelope.
    Differentiable (first derivatives); dtype, device and batch rules as `gla_projection`."""
    if not isinstance(spec, torch.Tensor):
        raise TypeError("spec must be a torch.Tensor")
    if spec.dtype not in _COMPLEX:
        raise TypeError(f"spec must be complex, got dtype {spec.dtype}")
    spec3 = _batched(spec, "spec", 2)
    n_freq, n_frames = spec3.shape[1], spec3.shape[2]
    if n_frames < 1 or n_freq < 1:
        raise ValueError(f"spec of shape {tuple(spec.shape)} holds no frames")
    out_dtype = _COMPLEX[spec.dtype]
    rdtype = _compute_dtype(out_dtype)
    args = _args(n_freq, rdtype, stft_kwargs)
    _check_items(spec3.shape[0], "istft", f"spec of shape {tuple(spec.shape)}")
    cdtype = torch.complex128 if rdtype == torch.float64 else torch.complex64
    if spec3.shape[0] == 0:
        return (spec3.real * 0).sum((1, 2))[:, None].expand(0, args.signal_length(n_frames)).to(out_dtype)
    device = require_gpu(spec.device)
    plan = get_plan(args, spec3.shape[0], n_frames, rdtype, device)
    x = _IstftFn.apply(spec3.to(device=device, dtype=cdtype).contiguous(), plan)
    trim_plan_cache()
    if spec.dim() == 2:
        x = x.squeeze(0)
    return x.to(device=spec.device, dtype=out_dtype)
