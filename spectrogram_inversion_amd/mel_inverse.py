"""Mel spectrogram -> linear magnitude -> waveform: the two-stage inversion of librosa's `mel_to_stft` / `mel_to_audio` and
torchaudio's `InverseMelScale` + `GriffinLim`, on libspecinv's kernels.

Stage one fits, per frame, the non-negative magnitude s that the filterbank maps closest to the mel column y,

    minimise 1/2 |M s - y|^2  subject to  s >= 0,

by FISTA (accelerated projected gradient) from s = 0 with step 1 / L, L = lambda_max(M M^T), in one launch for every frame and
iteration (`specinv_mel_nnls`, csrc/kernels_mel_nnls.h); the result is s ** (1 / power).  Stage two is any of the phase
retrieval methods on that magnitude.

`mel_to_stft_unfolded` is stage one as a layer to train through: the same launch forward, and one launch backward that recomputes
the iteration per frame and sweeps it in reverse (`specinv_mel_nnls_adjoint`, csrc/kernels_mel_nnls_adjoint.h).
"""
from __future__ import annotations

import ctypes as C
import hashlib
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from ._ingest import ingest
from .agla import agla_unfolded
from .methods import ADMM, RTISI_LA, _MAX_PLAN_BATCH, _slices, griffin_lim
from .plan import _RECOGNISED, Plan, args_helper, get_plan, require_gpu, trim_plan_cache

__all__ = ["mel_to_stft", "mel_to_audio", "mel_to_stft_unfolded", "mel_to_audio_unfolded", "nnls_lipschitz"]

_METHODS = {"griffin_lim": griffin_lim, "ADMM": ADMM, "RTISI_LA": RTISI_LA}
_NARROW = (torch.float16, torch.bfloat16)
_LIPSCHITZ: "OrderedDict[bytes, float]" = OrderedDict()


def nnls_lipschitz(mel_fb) -> float:
    """L = lambda_max(M M^T) of a (n_mels, F) filterbank, in float64 from the matrix's entries: the step of `mel_to_stft` is 1 / L."""
    m = np.asarray(mel_fb.detach().cpu().numpy() if isinstance(mel_fb, torch.Tensor) else mel_fb, dtype=np.float64)
    return float(np.linalg.eigvalsh(m @ m.T)[-1])


def _bank(mel_fb, dtype):
    """(the filterbank as the kernels see it - in the compute dtype -, its digest, L); L is cached by contents"""
    fb = mel_fb.detach() if isinstance(mel_fb, torch.Tensor) else torch.from_numpy(np.asarray(mel_fb))
    if fb.is_complex():
        raise TypeError("mel_fb must be real")
    if fb.dim() != 2:
        raise ValueError(f"mel_fb must be (n_mels, F), got shape {tuple(fb.shape)}")
    fb = fb.to(device="cpu", dtype=dtype).contiguous()
    host = fb.numpy()
    key = hashlib.sha1(host.tobytes()).digest() + str(host.shape).encode() + str(dtype).encode()
    lip = _LIPSCHITZ.get(key)
    if lip is None:
        if not np.all(np.isfinite(host)):
            raise ValueError("mel_fb holds a non-finite entry")
        lip = nnls_lipschitz(host)
        _LIPSCHITZ[key] = lip
        while len(_LIPSCHITZ) > 32:
            _LIPSCHITZ.popitem(last=False)
    else:
        _LIPSCHITZ.move_to_end(key)
    return fb, key, lip


def _nnls_setup(plan: Plan, fb, key, lip):
    """The plan's band form of this filterbank, rebuilt only when the plan last saw another one."""
    plan._sync_stream()
    if getattr(plan, "_nnls_key", None) != key:
        if lip <= 0.0:
            raise ValueError("mel_fb is all zeros: the NNLS step 1 / lambda_max(M M^T) is undefined")
        dev_fb = fb.to(plan.device)
        plan._nnls_key = None
        _lib.check(plan.lib.specinv_mel_nnls_setup(plan._h, dev_fb.data_ptr(), fb.shape[0], lip))
        plan._nnls_key = key


def _nnls(plan: Plan, fb, key, lip, mel3, n_iter, power):
    """One plan's NNLS."""
    _nnls_setup(plan, fb, key, lip)
    y = plan._in(mel3, plan.dtype, (plan.batch, fb.shape[0], plan.n_frames))
    out = torch.empty((plan.batch, plan.n_freq, plan.n_frames), dtype=plan.dtype, device=plan.device)
    _lib.check(plan.lib.specinv_mel_nnls(plan._h, y.data_ptr(), int(n_iter), float(power), out.data_ptr()))
    return out


def _checked(name, mel, mel_fb, power, n_iter, stft_kwargs):
    """The argument checks of `mel_to_stft` / `mel_to_stft_unfolded`, all that needs no device: (half, dtype, fb, key, lip, mel3,
    args) - `half` the narrow dtype to return (or None), `dtype` the compute dtype, `args` the plan's stft arguments."""
    if not isinstance(mel, torch.Tensor):
        raise TypeError("mel must be a torch.Tensor")
    if mel.is_complex():
        raise TypeError(f"{name} takes a real mel spectrogram, not a complex one")
    if not 4 > mel.dim() > 1:
        raise ValueError(f"mel must be (n_mels, T) or (B, n_mels, T), got shape {tuple(mel.shape)}")
    if n_iter < 0:
        raise ValueError(f"n_iter must be >= 0, got {n_iter}")
    if not (power > 0 and np.isfinite(power)):
        raise ValueError(f"power must be finite and > 0, got {power}")
    half = mel.dtype if mel.dtype in _NARROW else None
    dtype = torch.float32 if half else mel.dtype
    if dtype not in (torch.float32, torch.float64):
        raise NotImplementedError(f"dtype {mel.dtype} is not supported (float16 / bfloat16 / float32 / float64)")
    fb, key, lip = _bank(mel_fb, dtype)
    mel3 = mel.unsqueeze(0) if mel.dim() == 2 else mel
    if mel3.shape[1] != fb.shape[0]:
        raise ValueError(f"mel has {mel3.shape[1]} bands, mel_fb {fb.shape[0]}")
    kw = {k: stft_kwargs[k] for k in _RECOGNISED if k in stft_kwargs}
    kw.pop("return_complex", None)
    # (the plan of the magnitude's shape, (B, F, T): what griffin_lim & co. ask for with these kwargs)
    args = args_helper(torch.empty((1, fb.shape[1], 1), dtype=dtype), **kw)
    if args.n_freq != fb.shape[1]:
        raise ValueError(f"mel_fb has {fb.shape[1]} columns; a plan with these stft kwargs has {args.n_freq} bins")
    return half, dtype, fb, key, lip, mel3, args


def mel_to_stft(mel, mel_fb, power=1.0, n_iter=100, **stft_kwargs):
    r"""Linear magnitude (F, T) / (B, F, T) behind a mel spectrogram (n_mels, T) / (B, n_mels, T) (librosa's `mel_to_stft`).

    `mel_fb` is the (n_mels, F) filterbank the mel was built with (a tensor or an ndarray; F = n_fft // 2 + 1), `power` the
    exponent of that mel (mel = mel_fb @ |S| ** power: 1.0 magnitude, the default as for `LogMelSTFT`; 2.0 librosa's power mel).
    Per frame the non-negative least-squares fit of |S| ** power by `n_iter` FISTA iterations from zero, then the root.
    `**stft_kwargs` (those of `griffin_lim`) only pick the plan, so that a following phase retrieval with the same arguments
    reuses it.  CPU tensors are computed on the current HIP device and come back to the CPU; float16 / bfloat16 are computed in
    float32.  Not differentiable.
    """
    if isinstance(mel, torch.Tensor) and not mel.is_complex() and torch.is_grad_enabled() and mel.requires_grad:
        raise NotImplementedError("mel_to_stft is not differentiable; detach the input")
    half, dtype, fb, key, lip, mel3, args = _checked("mel_to_stft", mel, mel_fb, power, n_iter, stft_kwargs)
    F, B, T = fb.shape[1], mel3.shape[0], mel3.shape[2]
    device = require_gpu(mel.device)
    if B == 0 or T == 0:
        out = torch.zeros((B, F, T), dtype=dtype, device=device)
    elif B > _MAX_PLAN_BATCH:
        out = torch.cat([_nnls(Plan(args, hi - lo, T, dtype, device), fb, key, lip, mel3[lo:hi].to(device), n_iter, power)
                         for lo, hi in _slices(B)], 0)
    else:
        out = _nnls(get_plan(args, B, T, dtype, device), fb, key, lip, mel3.to(device), n_iter, power)
    trim_plan_cache()
    if mel.dim() == 2:
        out = out.squeeze(0)
    out = out.to(mel.device)
    return out.to(half) if half else out


def mel_to_audio(mel, mel_fb, power=1.0, n_iter=100, method="griffin_lim", **kwargs):
    r"""Waveform (L,) / (B, L) behind a mel spectrogram (librosa's `mel_to_audio`): `mel_to_stft`, then `method`
    ("griffin_lim", "ADMM" or "RTISI_LA") on the magnitude with `**kwargs` (its own options and the stft arguments).  Exactly
    `griffin_lim(mel_to_stft(mel, mel_fb, power, n_iter, **kwargs), **kwargs)`."""
    if method not in _METHODS:
        raise ValueError(f"method must be one of {sorted(_METHODS)}, got {method!r}")
    mag = mel_to_stft(mel, mel_fb, power=power, n_iter=n_iter, **kwargs)
    return _METHODS[method](mag, **kwargs)


class _MelNnlsUnfoldedFn(torch.autograd.Function):
    """`n_iter` FISTA iterations of the mel NNLS as one differentiable layer.  The forward pass is `mel_to_stft`'s launch and
    saves the mel alone; the backward pass is one `specinv_mel_nnls_adjoint` launch, which recomputes the iteration per frame
    in LDS, keeps its active sets there and sweeps back."""

    @staticmethod
    def forward(ctx, mel3, plan, bank, n_iter, power):
        _nnls_setup(plan, *bank)
        most = C.c_int()
        _lib.check(plan.lib.specinv_mel_nnls_adjoint_max_iter(plan._h, C.byref(most)))
        if n_iter > most.value:                                    # (here, not inside backward())
            raise NotImplementedError(f"mel_to_stft_unfolded: {n_iter} iterations of a frame of {plan.n_freq} bins and {bank[0].shape[0]} "
                                      f"mel bands ({plan.dtype}) do not fit a CU's LDS in the backward pass: this shape admits "
                                      f"n_iter <= {most.value}")
        y = ingest(mel3, plan.device, plan.dtype)
        ctx.plan, ctx.bank, ctx.n_iter, ctx.power = plan, bank, n_iter, power
        ctx.save_for_backward(y)
        return _nnls(plan, *bank, y, n_iter, power)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        plan = ctx.plan
        y, = ctx.saved_tensors
        _nnls_setup(plan, *ctx.bank)                                # (the plan may have seen another filterbank since)
        g = plan._in(g_out, plan.dtype, (plan.batch, plan.n_freq, plan.n_frames))
        g_mel = torch.empty_like(y)
        _lib.check(plan.lib.specinv_mel_nnls_adjoint(plan._h, y.data_ptr(), int(ctx.n_iter), float(ctx.power), g.data_ptr(),
                                                     g_mel.data_ptr()))
        return g_mel, None, None, None, None


def mel_to_stft_unfolded(mel, mel_fb, power=1.0, n_iter=100, **stft_kwargs):
    r"""`mel_to_stft` as a layer to train through: `n_iter` FISTA iterations, differentiable in `mel`.

    The arguments, shapes, dtypes, devices and the plan are those of `mel_to_stft`; without a gradient to compute the result is
    `mel_to_stft(...)` itself.  With grad mode on and `mel` requiring grad the same launch runs and the result carries the
    gradient to `mel` (first order only), computed by one launch that recomputes the iteration per frame and sweeps it in reverse:
    nothing but `mel` is kept for it.  The derivative of max(0, u) at u = 0 and of the root at 0 is 0, so a silent frame and a band
    that touches no bin receive exact zeros.  `mel_fb` is a constant.  The unroll a frame admits is bounded by a CU's LDS (at 80
    bands 1136 iterations at n_fft 2048 in float32, 182 at n_fft 8192 in float64); a longer one raises `NotImplementedError`
    at this call.  At most 65535 items.
    """
    half, dtype, fb, key, lip, mel3, args = _checked("mel_to_stft_unfolded", mel, mel_fb, power, n_iter, stft_kwargs)
    B, T = mel3.shape[0], mel3.shape[2]
    if B > _MAX_PLAN_BATCH:
        raise ValueError(f"mel of shape {tuple(mel.shape)} holds {B} items, mel_to_stft_unfolded takes at most {_MAX_PLAN_BATCH}")
    if not (torch.is_grad_enabled() and mel.requires_grad):
        return mel_to_stft(mel, mel_fb, power=power, n_iter=n_iter, **stft_kwargs)
    device = require_gpu(mel.device)
    y = mel3.to(device=device, dtype=dtype)
    if B == 0 or T == 0:
        out = y.new_zeros((B, fb.shape[1], T)) + 0.0 * y.sum()     # (zeros whose gradient is zeros of mel's shape)
    else:
        out = _MelNnlsUnfoldedFn.apply(y, get_plan(args, B, T, dtype, device), (fb, key, lip), int(n_iter), float(power))
    trim_plan_cache()
    if mel.dim() == 2:
        out = out.squeeze(0)
    out = out.to(mel.device)
    return out.to(half) if half else out


def mel_to_audio_unfolded(mel, mel_fb, power=1.0, nnls_iter=100, n_iter=5, alpha=0.99, beta=None, gamma=1.0, **stft_kwargs):
    r"""Waveform behind a mel spectrogram as a layer to train through: exactly `agla_unfolded(mel_to_stft_unfolded(mel, mel_fb,
    power, nnls_iter, **stft_kwargs), n_iter, alpha, beta, gamma, **stft_kwargs)`."""
    mag = mel_to_stft_unfolded(mel, mel_fb, power=power, n_iter=nnls_iter, **stft_kwargs)
    return agla_unfolded(mag, n_iter, alpha, beta, gamma, **stft_kwargs)
