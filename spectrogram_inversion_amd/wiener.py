"""`consistent_wiener`: Wiener filtering under a consistency penalty (Le Roux & Vincent, "Consistent Wiener filtering for audio
source separation", IEEE SPL 2013).  A mask-based separator (`hpss`, any network) gives a Wiener-type estimate, a real gain times
the mixture's STFT; `misi` makes magnitudes into waveforms that add up to the mixture.  This keeps the Wiener statistics and also
asks for a spectrogram that is the STFT of a signal: the element-wise work of a conjugate-gradient loop in csrc/kernels_cwf.h
around the library's four transforms.

Definition, per item.  X = `mix_spec`, complex, one-sided, (F, T); v_s = `var_target`, v_n = `var_noise`, real and >= 0,
broadcastable to X; a = `hop_length`, N = `n_fft`.  All scalars and sums are float64 whatever the input dtype, arrays are held in
the input's dtype.

    m      = floor * max_{f,t}(v_s + v_n)         m == 0: the item's result is S = 0 and it takes no part in what follows
    v_s, v_n <- max(v_s, m), max(v_n, m)
    Lam    = 1/v_s + 1/v_n
    g      = gamma / mean_{f,t}(v_s v_n / (v_s + v_n))   if relative (the default), else gamma
    G Z    = STFT(ISTFT(Z))                       the library's transforms with **stft_kwargs
    G' U   = istft_adjoint(stft_adjoint(U))       the real adjoint of G: <G a, b> = <a, G' b>
    <a, b> = sum_{f,t} Re a Re b + Im a Im b      over the one-sided bins of the item, unweighted
    A P    = Lam P + g (u - G' u),  u = P - G P
    M      = Lam + g (1 - a/N)                    diagonal preconditioner

S is the `n_iter`-th iterate of preconditioned conjugate gradients on A S = X / v_n, the stationarity condition of

    sum |X - S|^2 / v_n + |S|^2 / v_s + g |S - G S|^2

started from the Wiener estimate:

    S_0 = v_s / (v_s + v_n) X
    r = X / v_n - A S_0 ;  z = r / M ;  p = z ;  rz = <r, z> ;  rz0 = rz
    each iteration:
        q = A p ;  alpha = rz / <p, q> ;  S += alpha p ;  r -= alpha q ;  z = r / M ;  rz' = <r, z>
        beta = rz' / rz ;  p = z + beta p ;  rz = rz'

An item whose `rz` is 0 or whose `<p, q>` is not > 0 is finished: alpha = beta = 0 from then on.  An all-zero mixture is such an
item.  Every item has its own scalars: an item's result does not depend on what else is in the batch.  N = X - S, formed once at the
end.

G is not self-adjoint under this inner product (with `center=True` and reflect padding `<G a, b> - <a, G b>` is of the size of the
products themselves), so G' is the two adjoint transforms and not a second G: four transforms per iteration.

Not part of the reference's surface.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers

import torch

from . import _lib
from . import methods as _m
from ._ingest import ingest
from .plan import _RECOGNISED, args_helper, get_plan, require_gpu, trim_plan_cache

__all__ = ["consistent_wiener", "consistent_wiener_audio"]

_MAX_PLAN_BATCH = _m._MAX_PLAN_BATCH
_COMPLEX = {torch.complex32: torch.float32, torch.complex64: torch.float32, torch.complex128: torch.float64}
_REAL = (torch.float16, torch.bfloat16, torch.float32, torch.float64)


def _checked_options(gamma, n_iter, tol, eva_iter, floor):
    if isinstance(gamma, bool) or not isinstance(gamma, numbers.Real) or not (gamma > 0 and math.isfinite(gamma)):
        raise ValueError(f"gamma must be a finite number > 0, got {gamma!r}")
    if isinstance(floor, bool) or not isinstance(floor, numbers.Real) or not 0 < floor < 1:
        raise ValueError(f"floor must be a number in (0, 1), got {floor!r}")
    if isinstance(n_iter, bool) or not isinstance(n_iter, int) or n_iter < 0:
        raise ValueError(f"n_iter must be an int >= 0, got {n_iter!r}")
    if isinstance(tol, bool) or not isinstance(tol, numbers.Real) or not tol >= 0:
        raise ValueError(f"tol must be a number >= 0, got {tol!r}")
    if isinstance(eva_iter, bool) or not isinstance(eva_iter, int) or eva_iter < 1:
        raise ValueError(f"eva_iter must be an int >= 1, got {eva_iter!r}")


def _checked_variance(v, name, shape):
    if not isinstance(v, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if v.dtype not in _REAL:
        raise TypeError(f"{name} must be real (float16 / bfloat16 / float32 / float64), got dtype {v.dtype}")
    try:
        ok = torch.broadcast_shapes(tuple(v.shape), tuple(shape)) == tuple(shape)
    except RuntimeError:
        ok = False
    if not ok:
        raise ValueError(f"{name} of shape {tuple(v.shape)} does not broadcast to mix_spec's {tuple(shape)}")
    if torch.is_grad_enabled() and v.requires_grad:
        raise NotImplementedError("consistent_wiener is not differentiable; detach the inputs")


def consistent_wiener(mix_spec, var_target, var_noise, gamma=1.0, n_iter=30, tol=0.0, eva_iter=10, floor=1e-8, relative=True,
                      return_info=False, **stft_kwargs):
    r"""The mixture's spectrogram (F, T) / (B, F, T), complex and one-sided, split into `(S, N)`: the target under the Wiener
    statistics `var_target`, `var_noise` (real, >= 0, broadcastable to `mix_spec`: a (F, 1) noise profile, a scalar tensor) and a
    consistency penalty of weight `gamma`, and the rest `N = mix_spec - S`.  Both are complex, of `mix_spec`'s shape, dtype family
    and device.  The definition is the module's.

    `gamma`, finite and > 0, weighs |S - STFT(ISTFT(S))|^2; with `relative=True` it is taken relative to the item's mean Wiener
    error variance, which makes the result scale with the input (X c with v c^2 gives S c).  `n_iter` conjugate-gradient iterations
    are run, `n_iter=0` returns the Wiener estimate.  `tol > 0` reads the residuals back after every `eva_iter`-th iteration and
    stops when every item is at or below `tol`; `tol=0` reads nothing back before the end.  `floor`, in (0, 1), bounds the
    variances from below relative to the item's largest `var_target + var_noise`.  `**stft_kwargs` are read as everywhere
    (`hop_length`, `win_length`, `window`, `center`, `pad_mode`, `normalized`); `n_fft` is 2 (F - 1).

    `return_info=True` adds a dict: `residual`, float64 (B,), sqrt(rz / rz0) per item and 0 for finished items, and `n_iter`, the
    iterations run.

    complex32 is computed as complex64 and rounded back.  CPU tensors are computed on the current HIP device and come back to the
    CPU.  At most 65535 items.  One-sided spectrograms only.  Not differentiable.  A running method on a cached plan is not
    disturbed.
    """
    if not isinstance(mix_spec, torch.Tensor):
        raise TypeError("mix_spec must be a torch.Tensor")
    if mix_spec.dtype not in _COMPLEX:
        raise TypeError(f"mix_spec must be complex, got dtype {mix_spec.dtype}")
    if mix_spec.dim() not in (2, 3):
        raise ValueError(f"mix_spec must be (F, T) or (B, F, T), got shape {tuple(mix_spec.shape)}")
    if mix_spec.shape[-1] < 1 or mix_spec.shape[-2] < 2:
        raise ValueError(f"mix_spec of shape {tuple(mix_spec.shape)} holds no one-sided spectrogram")
    _checked_variance(var_target, "var_target", mix_spec.shape)
    _checked_variance(var_noise, "var_noise", mix_spec.shape)
    _checked_options(gamma, n_iter, tol, eva_iter, floor)
    if stft_kwargs.get("onesided", None) is False:
        raise NotImplementedError("consistent_wiener takes one-sided spectrograms only")
    window = stft_kwargs.get("window", None)
    if window is not None and window.is_complex():
        raise NotImplementedError("consistent_wiener takes one-sided spectrograms only: a complex window makes a two-sided one")
    if torch.is_grad_enabled() and mix_spec.requires_grad:
        raise NotImplementedError("consistent_wiener is not differentiable; detach the inputs")
    batch = mix_spec.shape[0] if mix_spec.dim() == 3 else 1
    if batch > _MAX_PLAN_BATCH:
        raise ValueError(f"mix_spec of shape {tuple(mix_spec.shape)} holds {batch} items, consistent_wiener takes at most "
                         f"{_MAX_PLAN_BATCH}")
    rdtype = _COMPLEX[mix_spec.dtype]
    cdtype = torch.complex64 if rdtype == torch.float32 else torch.complex128
    args = args_helper(torch.empty((mix_spec.shape[-2], 1), dtype=rdtype, device="meta"), **stft_kwargs)
    if batch == 0:
        S, N = torch.zeros_like(mix_spec), torch.zeros_like(mix_spec)
        info = {"residual": torch.zeros(0, dtype=torch.float64, device=mix_spec.device), "n_iter": 0}
        return (S, N, info) if return_info else (S, N)

    device = require_gpu(mix_spec.device)
    shape3 = (batch,) + tuple(mix_spec.shape[-2:])
    x3 = ingest(mix_spec.reshape(shape3), device, cdtype)
    vs3 = ingest(var_target.expand(mix_spec.shape).reshape(shape3), device, rdtype)
    vn3 = ingest(var_noise.expand(mix_spec.shape).reshape(shape3), device, rdtype)
    plan = get_plan(args, batch, shape3[2], rdtype, device)
    plan._sync_stream()
    S = torch.empty(shape3, dtype=cdtype, device=device)
    N = torch.empty(shape3, dtype=cdtype, device=device)
    residual = (C.c_double * batch)()
    iters = C.c_int(0)
    _lib.check(plan.lib.specinv_cwf_run(plan._h, x3.data_ptr(), vs3.data_ptr(), vn3.data_ptr(), float(gamma), int(bool(relative)),
                                        float(floor), n_iter, eva_iter, float(tol), S.data_ptr(), N.data_ptr(),
                                        residual if return_info else None, C.byref(iters)))
    trim_plan_cache()
    S = S.reshape(mix_spec.shape).to(device=mix_spec.device, dtype=mix_spec.dtype)
    N = N.reshape(mix_spec.shape).to(device=mix_spec.device, dtype=mix_spec.dtype)
    if not return_info:
        return S, N
    info = {"residual": torch.tensor(list(residual), dtype=torch.float64, device=mix_spec.device), "n_iter": int(iters.value)}
    return S, N, info


def consistent_wiener_audio(x, var_target, var_noise, n_fft=None, gamma=1.0, n_iter=30, tol=0.0, eva_iter=10, floor=1e-8,
                            relative=True, return_info=False, **stft_kwargs):
    r"""A waveform (L,) / (B, L) split into `(x_s, x_n)`: with `X = stft(x, n_fft, **stft_kwargs)` and `S` from
    `consistent_wiener(X, var_target, var_noise, ...)`, `x_s = istft(S, **stft_kwargs)` of length L', and `x_n = x[..., :L'] - x_s`,
    so that the two add up to the input (to the rounding of that difference).  The variances are over the bins of `X`.  `n_fft` defaults as in `stft`; the other
    arguments and rules are `consistent_wiener`'s, and `return_info=True` adds its dict."""
    from .projection import istft, stft
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    _checked_options(gamma, n_iter, tol, eva_iter, floor)
    if torch.is_grad_enabled() and x.requires_grad:
        raise NotImplementedError("consistent_wiener_audio is not differentiable; detach the inputs")
    kw = {k: v for k, v in stft_kwargs.items() if k in _RECOGNISED}
    X = stft(x, n_fft, **kw)
    out = consistent_wiener(X, var_target, var_noise, gamma, n_iter, tol, eva_iter, floor, relative, return_info, **kw)
    x_s = istft(out[0], **kw).to(x.dtype)
    x_n = x[..., :x_s.shape[-1]] - x_s
    return (x_s, x_n, out[2]) if return_info else (x_s, x_n)
