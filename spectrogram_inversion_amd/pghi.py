"""`rtpghi`: phase gradient heap integration in its real-time form with one look-ahead frame (Prusa, Balazs & Sondergaard 2017;
Prusa & Sondergaard 2016), a phase for magnitudes alone in one kernel launch (csrc/kernels_pghi.h).  It is the
non-iterative estimate LTFAT, phaseret and tifresi ship, and the start the paper recommends for fast Griffin-Lim:

    x = si.accelerated_griffin_lim(si.rtpghi(mag, **kw), **kw)

and the same into `griffin_lim`, `ADMM`, `misi` or `constrained_griffin_lim`.

Definition, per item.  N = `n_fft`, a = `hop_length`, F = N/2 + 1, s[m,n] the magnitudes, g = `gamma`.  All arithmetic is float64
whatever the input dtype.

    floor = tol * max(0, max s)                 (m,n) is live iff s > 0 and s >= floor
    l[m,n] = log(max(s, floor)),  mirrored in frequency: l[-1] = l[1], l[F] = l[F-2]       (no live bin: l is never evaluated)
    wt[m,n] = (2 pi / N) * ((a m) mod N) + (a N / g) * ((l[m+1,n] - l[m-1,n]) / 2)         (a m reduced as an integer)
    wf[m,n] = pi - (g / (a N)) * D[m,n]
    D[m,n]  = (l[m,n+1] - l[m,n-1]) / 2 for 0 < n < T-1;  l[m,1] - l[m,0] and l[m,T-1] - l[m,T-2] at the ends;  0 for T = 1

The pi is `torch.stft`'s phase convention: a frame starts at sample 0 and the window centre sits at N/2.  For a Gaussian window
exp(-pi t^2 / g) and a frame-centred phase, d phi / dt = 2 pi xi + (1/g) d log|V| / d xi and d phi / d xi = -g d log|V| / dt.

Frame n, given frame n-1:

    c[m] = s[m,n] if live else -inf;   p[m] = s[m,n-1] if (m,n-1) is live else -inf
    n = 0: p[m] = -inf, but the lowest-index maximum of s[:,0] has p = +inf if it is live
    Lf[0] = -inf,    Lf[m] = min(c[m-1], max(p[m-1], Lf[m-1]))
    Rg[F-1] = -inf,  Rg[m] = min(c[m+1], max(p[m+1], Rg[m+1]))
    parent of a live bin, b = max(p[m], Lf[m], Rg[m]):  code 0 if p[m] >= b (time wins ties, and when all three are -inf),
        else code 1 if Lf[m] >= b, else code 2;  a bin that is not live has code 3
    code 0: phi[m,n] = phi[m,n-1] + (wt[m,n-1] + wt[m,n]) / 2, in frame 0 exactly 0
    code 1: phi[m,n] = phi[m-1,n] + (wf[m-1,n] + wf[m,n]) / 2
    code 2: phi[m,n] = phi[m+1,n] - (wf[m+1,n] + wf[m,n]) / 2
    code 3: phi = 0, and that 0 is what a later time step reads
    result (s cos phi, s sin phi), evaluated in float64 and rounded once

This is RTPGHI's heap: it holds frame n-1 with keys p, a popped bin sets its unset neighbours and pushes them with key c, so a bin
is set by the candidate with the widest max-min path, and x -> min(c, max(p, x)) composes associatively.  Every decision compares
input values exactly.  NaN input is unspecified.

Not part of the reference's surface.
"""
from __future__ import annotations

import math
import numbers

import torch

from . import _lib
from ._ingest import ingest
from .plan import args_helper, require_gpu

__all__ = ["rtpghi", "HANN_GAMMA", "HAMMING_GAMMA"]

HANN_GAMMA = 0.25645          # gamma / win_length^2 of the Hann window (Prusa, Balazs & Sondergaard 2017)
HAMMING_GAMMA = 0.29794       # ... of the Hamming window
_MAX_FFT = 5828               # the kernel's limit: above it a frame's state no longer fits a compute unit's LDS
_REAL = {torch.float16: torch.float32, torch.float32: torch.float32, torch.float64: torch.float64}


def rtpghi(spec, gamma=None, tol=1e-6, return_phase=False, return_parents=False, **stft_kwargs):
    r"""Magnitudes (F, T) / (B, F, T), real and non-negative, with the phase RTPGHI integrates from their gradients: a complex
    tensor `spec * exp(1j * phi)` of `spec`'s shape, dtype family and device.  The definition is the module's.

    `gamma` is the Gaussian-equivalent width of the analysis window in samples^2, finite and > 0; `None` is the Hann window's
    `0.25645 * win_length**2`, and `0.29794 * win_length**2` is the published Hamming value.  `tol`, 0 < tol < 1, is the relative
    magnitude floor: bins below `tol` times the item's maximum are not integrated and get phase 0.  `**stft_kwargs` are read as
    everywhere (`hop_length`, `win_length`, `window`, `onesided`); `n_fft` is 2 (F - 1), at most 5828, and may be given to be checked
    against F: an odd one, which has the same bin count as the even one below it, is not implemented.

    `return_phase=True` also returns the unwrapped float64 phase (B, F, T); `return_parents=True` also returns the int8 codes
    (B, F, T): 0 time direction, 1 from bin m - 1, 2 from bin m + 1, 3 below the floor.  Both exist for tests and diagnostics.

    float16 is computed as float32 and rounded back.  A CPU tensor is computed on the current HIP device and comes back to the
    CPU.  Any number of items; no plan is made and a running method is not disturbed.  Not differentiable.
    """
    if not isinstance(spec, torch.Tensor):
        raise TypeError("spec must be a torch.Tensor")
    if spec.dtype not in _REAL:
        raise TypeError(f"spec must hold real magnitudes (float16, float32 or float64), got dtype {spec.dtype}")
    if gamma is not None and (isinstance(gamma, bool) or not isinstance(gamma, numbers.Real)
                              or not (gamma > 0 and math.isfinite(gamma))):
        raise ValueError(f"gamma must be a finite number > 0 or None, got {gamma!r}")
    if isinstance(tol, bool) or not isinstance(tol, numbers.Real) or not 0 < tol < 1:
        raise ValueError(f"tol must be a number in (0, 1), got {tol!r}")
    if spec.dim() not in (2, 3):
        raise ValueError(f"spec must be (F, T) or (B, F, T), got shape {tuple(spec.shape)}")
    if spec.shape[-1] < 1 or spec.shape[-2] < 1:
        raise ValueError(f"spec of shape {tuple(spec.shape)} holds no bins")
    if spec.shape[-1] >= 1 << 31:
        raise ValueError(f"spec of shape {tuple(spec.shape)}: T must be below 2^31")
    if stft_kwargs.get("onesided", None) is False:
        raise NotImplementedError("rtpghi takes one-sided spectrograms only")
    window = stft_kwargs.get("window", None)
    if window is not None and window.is_complex():
        raise NotImplementedError("rtpghi takes one-sided spectrograms only: a complex window makes a two-sided one")
    if spec.shape[-2] < 2:
        raise ValueError(f"spec of shape {tuple(spec.shape)}: a one-sided spectrogram has at least 2 bins")
    n_fft = stft_kwargs.get("n_fft", None)
    if n_fft is not None:
        if isinstance(n_fft, bool) or not isinstance(n_fft, int) or n_fft < 2:
            raise ValueError(f"n_fft must be an int >= 2, got {n_fft!r}")
        if n_fft % 2:
            raise NotImplementedError(f"rtpghi takes an even n_fft only, got {n_fft}")
        if n_fft // 2 + 1 != spec.shape[-2]:
            raise ValueError(f"spec of shape {tuple(spec.shape)} does not hold the {n_fft // 2 + 1} bins of n_fft {n_fft}")
    args = args_helper(spec, **stft_kwargs)
    if args.n_fft > _MAX_FFT:
        raise NotImplementedError(f"rtpghi: n_fft {args.n_fft} is beyond the kernel's limit of {_MAX_FFT}")
    if torch.is_grad_enabled() and spec.requires_grad:
        raise NotImplementedError("rtpghi is not differentiable; detach the input")
    # (win_length as the caller gave it: args_helper widens a shorter window to n_fft by zero padding, gamma is the window's own)
    win_length = stft_kwargs.get("win_length", None) or args.n_fft
    gamma = HANN_GAMMA * float(win_length) ** 2 if gamma is None else float(gamma)
    dtype = _REAL[spec.dtype]
    cdtype = torch.complex64 if dtype == torch.float32 else torch.complex128
    out_dtype = {torch.float16: torch.complex32, torch.float32: torch.complex64, torch.float64: torch.complex128}[spec.dtype]
    shape3 = (-1,) + tuple(spec.shape[-2:])
    batch = spec.numel() // (spec.shape[-2] * spec.shape[-1])
    if batch == 0:
        res = [spec.new_zeros(spec.shape, dtype=out_dtype)]
        if return_phase:
            res.append(spec.new_zeros((0,) + tuple(spec.shape[-2:]), dtype=torch.float64))
        if return_parents:
            res.append(spec.new_zeros((0,) + tuple(spec.shape[-2:]), dtype=torch.int8))
        return res[0] if len(res) == 1 else tuple(res)
    device = require_gpu(spec.device)
    s3 = ingest(spec.reshape(shape3), device, dtype)
    out = torch.empty(s3.shape, dtype=cdtype, device=device)
    phase = torch.empty(s3.shape, dtype=torch.float64, device=device) if return_phase else None
    parents = torch.empty(s3.shape, dtype=torch.int8, device=device) if return_parents else None
    _lib.call_op("specinv_pghi", (s3, out, phase, parents, s3.shape[0], s3.shape[1], s3.shape[2], args.n_fft, args.hop_length, gamma,
                                  float(tol)), dtype != torch.float32, device)
    res = [out.reshape(spec.shape).to(device=spec.device, dtype=out_dtype)]
    if return_phase:
        res.append(phase.to(spec.device))
    if return_parents:
        res.append(parents.to(spec.device))
    return res[0] if len(res) == 1 else tuple(res)
