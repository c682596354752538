"""`spatial_covariance`, `beamform`, `beamform_apply` and `beamform_audio`: mask-based beamforming in one launch.
`wpe` hands back all the channels of a recording and everything after it - `denoise`, `consistent_wiener`, every inversion
method - takes one; this is the array step between them, the chain of the CHiME systems: WPE, a mask-based beamformer, a
single-channel post-filter.  The masks are what the package already produces: `spectral_gain`'s `G`, or a separator's.  The three
solutions are the reference-channel MVDR of Souden, Benesty and Affes ("On optimal frequency-domain multichannel linear filtering
for noise reduction", IEEE TASLP 2010), the MVDR on the principal eigenvector found by power iteration (torchaudio's `rtf_power`),
and the multichannel Wiener filter with the noise weight `mu`.

Definition (tests/_beamform_oracle.py is its float64 statement).  X is (C, F, T), the channels of one recording.  Per bin f, with
x_t = X[:, f, t], m the target mask, n the noise mask (1 - m when none is given) and tiny the smallest normal double:

    Phi(m)  = sum_t m_t x_t x_t^H / max(sum_t m_t, tiny)             Phi_s = Phi(mask_target), Phi_n = Phi(mask_noise)
    load(A) = A + (diag_load Re tr(A) / C + tiny) I
    souden:     A = load(Phi_n);  N = A^-1 Phi_s;  w = N[:, ref] / max(Re tr(N), tiny)
    rtf_power:  A, N as above;  v = N[:, ref];  (n_power_iter - 1) times:  v <- N (v / max(|Re v|_inf, |Im v|_inf, tiny));
                a = A v;  w = v conj(a[ref]) / max(Re(a^H v), tiny)
    mwf:        A = load(Phi_s + mu Phi_n);  w = A^-1 Phi_s[:, ref]
    Y[f, t] = w^H x_t

All sums, the factorisation and the solves are float64 for complex64 input as well; `Y` is rounded once to the input's dtype.  A
silent bin, an all-zero item or an all-zero mask gives Phi = 0, w = 0 and Y = 0 exactly, and nothing is ever NaN or Inf for finite
input.  Phi is returned before the loading.  T = 0 returns zeros.

Not part of the reference's surface.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from ._ingest import broadcasts_to, ingest, is_int, is_real
from .plan import _RECOGNISED, require_gpu

__all__ = ["spatial_covariance", "beamform", "beamform_apply", "beamform_audio"]

MAX_CHANNELS = 16              # (csrc/kernels_beamform.h: kBfMaxChannels)
MAX_POWER_ITER = 64            # n_power_iter: the launch's length is bounded (kBfMaxPowerIter)
TILE = 64                      # frames of a tile of the walk: the lane is the frame (kBfTile)
SOLUTIONS = tuple(_lib.BEAMFORM_SOLUTIONS)
_CPLX = (torch.complex64, torch.complex128)
_REAL = (torch.float16, torch.bfloat16, torch.float32, torch.float64)


def _checked_spec(spec, what):
    """(lead, channels, n_freq, n_frames): `lead` is the shape in front of the channel axis - () or (B,)."""
    if not isinstance(spec, torch.Tensor):
        raise TypeError("spec must be a torch.Tensor")
    if spec.dtype not in _CPLX:
        raise TypeError(f"spec must be complex64 or complex128 (no half precision, no real magnitudes), got dtype {spec.dtype}")
    if spec.dim() not in (2, 3, 4):
        raise ValueError(f"spec must be (F, T), (C, F, T) - the channels of one recording, not a batch - or (B, C, F, T), got shape "
                         f"{tuple(spec.shape)}")
    if torch.is_grad_enabled() and spec.requires_grad:
        raise NotImplementedError(f"{what} is not differentiable; detach the input")
    lead = tuple(spec.shape[:1]) if spec.dim() == 4 else ()
    channels = spec.shape[-3] if spec.dim() >= 3 else 1
    if channels > MAX_CHANNELS:
        raise NotImplementedError(f"channels must be <= {MAX_CHANNELS}, got {channels}")
    return lead, channels, spec.shape[-2], spec.shape[-1]


def _checked_mask(mask, name, want, what):
    if not isinstance(mask, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if mask.dtype not in _REAL:
        raise TypeError(f"{name} must be real (float16 / bfloat16 / float32 / float64), got dtype {mask.dtype}")
    if not broadcasts_to(mask.shape, want):
        raise ValueError(f"{name} of shape {tuple(mask.shape)} does not broadcast to {want}, spec's shape without the channel axis")
    if torch.is_grad_enabled() and mask.requires_grad:
        raise NotImplementedError(f"{what} is not differentiable; detach the inputs")
    if mask.numel() and not bool((mask.detach() >= 0).all()):
        raise ValueError(f"{name} must be non-negative")


def _checked_params(solution, ref_channel, channels, diag_load, n_power_iter, mu):
    if solution not in _lib.BEAMFORM_SOLUTIONS:
        raise ValueError(f"solution must be one of {SOLUTIONS}, got {solution!r}")
    if not is_int(ref_channel):
        raise TypeError(f"ref_channel must be an int, got {ref_channel!r}")
    if channels is not None and not 0 <= ref_channel < channels:
        raise ValueError(f"ref_channel must be in [0, {channels}), got {ref_channel}")
    if not is_int(n_power_iter) or n_power_iter < 1:
        raise ValueError(f"n_power_iter must be an int >= 1, got {n_power_iter!r}")
    if n_power_iter > MAX_POWER_ITER:
        raise NotImplementedError(f"n_power_iter must be <= {MAX_POWER_ITER} (the iterations run inside the one launch), got {n_power_iter}")
    for v, name in ((diag_load, "diag_load"), (mu, "mu")):
        if not is_real(v) or not (v >= 0 and math.isfinite(v)):
            raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")
    return _lib.BEAMFORM_SOLUTIONS[solution], ref_channel, float(diag_load), n_power_iter, float(mu)


def _launch(spec, lead, channels, n_freq, n_frames, mask_t, mask_n, weights, params, want_y, want_w, want_scm):
    """One launch.  Returns (Y, w, Phi_s, Phi_n) on spec's device, None where not asked for."""
    y_shape, w_shape, s_shape = lead + (n_freq, n_frames), lead + (n_freq, channels), lead + (n_freq, channels, channels)
    if spec.numel() == 0:
        z = lambda shape, dtype: spec.new_zeros(shape, dtype=dtype)      # noqa: E731
        return (z(y_shape, spec.dtype) if want_y else None, z(w_shape, torch.complex128) if want_w else None,
                z(s_shape, torch.complex128) if want_scm else None, z(s_shape, torch.complex128) if want_scm and want_y else None)
    device = require_gpu(spec.device)
    s4 = ingest(spec.reshape((-1, channels, n_freq, n_frames)), device, spec.dtype)
    batch = s4.shape[0]
    as_mask = lambda m: None if m is None else ingest(m.expand(y_shape).reshape(batch, n_freq, n_frames), device, torch.float64)   # noqa: E731
    mt, mn = as_mask(mask_t), as_mask(mask_n)
    w_in = None if weights is None else ingest(weights.reshape(batch, n_freq, channels), device, torch.complex128)
    new = lambda on, shape, dtype: torch.empty(shape, dtype=dtype, device=device) if on else None      # noqa: E731
    out = new(want_y, (batch, n_freq, n_frames), spec.dtype)
    w_out = new(want_w, (batch, n_freq, channels), torch.complex128)
    scm_t = new(want_scm, (batch, n_freq, channels, channels), torch.complex128)
    scm_n = new(want_scm and want_y, (batch, n_freq, channels, channels), torch.complex128)      # (not for spatial_covariance)
    solution, ref, diag_load, n_power_iter, mu = params
    _lib.call_op("specinv_beamform", (s4, mt, mn, w_in, out, w_out, scm_t, scm_n, batch, channels, n_freq, n_frames, solution, ref,
                                      n_power_iter, diag_load, mu), spec.dtype != torch.complex64, device)
    back = lambda t, shape: None if t is None else t.reshape(shape).to(device=spec.device)       # noqa: E731
    return back(out, y_shape), back(w_out, w_shape), back(scm_t, s_shape), back(scm_n, s_shape)


_NO_PARAMS = (_lib.BEAMFORM_SOLUTIONS["souden"], 0, 0.0, 1, 1.0)


def spatial_covariance(spec, mask=None):
    r"""The mask-weighted spatial covariance `Phi(mask)` of the module's definition: complex128 (..., F, C, C), exactly Hermitian,
    on `spec`'s device.  `spec` is (F, T) (C = 1), (C, F, T) - the channels of one recording - or (B, C, F, T), complex64 or
    complex128; `mask` is real, non-negative and broadcastable to `spec`'s shape without the channel axis, `None` is all ones.  It
    is `beamform`'s launch in a covariance-only mode: with the `mask_target` of a `beamform(..., return_scm=True)` call it equals
    that call's `Phi_s` bit for bit.  Limits as `beamform`."""
    lead, channels, n_freq, n_frames = _checked_spec(spec, "spatial_covariance")
    if mask is not None:
        _checked_mask(mask, "mask", lead + (n_freq, n_frames), "spatial_covariance")
    return _launch(spec, lead, channels, n_freq, n_frames, mask, None, None, _NO_PARAMS, False, False, True)[2]


def beamform(spec, mask_target, mask_noise=None, solution="souden", ref_channel=0, diag_load=1e-7, n_power_iter=3, mu=1.0,
             return_weights=False, return_scm=False):
    r"""A multi-channel complex spectrogram beamformed to one channel: `Y`, of `spec`'s dtype (complex64 or complex128) and device,
    with the channel axis removed.  The definition is the module's.

    `spec` is (C, F, T) for the C channels of ONE recording - the leading axis of a 3-D input is channels, not a batch - or
    (B, C, F, T) for a batch; (F, T) is C = 1.  Items are processed independently: item b of a batch gives the bits it gives
    alone.  `mask_target` and `mask_noise` are real (float16 / bfloat16 / float32 / float64, read as float64), non-negative and
    broadcastable to `spec`'s shape without the channel axis - (F, 1), (1, T) and 0-d are valid; `mask_noise=None` is
    `1 - mask_target`, formed in float64.

    `solution` is "souden", "rtf_power" (`n_power_iter` >= 1 steps) or "mwf" (`mu` >= 0 weighs the noise); `ref_channel` in
    [0, C) is the channel whose target component the result estimates; `diag_load` >= 0 adds that fraction of the mean diagonal
    to the matrix that is inverted.

    `return_weights=True` adds `w`, complex128 (..., F, C); `return_scm=True` adds `Phi_s` and `Phi_n`, complex128 (..., F, C, C),
    before the loading.  The result is `Y` or the tuple `(Y[, w][, Phi_s, Phi_n])`.

    Limits: C <= 16, n_power_iter <= 64; any F, T, B.  Offline only, one target, one `ref_channel` for all items.  Not
    differentiable.  No half-precision `spec`, no sharded form, no `frame_major` form.  Any layout torch can express is read as
    torch would read it.  A CPU tensor is computed on the current HIP device and comes back.
    """
    lead, channels, n_freq, n_frames = _checked_spec(spec, "beamform")
    want = lead + (n_freq, n_frames)
    if mask_target is None:
        raise TypeError("mask_target must be a torch.Tensor")
    _checked_mask(mask_target, "mask_target", want, "beamform")
    if mask_noise is not None:
        _checked_mask(mask_noise, "mask_noise", want, "beamform")
    params = _checked_params(solution, ref_channel, channels, diag_load, n_power_iter, mu)
    y, w, ps, pn = _launch(spec, lead, channels, n_freq, n_frames, mask_target, mask_noise, None, params, True, return_weights, return_scm)
    res = (y,) + ((w,) if return_weights else ()) + ((ps, pn) if return_scm else ())
    return res[0] if len(res) == 1 else res


def beamform_apply(spec, weights):
    r"""`Y[f, t] = w^H[f] x[f, t]` for given weights: `spec` as in `beamform`, `weights` the `w` of a
    `beamform(..., return_weights=True)` call - complex, (..., F, C).  Estimate on one block and apply to another, or apply
    weights of your own.  It is `beamform`'s launch in a filter-only mode: with the `w` and `spec` of one `beamform` call the
    result equals that call's `Y` bit for bit.  Limits as `beamform`."""
    lead, channels, n_freq, n_frames = _checked_spec(spec, "beamform_apply")
    if not isinstance(weights, torch.Tensor):
        raise TypeError("weights must be a torch.Tensor")
    if weights.dtype not in _CPLX:
        raise TypeError(f"weights must be complex64 or complex128, got dtype {weights.dtype}")
    if tuple(weights.shape) != lead + (n_freq, channels):
        raise ValueError(f"weights must be of shape {lead + (n_freq, channels)}, got {tuple(weights.shape)}")
    if torch.is_grad_enabled() and weights.requires_grad:
        raise NotImplementedError("beamform_apply is not differentiable; detach the inputs")
    return _launch(spec, lead, channels, n_freq, n_frames, None, None, weights, _NO_PARAMS, True, False, False)[0]


def beamform_audio(x, n_fft=None, mask_target=None, mask_noise=None, solution="souden", ref_channel=0, diag_load=1e-7, n_power_iter=3,
                   mu=1.0, **stft_kwargs):
    r"""A multi-channel waveform (C, L) - the channels of one recording - or (B, C, L) beamformed to one channel: (L',) or (B, L').
    With X = stft(x, n_fft, **stft_kwargs), the leading axes flattened for the transform, it is exactly

        istft(beamform(X, mask_target, mask_noise, solution, ref_channel, diag_load, n_power_iter, mu), **stft_kwargs)

    the composition of the public calls, bit for bit.  With `mask_target=None` the mask is
    `spectral_gain(X[..., ref_channel, :, :])` with that function's defaults.  The options are `beamform`'s, `**stft_kwargs` are
    `stft`'s (`hop_length`, `window`, ...; `n_fft` defaults as there).  Not differentiable.
    """
    from .enhance import spectral_gain
    from .projection import istft, stft
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    if x.dim() not in (2, 3):
        raise ValueError(f"x must be (C, L) - the channels of one recording - or (B, C, L), got shape {tuple(x.shape)}")
    if x.shape[-2] > MAX_CHANNELS:
        raise NotImplementedError(f"channels must be <= {MAX_CHANNELS}, got {x.shape[-2]}")
    _checked_params(solution, ref_channel, x.shape[-2], diag_load, n_power_iter, mu)
    if torch.is_grad_enabled() and x.requires_grad:
        raise NotImplementedError("beamform_audio is not differentiable; detach the input")
    kw = {k: v for k, v in stft_kwargs.items() if k in _RECOGNISED}
    X = stft(x.reshape(-1, x.shape[-1]), n_fft, **kw)
    X = X.reshape(tuple(x.shape[:-1]) + tuple(X.shape[-2:]))
    if mask_target is None:
        mask_target = spectral_gain(X[..., ref_channel, :, :])
    Y = beamform(X, mask_target, mask_noise, solution, ref_channel, diag_load, n_power_iter, mu)
    y = istft(Y.reshape((-1,) + tuple(Y.shape[-2:])), **kw)
    return y.reshape(tuple(x.shape[:-2]) + (y.shape[-1],))
