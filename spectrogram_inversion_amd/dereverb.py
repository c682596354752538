"""`wpe`, `wpe_apply` and `dereverb`: weighted prediction error dereverberation in one launch.  `denoise` answers
additive noise; this is the answer to the other degradation of a far-field recording, and the package's first multi-channel entry
point: the offline WPE of Nakatani et al. ("Speech dereverberation based on variance-normalized delayed linear prediction", IEEE
TASLP 2010), the form `nara_wpe` made common.  Per frequency bin the late reverberant tail of a frame is predicted from the frames
at least `delay` back by a linear filter over all channels, fitted by least squares weighted with the reciprocal of the
dereverberated signal's own power, which is re-estimated `n_iter` times.

Definition (tests/_wpe_oracle.py is its float64 statement).  X is (C, F, T), the channels of one recording; K = taps, D = C K.
Per bin f, with x_t = X[:, f, t]:

    xs_t    in C^D, entry (c', k) at row c' K + k = X[c', f, t - delay - k], zero where that frame index is negative
    q_t     = mean_c |Y[c, f, t]|^2, Y the previous iteration's result (in float64, before any rounding); in the first iteration
              Y = X, or q_t = power[f, t] when `power` is given
    p_t     = the mean of q over the frames t - psd_context ... t + psd_context that exist
    lam_t   = max(p_t, eps max_t p_t, tiny), tiny the smallest normal double
    R       = sum_t xs_t xs_t^H / lam_t          P = sum_t xs_t x_t^H / lam_t  (D x C)
    R      <- R + (diag_load tr(R) / D + tiny) I
    G       = R^-1 P                              Y[:, f, t] = x_t - G^H xs_t

All sums, the factorisation and the solve are float64 for complex64 input as well; the result is rounded once to the input's
dtype.  A silent bin gives G = 0 and Y = X = 0, and nothing is ever NaN or Inf for finite input, an all-zero item included.
`n_iter=0` returns X (and G = 0); T <= delay is valid and returns X; `delay=0` is rejected - the filter would predict a frame
from itself and return zeros.

Not part of the reference's surface.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from ._ingest import broadcasts_to, ingest, is_int, is_real
from .plan import _RECOGNISED, require_gpu

__all__ = ["wpe", "wpe_apply", "dereverb"]

MAX_UNKNOWNS = 64              # channels x taps (csrc/kernels_wpe.h: kWpeMaxD)
MAX_CONTEXT = 64               # psd_context: the context mean reads 2 psd_context + 1 values a frame (kWpeMaxContext)
MAX_ITER = 100                 # n_iter: every iteration runs inside the one launch (kWpeMaxIter)
TILE_FRAMES = 32             # frames of a tile of the walk (kWpeTile); 16 beyond 32 channels (kWpeTileWide, kWpeWideChannels)
_CPLX = (torch.complex64, torch.complex128)
_REAL = (torch.float16, torch.bfloat16, torch.float32, torch.float64)


def _int(v, name, lo):
    if not is_int(v) or v < lo:
        raise ValueError(f"{name} must be an int >= {lo}, got {v!r}")
    return v


def _checked_delay(delay):
    if not is_int(delay):
        raise ValueError(f"delay must be an int >= 1, got {delay!r}")
    if delay < 1:
        raise ValueError(f"delay must be >= 1 (at 0 the filter predicts a frame from itself and the result is zero), got {delay!r}")
    return min(delay, (1 << 62))


def _checked_params(taps, delay, n_iter, psd_context, eps, diag_load):
    _int(taps, "taps", 1)
    delay = _checked_delay(delay)
    _int(n_iter, "n_iter", 0)
    _int(psd_context, "psd_context", 0)
    if n_iter > MAX_ITER:
        raise NotImplementedError(f"n_iter must be <= {MAX_ITER} (all iterations run in one launch), got {n_iter}")
    if psd_context > MAX_CONTEXT:
        raise NotImplementedError(f"psd_context must be <= {MAX_CONTEXT} (a frame's power is averaged over 2 psd_context + 1 reads), "
                                  f"got {psd_context}")
    for v, name in ((eps, "eps"), (diag_load, "diag_load")):
        if not is_real(v) or not (v >= 0 and math.isfinite(v)):
            raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")
    return taps, delay, n_iter, psd_context, float(eps), float(diag_load)


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
    return lead, channels, spec.shape[-2], spec.shape[-1]


def _checked_unknowns(channels, taps):
    if channels * taps > MAX_UNKNOWNS:
        raise NotImplementedError(f"channels x taps must be <= {MAX_UNKNOWNS}, got {channels} x {taps} = {channels * taps}")


def _launch(spec, lead, channels, n_freq, n_frames, taps, delay, n_iter, ctx, eps, diag_load, power, filt, want_filter, want_power):
    """One launch.  Returns (Y, G or None, lam or None) on spec's device."""
    d = channels * taps
    g_shape = lead + (n_freq, channels, taps, channels)
    if spec.numel() == 0:
        return (spec.new_zeros(spec.shape), spec.new_zeros(g_shape, dtype=torch.complex128) if want_filter else None,
                spec.new_zeros(lead + (n_freq, n_frames), dtype=torch.float64) if want_power else None)
    device = require_gpu(spec.device)
    s4 = ingest(spec.reshape((-1, channels, n_freq, n_frames)), device, spec.dtype)
    batch = s4.shape[0]
    out = torch.empty_like(s4)
    pw = g_in = g_out = lam = scratch = None
    if filt is not None:
        g_in = ingest(filt.reshape(batch, n_freq, d, channels), device, torch.complex128)
    else:
        if power is not None:
            pw = ingest(power.expand(lead + (n_freq, n_frames)).reshape(batch, n_freq, n_frames), device, torch.float64)
        lam = torch.empty((batch, n_freq, n_frames), dtype=torch.float64, device=device)
        if ctx > 0:
            scratch = torch.empty_like(lam)
        if want_filter:
            g_out = torch.empty((batch, n_freq, d, channels), dtype=torch.complex128, device=device)
    _lib.call_op("specinv_wpe", (s4, pw, g_in, out, g_out, lam, scratch, batch, channels, n_freq, n_frames, taps, delay, n_iter, ctx,
                                 eps, diag_load), spec.dtype != torch.complex64, device)
    back = lambda t, shape: t.reshape(shape).to(device=spec.device)       # noqa: E731
    return (back(out, spec.shape), back(g_out, g_shape) if want_filter else None,
            back(lam, lead + (n_freq, n_frames)) if want_power else None)


def wpe(spec, taps=10, delay=3, n_iter=3, psd_context=0, eps=1e-10, diag_load=1e-10, power=None, return_filter=False,
        return_power=False):
    r"""A reverberant complex spectrogram dereverberated: `Y`, of `spec`'s shape, dtype (complex64 or complex128) and device.  The
    definition is the module's.

    `spec` is (F, T) for one channel, (C, F, T) for the C channels of ONE recording - the leading axis of a 3-D input is channels,
    not a batch - or (B, C, F, T) for a batch; a batch of single-channel recordings is (B, 1, F, T).  The channels of an item are
    filtered jointly, items independently: item b of a batch gives the bits it gives alone.

    `taps` (K >= 1) lags per channel starting `delay` (>= 1) frames back; `n_iter` (>= 0) re-estimations of the power;
    `psd_context` (>= 0) frames either side over which the power is averaged; `eps` floors the power at `eps` times its maximum
    over the bin's frames; `diag_load` adds that fraction of R's mean diagonal to it.  `power`, real, non-negative and
    broadcastable to (..., F, T) - `spec`'s shape without the channel axis - replaces |X|^2 in the first iteration: a PSD from
    `spectral_gain`, or a network's ("DNN-WPE"); `psd_context` averages it as well.

    `return_filter=True` adds `G`, complex128 (..., F, C, taps, C): `G[f, c', k, c]` is the weight of channel c' at lag delay + k
    in the prediction of channel c.  `return_power=True` adds the last `lam`, float64 (..., F, T).  The result is `Y` or the tuple
    `(Y[, G][, lam])`.

    Limits: C x taps <= 64, psd_context <= 64, n_iter <= 100 (the launch's length is bounded); any F, T, B.  Not differentiable.  No half precision, no sharded form, no `frame_major` form.  Any
    layout torch can express is read as torch would read it.  A CPU tensor is computed on the current HIP device and comes back.
    """
    lead, channels, n_freq, n_frames = _checked_spec(spec, "wpe")
    taps, delay, n_iter, ctx, eps, diag_load = _checked_params(taps, delay, n_iter, psd_context, eps, diag_load)
    _checked_unknowns(channels, taps)
    if power is not None:
        if not isinstance(power, torch.Tensor):
            raise TypeError("power must be a torch.Tensor")
        if power.dtype not in _REAL:
            raise TypeError(f"power must be real (float16 / bfloat16 / float32 / float64), got dtype {power.dtype}")
        want = lead + (n_freq, n_frames)
        if not broadcasts_to(power.shape, want):
            raise ValueError(f"power of shape {tuple(power.shape)} does not broadcast to {want}, spec's shape without the channel axis")
        if torch.is_grad_enabled() and power.requires_grad:
            raise NotImplementedError("wpe is not differentiable; detach the inputs")
    y, g, lam = _launch(spec, lead, channels, n_freq, n_frames, taps, delay, n_iter, ctx, eps, diag_load, power, None, return_filter,
                        return_power)
    res = (y,) + ((g,) if return_filter else ()) + ((lam,) if return_power else ())
    return res[0] if len(res) == 1 else res


def wpe_apply(spec, filt, delay):
    r"""`spec - G^H xs` for a given filter: `spec` as in `wpe`, `filt` the `G` of a `wpe(..., return_filter=True)` call - complex,
    (..., F, C, taps, C) - and `delay` that call's.  Estimate on one block and apply to another, or inspect a filter.  It is
    `wpe`'s launch in a filter-only mode: with the `G` and `spec` of one `wpe` call the result equals that call's `Y` bit for bit.
    Limits as `wpe`."""
    lead, channels, n_freq, n_frames = _checked_spec(spec, "wpe_apply")
    delay = _checked_delay(delay)
    if not isinstance(filt, torch.Tensor):
        raise TypeError("filt must be a torch.Tensor")
    if filt.dtype not in _CPLX:
        raise TypeError(f"filt must be complex64 or complex128, got dtype {filt.dtype}")
    if filt.dim() != len(lead) + 4 or tuple(filt.shape[:-2]) != lead + (n_freq, channels) or filt.shape[-1] != channels \
            or filt.shape[-2] < 1:
        raise ValueError(f"filt must be of shape {lead + (n_freq, channels, 'taps', channels)}, got {tuple(filt.shape)}")
    if torch.is_grad_enabled() and filt.requires_grad:
        raise NotImplementedError("wpe_apply is not differentiable; detach the inputs")
    taps = filt.shape[-2]
    _checked_unknowns(channels, taps)
    return _launch(spec, lead, channels, n_freq, n_frames, taps, delay, 0, 0, 0.0, 0.0, None, filt, False, False)[0]


def dereverb(x, n_fft=None, taps=10, delay=3, n_iter=3, psd_context=0, eps=1e-10, diag_load=1e-10, **stft_kwargs):
    r"""A reverberant waveform (L,), (C, L) - the channels of one recording - or (B, C, L) dereverberated: a waveform of that shape.
    With the leading axes flattened for the transforms it is exactly

        istft(wpe(stft(x, n_fft, **stft_kwargs), taps, delay, n_iter, psd_context, eps, diag_load), **stft_kwargs)

    the composition of the public calls, bit for bit.  The options are `wpe`'s, `**stft_kwargs` are `stft`'s (`hop_length`,
    `window`, ...; `n_fft` defaults as there).  float16 / bfloat16 audio is transformed as `stft` transforms it (in float32).  Not
    differentiable.
    """
    from .projection import istft, stft
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    if x.dim() not in (1, 2, 3):
        raise ValueError(f"x must be (L,), (C, L) - the channels of one recording - or (B, C, L), got shape {tuple(x.shape)}")
    taps, delay, n_iter, ctx, eps, diag_load = _checked_params(taps, delay, n_iter, psd_context, eps, diag_load)
    _checked_unknowns(x.shape[-2] if x.dim() >= 2 else 1, taps)
    if torch.is_grad_enabled() and x.requires_grad:
        raise NotImplementedError("dereverb is not differentiable; detach the input")
    kw = {k: v for k, v in stft_kwargs.items() if k in _RECOGNISED}
    X = stft(x.reshape(-1, x.shape[-1]), n_fft, **kw)
    Y = wpe(X.reshape(tuple(x.shape[:-1]) + tuple(X.shape[-2:])) if x.dim() >= 2 else X[0], taps, delay, n_iter, ctx, eps, diag_load)
    y = istft(Y.reshape((-1,) + tuple(Y.shape[-2:])), **kw)
    return y.reshape(tuple(x.shape[:-1]) + (y.shape[-1],))
