"""`noise_psd`, `spectral_gain` and `denoise`: single-channel speech enhancement in one launch.  `consistent_wiener`
and `misi` start from variances the caller must already have; this is the classical front end that estimates them from one noisy
recording: the noise-power tracker of Gerkmann & Hendriks ("Unbiased MMSE-based noise power estimation with low complexity and
low tracking delay", IEEE TASLP 2012: speech presence probability with a fixed prior), the decision-directed a-priori SNR and the
Wiener or log-spectral-amplitude (LSA) gain of Ephraim & Malah (IEEE TASSP 1984 / 1985).  `xi * sigma2` and `sigma2` are exactly
`consistent_wiener`'s `var_target` and `var_noise`.

Definition (tests/_enhance_oracle.py is its float64 statement).  Per item and bin, frames l = 0 ... T - 1:

    P_l = |X_l|^2, or m_l^2 for real magnitudes.  All state and arithmetic are float64 whatever the input dtype.
    tiny = 1e-300.  xi1 = 10^(prior_snr_db / 10).

Tracker.  Start, when no `state` is given: sigma2_{-1} is the mean of P_l over the first min(init_frames, T) frames, Pbar_{-1} = 0.

    g'     = P_l / max(sigma2_{l-1}, tiny)
    p      = 1 / (1 + (1 + xi1) exp(-g' xi1 / (1 + xi1)))
    Pbar_l = a_spp Pbar_{l-1} + (1 - a_spp) p
    if Pbar_l > 0.99:  p = min(p, 0.99)
    sigma2_l = a_pow sigma2_{l-1} + (1 - a_pow) ((1 - p) P_l + p sigma2_{l-1})

When `noise` is given, the tracker is bypassed and sigma2_l is that tensor, broadcast: a full array, an (F, 1) profile or a scalar.

Gain.

    g    = P_l / max(sigma2_l, tiny)
    xi_l = max(alpha A2_{l-1} / max(sigma2_l, tiny) + (1 - alpha) max(g - 1, 0), xi_min)
    w    = xi_l / (1 + xi_l)
    "wiener": G = w
    "lsa":    G = w exp(E1(max(w g, 1e-12)) / 2)
    G_l  = min(max(G, g_min), 1)
    A2_l = G_l^2 P_l

Without a `state` the first term at l = 0 is alpha.  xi_min = 10^(xi_min_db / 10), g_min = 10^(gain_floor_db / 20).  The cap at 1
is needed: without it the LSA rule gives gains above 10^3 on near-empty bins.  E1 is the exponential integral; the device
evaluates it to a relative error below 1e-13 on [1e-12, 700] (the series up to 1, Chebyshev sums in 1 / v above) and as 0 beyond.
The three quotients by max(sigma2, tiny) are capped at 1e300, so that nothing overflows and nothing is ever NaN.

State.  `state` is a float64 tensor (..., F, 3) holding sigma2, Pbar, A2.  Passing it skips the start rules; `return_state=True`
returns the last frame's values.  One call on T frames and two calls on [0, T1) and [T1, T) chained through the state give the same
bits: the streaming form (the first chunk holds at least min(init_frames, T) frames, which the start rule reads and takes for
noise alone).

The defaults are the papers' values (alpha_pow 0.8, alpha_spp 0.9, a 15 dB prior, alpha 0.98, xi_min -25 dB) and a -20 dB gain
floor; they are not tuned on anything.

Not part of the reference's surface.
"""
from __future__ import annotations

import math

import torch

from . import _lib
from ._ingest import broadcasts_to, ingest, is_int, is_real
from .plan import _RECOGNISED, require_gpu

__all__ = ["noise_psd", "spectral_gain", "denoise"]

_TILE_FRAMES = 32              # frames of a tile of the (B, F, T) walk (csrc/kernels_enhance.h: kEnhTile)
# dtype -> (the dtype computed in, the real dtype returned, complex?)
_KINDS = {torch.float16: (torch.float32, torch.float16, False), torch.bfloat16: (torch.float32, torch.bfloat16, False),
          torch.float32: (torch.float32, torch.float32, False), torch.float64: (torch.float64, torch.float64, False),
          torch.complex32: (torch.float32, torch.float16, True), torch.complex64: (torch.float32, torch.float32, True),
          torch.complex128: (torch.float64, torch.float64, True)}
_REAL = (torch.float16, torch.bfloat16, torch.float32, torch.float64)


def _unit(v, name):
    if not is_real(v) or not 0 <= v <= 1:
        raise ValueError(f"{name} must be a number in 0 ... 1, got {v!r}")
    return float(v)


def _checked_tracker(init_frames, alpha_pow, alpha_spp, prior_snr_db):
    if not is_int(init_frames) or not 1 <= init_frames < 1 << 31:
        raise ValueError(f"init_frames must be an int >= 1, got {init_frames!r}")
    if not is_real(prior_snr_db) or not -3000 <= prior_snr_db <= 3000:
        raise ValueError(f"prior_snr_db must be a number in -3000 ... 3000, got {prior_snr_db!r}")
    return init_frames, _unit(alpha_pow, "alpha_pow"), _unit(alpha_spp, "alpha_spp"), 10.0 ** (prior_snr_db / 10.0)


def _checked_gain(rule, alpha, xi_min_db, gain_floor_db):
    if rule not in _lib.ENHANCE_RULES:
        raise ValueError(f"rule must be 'wiener' or 'lsa', got {rule!r}")
    if not is_real(xi_min_db) or not -3000 <= xi_min_db <= 3000:
        raise ValueError(f"xi_min_db must be a number in -3000 ... 3000, got {xi_min_db!r}")
    if not is_real(gain_floor_db) or not -6000 <= gain_floor_db <= 0:
        raise ValueError(f"gain_floor_db must be a number in -6000 ... 0, got {gain_floor_db!r}")
    return _lib.ENHANCE_RULES[rule], _unit(alpha, "alpha"), 10.0 ** (xi_min_db / 10.0), 10.0 ** (gain_floor_db / 20.0)


def _checked_spec(spec, frame_major, what):
    if not isinstance(spec, torch.Tensor):
        raise TypeError("spec must be a torch.Tensor")
    if spec.dtype not in _KINDS:
        raise TypeError(f"spec must be real or complex floating point, got dtype {spec.dtype}")
    if spec.dim() not in (2, 3):
        raise ValueError(f"spec must be (F, T) or (B, F, T) - (T, F) or (B, T, F) with frame_major=True - got shape {tuple(spec.shape)}")
    if spec.shape[-1] < 1 or spec.shape[-2] < 1:
        raise ValueError(f"spec of shape {tuple(spec.shape)} holds no bins or no frames")
    if torch.is_grad_enabled() and spec.requires_grad:
        raise NotImplementedError(f"{what} is not differentiable; detach the input")
    return (spec.shape[-1], spec.shape[-2]) if frame_major else (spec.shape[-2], spec.shape[-1])


def _checked_state(state, spec, n_freq, what):
    if not isinstance(state, torch.Tensor):
        raise TypeError("state must be a torch.Tensor")
    if state.dtype != torch.float64:
        raise TypeError(f"state must be float64, got dtype {state.dtype}")
    want = tuple(spec.shape[:-2]) + (n_freq, 3)
    if tuple(state.shape) != want:
        raise ValueError(f"state must be of shape {want}, got {tuple(state.shape)}")
    if torch.is_grad_enabled() and state.requires_grad:
        raise NotImplementedError(f"{what} is not differentiable; detach the inputs")


def _checked_noise(noise, spec, what):
    if not isinstance(noise, torch.Tensor):
        raise TypeError("noise must be a torch.Tensor")
    if noise.dtype not in _REAL:
        raise TypeError(f"noise must be real (float16 / bfloat16 / float32 / float64), got dtype {noise.dtype}")
    if not broadcasts_to(noise.shape, spec.shape):
        raise ValueError(f"noise of shape {tuple(noise.shape)} does not broadcast to spec's {tuple(spec.shape)}")
    if torch.is_grad_enabled() and noise.requires_grad:
        raise NotImplementedError(f"{what} is not differentiable; detach the inputs")


def _run(spec, n_freq, n_frames, frame_major, noise, state, rule, tracker, gain, want):
    """One launch.  `want`: the names of the outputs among noise, spp, gain, snr, enhanced, state.  Returns a dict of tensors of
    spec's shape (state: (..., F, 3)) on spec's device, the real ones in spec's real dtype."""
    cdt, out_dtype, cplx = _KINDS[spec.dtype]
    init_frames, a_pow, a_spp, xi1 = tracker
    alpha, xi_min, g_min = gain
    lead = tuple(spec.shape[:-2])
    if spec.numel() == 0:
        res = {k: spec.new_zeros(spec.shape, dtype=spec.dtype if k == "enhanced" else out_dtype) for k in want if k != "state"}
        if "state" in want:
            res["state"] = spec.new_zeros(lead + (n_freq, 3), dtype=torch.float64)
        return res
    device = require_gpu(spec.device)
    shape3 = (-1,) + tuple(spec.shape[-2:])
    in_dtype = (torch.complex64 if cdt == torch.float32 else torch.complex128) if cplx else cdt
    s3 = ingest(spec.reshape(shape3), device, in_dtype)
    batch = s3.shape[0]
    mode, nz = _lib.ENHANCE_TRACK, None
    if noise is not None:
        full = noise.expand(spec.shape)
        t_dim = -2 if frame_major else -1
        if full.stride(t_dim) == 0 or n_frames == 1:           # one value per chain: an (F, 1) profile, a scalar
            mode, nz = _lib.ENHANCE_NOISE_PROFILE, ingest(full.select(t_dim, 0).reshape(batch, n_freq), device, cdt)
        else:
            mode, nz = _lib.ENHANCE_NOISE_FULL, ingest(full.reshape(shape3), device, cdt)
    st_in = None if state is None else ingest(state.reshape(batch, n_freq, 3), device, torch.float64)
    outs = {}
    for k in want:
        if k == "state":
            outs[k] = torch.empty((batch, n_freq, 3), dtype=torch.float64, device=device)
        elif k == "noise" and noise is not None:
            continue                                               # (the tracker does not run: it is the input, below)
        else:
            outs[k] = torch.empty(s3.shape, dtype=in_dtype if k == "enhanced" else cdt, device=device)
    _lib.call_op("specinv_enhance", (s3, nz, st_in, outs.get("noise"), outs.get("spp"), outs.get("gain"), outs.get("snr"),
                                     outs.get("enhanced"), outs.get("state"), batch, n_freq, n_frames, init_frames, mode, rule, a_pow,
                                     a_spp, xi1, alpha, xi_min, g_min, int(cplx), int(bool(frame_major))), cdt != torch.float32, device)
    res = {}
    for k in want:
        if k == "state":
            res[k] = outs[k].reshape(lead + (n_freq, 3)).to(device=spec.device)
        elif k == "noise" and noise is not None:
            res[k] = noise.detach().expand(spec.shape).to(device=spec.device, dtype=out_dtype).contiguous()
        else:
            res[k] = outs[k].reshape(spec.shape).to(device=spec.device, dtype=spec.dtype if k == "enhanced" else out_dtype)
    return res


def noise_psd(spec, init_frames=5, alpha_pow=0.8, alpha_spp=0.9, prior_snr_db=15.0, state=None, return_spp=False,
              return_state=False, frame_major=False):
    r"""The noise power `sigma2` of a spectrogram (F, T) / (B, F, T), complex or real magnitudes: a real array of its shape, real
    dtype and device, tracked along the frames of every bin.  The definition is the module's tracker.

    `init_frames` (an int >= 1) frames give the start; `alpha_pow` and `alpha_spp` (in 0 ... 1) smooth the power and the speech
    presence probability; `prior_snr_db` is the a-priori SNR the presence test assumes.  The defaults are the paper's values, not
    tuned ones.  `state` (float64, (..., F, 3): sigma2, Pbar, A2) continues an earlier call and `return_state=True` adds the last
    frame's state; `return_spp=True` adds `p`, the presence probability of the update.  The result is `sigma2`, or the tuple
    `(sigma2[, spp][, state])`.  With `frame_major=True` the arrays are (T, F) / (B, T, F); the state stays (..., F, 3).

    Any F >= 1 and T >= 1, any number of items.  float16 / bfloat16 / complex32 are computed as float32 and rounded back; the
    state and all arithmetic are float64.  Any layout torch can express is read as torch would read it.  A CPU tensor is computed
    on the current HIP device and comes back to the CPU.  Not differentiable.
    """
    n_freq, n_frames = _checked_spec(spec, frame_major, "noise_psd")
    tracker = _checked_tracker(init_frames, alpha_pow, alpha_spp, prior_snr_db)
    if state is not None:
        _checked_state(state, spec, n_freq, "noise_psd")
    want = ["noise"] + (["spp"] if return_spp else []) + (["state"] if return_state else [])
    res = _run(spec, n_freq, n_frames, frame_major, None, state, _lib.ENHANCE_RULES["wiener"], tracker, (0.98, 1.0, 1.0), want)
    return res["noise"] if len(want) == 1 else tuple(res[k] for k in want)


def spectral_gain(spec, noise=None, rule="lsa", alpha=0.98, xi_min_db=-25.0, gain_floor_db=-20.0, init_frames=5, alpha_pow=0.8,
                  alpha_spp=0.9, prior_snr_db=15.0, state=None, return_snr=False, return_noise=False, return_enhanced=False,
                  return_state=False, frame_major=False):
    r"""The enhancement gain `G` of a spectrogram (F, T) / (B, F, T), complex or real magnitudes: a real array of its shape, real
    dtype and device with `g_min <= G <= 1`.  The definition is the module's: the tracker (or `noise`, real and broadcastable to
    `spec`, which bypasses it and makes its four parameters irrelevant), the decision-directed a-priori SNR with weight `alpha`
    (in 0 ... 1) and floor `xi_min_db`, and the gain rule `rule`, "wiener" or "lsa", floored at `gain_floor_db` (<= 0).  The
    defaults are the papers' values, not tuned ones.

    The extras come from the same launch, in this order after `G`: `return_snr` adds `xi`, `return_noise` adds `sigma2`,
    `return_enhanced` adds `G * spec` (of `spec`'s dtype, each part rounded once from the float64 product), `return_state` adds
    the last frame's state.  `xi * sigma2` and `sigma2` are `consistent_wiener`'s `var_target` and `var_noise`.  `state`,
    `frame_major`, dtypes, layouts, devices and limits are `noise_psd`'s; `noise` is read in `spec`'s real dtype.
    """
    n_freq, n_frames = _checked_spec(spec, frame_major, "spectral_gain")
    if noise is not None:
        _checked_noise(noise, spec, "spectral_gain")
    rule_id, alpha, xi_min, g_min = _checked_gain(rule, alpha, xi_min_db, gain_floor_db)
    tracker = _checked_tracker(init_frames, alpha_pow, alpha_spp, prior_snr_db)
    if state is not None:
        _checked_state(state, spec, n_freq, "spectral_gain")
    want = ["gain"] + [k for k, on in (("snr", return_snr), ("noise", return_noise), ("enhanced", return_enhanced),
                                       ("state", return_state)) if on]
    res = _run(spec, n_freq, n_frames, frame_major, noise, state, rule_id, tracker, (alpha, xi_min, g_min), want)
    return res["gain"] if len(want) == 1 else tuple(res[k] for k in want)


def denoise(x, n_fft=None, rule="lsa", consistent=False, gamma=1.0, n_iter=30, alpha=0.98, xi_min_db=-25.0, gain_floor_db=-20.0,
            init_frames=5, alpha_pow=0.8, alpha_spp=0.9, prior_snr_db=15.0, **stft_kwargs):
    r"""A noisy waveform (L,) / (B, L) enhanced: a waveform.  With `X = stft(x, n_fft, **stft_kwargs)` and
    `G, xi, sigma2 = spectral_gain(X, rule=rule, ..., return_snr=True, return_noise=True)` it is exactly

        istft(G * X, **stft_kwargs)                                                                        consistent=False
        istft(consistent_wiener(X, xi * sigma2, sigma2, gamma=gamma, n_iter=n_iter, **stft_kwargs)[0], **stft_kwargs)    consistent=True

    the composition of the public calls, bit for bit.  `consistent=True` asks the filtered spectrogram to be the STFT of a signal
    (`consistent_wiener`, whose limits then apply: a one-sided STFT, at most 65535 items).  The tracker's and the gain's options
    are `spectral_gain`'s, `**stft_kwargs` are `stft`'s (`hop_length`, `window`, ...; `n_fft` defaults as there).  Not
    differentiable.
    """
    from .projection import istft, stft
    from .wiener import consistent_wiener
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    _checked_gain(rule, alpha, xi_min_db, gain_floor_db)
    _checked_tracker(init_frames, alpha_pow, alpha_spp, prior_snr_db)
    if not is_real(gamma) or not (gamma > 0 and math.isfinite(gamma)):
        raise ValueError(f"gamma must be a finite number > 0, got {gamma!r}")
    if not is_int(n_iter) or n_iter < 0:
        raise ValueError(f"n_iter must be an int >= 0, got {n_iter!r}")
    if torch.is_grad_enabled() and x.requires_grad:
        raise NotImplementedError("denoise is not differentiable; detach the input")
    kw = {k: v for k, v in stft_kwargs.items() if k in _RECOGNISED}
    X = stft(x, n_fft, **kw)
    opts = dict(rule=rule, alpha=alpha, xi_min_db=xi_min_db, gain_floor_db=gain_floor_db, init_frames=init_frames,
                alpha_pow=alpha_pow, alpha_spp=alpha_spp, prior_snr_db=prior_snr_db)
    if not consistent:
        return istft(spectral_gain(X, **opts) * X, **kw)
    G, xi, sigma2 = spectral_gain(X, return_snr=True, return_noise=True, **opts)
    return istft(consistent_wiener(X, xi * sigma2, sigma2, gamma=gamma, n_iter=n_iter, **kw)[0], **kw)
