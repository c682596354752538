"""`gla_projection`, `stft` and `istft` restated in torch, so that autograd differentiates them on the CPU, and the adjoint
recursion of csrc/kernels_proj_adjoint.h written out in torch ops without autograd.  A helper of the projection tests, not a test
file.

    P(x; m) = istft(S m / (|S| + 1e-16)) ,  S = stft(x)

The transforms are tests/_misi_torch.py's: `torch.stft`; the inverse real / complex transform of every frame, times the window,
overlap-added, divided by the window-square envelope.  All arithmetic in the dtype of `x`."""
import functools

import numpy as np
import torch

import _misi_torch as mt
from _util import hann
from oracle.stftlib import signal_length


def setup(n_freq, dtype, n_frames, stft_kwargs):
    """(StftArgs, window, envelope, L)"""
    a, w = mt._setup(n_freq, dtype, stft_kwargs)
    return a, w, mt.envelope(n_frames, a, w), signal_length(n_frames, a)


def stft(x, n_freq, **stft_kwargs):
    """(B, L) real -> (B, F, T) complex"""
    a, w = mt._setup(n_freq, x.dtype, stft_kwargs)
    return mt.stft(x, a, w)


def istft(spec, **stft_kwargs):
    """(B, F, T) complex -> (B, L)"""
    a, w, env, _ = setup(spec.shape[1], spec.real.dtype, spec.shape[2], stft_kwargs)
    return mt.istft(spec, a, w, env)


def project(x, mag, **stft_kwargs):
    """x (B, L), mag (B, F, T) real CPU tensors of one precision -> (B, L); differentiable with respect to both"""
    a, w, env, L = setup(mag.shape[1], x.dtype, mag.shape[2], stft_kwargs)
    assert x.shape[1] == L, (x.shape, L)
    S = mt.stft(x, a, w)
    return mt.istft(S * mag / (S.abs() + 1e-16), a, w, env)


def _pad_sources(L, a):
    """index of the signal sample every padded position reads (-1: a zero of constant padding)"""
    idx = np.arange(L)
    if not a.padding:
        return idx
    mode = {"reflect": "reflect", "replicate": "edge", "circular": "wrap"}.get(a.pad_mode)
    if mode is None:
        return np.pad(idx, a.padding, mode="constant", constant_values=-1)
    return np.pad(idx, a.padding, mode=mode)


def project_adjoint(x, mag, g_y, **stft_kwargs):
    """The recursion of csrc/kernels_proj_adjoint.h in torch ops, no autograd: (g_x, g_mag) for the cotangent g_y of P(x; mag).
        u = g_y / env ;  Y = unscaled windowed DFT of the zero-padded frames of u ;  R = stft(x)
        gQ = inv_scale (interior ? 2 Y : Re Y)  (two-sided: inv_scale Y) ;  d = |R| + 1e-16 ;  dot = Re(conj(gQ) R)
        gm = dot / d ;  gR = gQ m / d - R (|R| > 0 ? dot m / (d^2 |R|) : 0) ;  interior bins halved
        g_x = fold(overlap-add(w fwd_scale sum_k gR_k e^{+}))"""
    with torch.no_grad():
        B, F, T = mag.shape
        a, w, env, L = setup(F, x.dtype, T, stft_kwargs)
        N, hop, pad = a.n_fft, a.hop_length, a.padding
        fwd = N ** -0.5 if a.normalized else 1.0
        inv = N ** -0.5 if a.normalized else 1.0 / N
        u = torch.nn.functional.pad(g_y / env, (pad, pad))
        Y = torch.stft(u, N, hop_length=hop, win_length=N, window=w, center=False, normalized=False, onesided=a.onesided,
                       return_complex=True)
        R = mt.stft(x, a, w)
        if a.onesided:
            interior = torch.ones(F, dtype=torch.bool)
            interior[0] = interior[N // 2] = False
            interior = interior[None, :, None]
            gQ = torch.where(interior, 2 * inv * Y, torch.complex(inv * Y.real, torch.zeros_like(Y.real)))
        else:
            gQ = inv * Y
        r = R.abs()
        d = r + 1e-16
        dot = gQ.real * R.real + gQ.imag * R.imag
        gm = dot / d
        c2 = torch.where(r > 0, dot * mag / (d * d * torch.where(r > 0, r, torch.ones_like(r))), torch.zeros_like(r))
        gR = gQ * (mag / d) - R * c2
        if a.onesided:
            gR = torch.where(interior, 0.5 * gR, gR)
            fr = torch.fft.irfft(gR.transpose(1, 2), n=N, dim=-1) * N
        else:
            fr = torch.fft.ifft(gR.transpose(1, 2), n=N, dim=-1).real * N
        full = mt._overlap_add(fr * (w * fwd), hop, 0)              # over the padded signal
        src = torch.from_numpy(_pad_sources(L, a))
        keep = src >= 0
        g_x = torch.zeros((B, L), dtype=x.dtype).index_add_(1, src[keep], full[:, keep])
        return g_x, gm


def hamming(n, dtype):
    return (0.54 - 0.46 * np.cos(2 * np.pi * np.arange(n) / n)).astype(dtype)


# ---- the cases of tests/test_gpu_projection.py ---------------------------------------------------------------------------------
# name: n_fft, hop, frames, window length, extra stft kwargs; B = 2.  (center=False: a Hamming window - a Hann window's first
# sample is 0 and so is the envelope's there)
CONFIGS = {
    "128/32": (128, 32, 9, 128, {}),                                 # several frames per wave, the last group partly filled
    "256/100/200": (256, 100, 7, 200, dict(win_length=200)),
    "512/128": (512, 128, 10, 512, {}),                              # float64: four points per lane
    "1024/256": (1024, 256, 12, 1024, {}),                           # one frame per wave
    "1024/256 center=False": (1024, 256, 12, 1024, dict(center=False)),
    "2048/512 normalized": (2048, 512, 9, 2048, dict(normalized=True)),
    "2048/512": (2048, 512, 9, 2048, {}),                            # float64: a frame on a team of two waves
    "512/128 constant": (512, 128, 10, 512, dict(pad_mode="constant")),
    "400/160": (400, 160, 8, 400, {}),                               # staged
    "64/16 two-sided normalized": (64, 16, 11, 64, dict(onesided=False, normalized=True)),   # staged
}
FUSED = [("128/32", np.float32), ("128/32", np.float64), ("256/100/200", np.float32), ("256/100/200", np.float64),
         ("512/128", np.float32), ("512/128", np.float64), ("1024/256", np.float32), ("1024/256 center=False", np.float64),
         ("2048/512 normalized", np.float32), ("2048/512", np.float64), ("512/128 constant", np.float32)]
STAGED = [(n, d) for n in ("400/160", "64/16 two-sided normalized") for d in (np.float32, np.float64)]


def stft_kwargs(name, dtype):
    n_fft, hop, frames, wl, extra = CONFIGS[name]
    win = hamming(wl, dtype) if extra.get("center") is False else hann(wl, dtype)
    return dict(hop_length=hop, window=win, **extra)


# The float32 cases that compare two float32 implementations at 2e-5 (the fused kernel against the staged path) need inputs whose own
# float32 noise is below that: a bin of R = STFT(x) that passes close to zero enters the gradient with 1 / |R|^2, and a case with such a
# bin measures its conditioning, not the kernels.  The measure needs no device - the restatement's own float32-against-float64
# gradient error, the larger of x's and mag's - and the seed of a case is the first from 0 at which it is at most 1e-5
# (tests/test_projection_host.py asserts it).  2048/512 normalized, 18 450 bins, has no such seed among the first 120 (median 2.4e-4):
# it takes the best of them, 1.9e-5.  Every other case keeps n_fft + hop + frames.
SEEDS = {("128/32", None): 1, ("256/100/200", None): 2, ("512/128", None): 1, ("1024/256", None): 0, ("512/128 constant", None): 0,
         ("2048/512 normalized", None): 12}


def draw(name, dtype, batch, frames, seed):
    """(x, mag, w, kw) as NumPy arrays: x standard normal (B, L), mag = |STFT(another normal signal)| (0.5 + U(0, 1)) (B, F, T), w
    the fixed random weights of the loss sum(w * y)"""
    n_fft, hop, T, wl, extra = CONFIGS[name]
    T = frames or T
    kw = stft_kwargs(name, dtype)
    F = n_fft // 2 + 1 if extra.get("onesided", True) else n_fft
    a, _ = mt._setup(F, torch.float64, kw)
    L = signal_length(T, a)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((batch, L))
    other = torch.from_numpy(rng.standard_normal((batch, L)))
    mag = stft(other, F, **dict(kw, window=kw["window"].astype(np.float64))).abs().numpy() * (0.5 + rng.random((batch, F, T)))
    w = np.random.default_rng(7).standard_normal((batch, L))
    return x.astype(dtype), mag.astype(dtype), w.astype(dtype), kw


@functools.lru_cache(maxsize=None)
def inputs(name, dtype, batch=2, frames=None):
    n_fft, hop, T, _, _ = CONFIGS[name]
    return draw(name, dtype, batch, frames, SEEDS.get((name, frames), n_fft + hop + (frames or T)))


def grads(x, mag, w, kw, compute):
    """Autograd on the restatement in `compute`: (y, grad x, grad mag) as NumPy arrays"""
    wide = lambda v: v.astype(np.result_type(v.dtype, compute))                # noqa: E731
    xt, mt_ = torch.from_numpy(wide(x)).requires_grad_(True), torch.from_numpy(wide(mag)).requires_grad_(True)
    y = project(xt, mt_, **dict(kw, window=wide(kw["window"])))
    (y * torch.from_numpy(wide(w))).sum().backward()
    return y.detach().numpy(), xt.grad.numpy(), mt_.grad.numpy()


@functools.lru_cache(maxsize=None)
def reference(name, dtype, compute=None, batch=2, frames=None):
    """Autograd on the restatement, on the CPU, the inputs of `dtype` computed in `compute` (default: `dtype`): (y, grad x, grad
    mag) as NumPy arrays; computed once per case."""
    return grads(*inputs(name, dtype, batch, frames), compute or dtype)
