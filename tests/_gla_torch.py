"""`griffin_lim` and `ADMM` restated in torch on the transforms of tests/_misi_torch.py and the `phase_init` of tests/_agla_torch.py,
so that autograd differentiates them on the CPU: the reference of the spectrogram gradients at real frame sizes, and of the
element-wise steps `gla_update` / `admm_update` on their own.  A helper of the gradient tests, not a test file.

    C0 = spec (complex)  or  phase_init(spec) ;  m = |spec|  or  spec ;  x = istft(C0)
    griffin_lim:  P = C0 ; repeat:  S = stft(x) - lr P ;  P = S ;  x = istft(S m / (|S| + 1e-16)) ,  lr = alpha / (1 + alpha)
    ADMM:  X = Y = C0, U = 0 ; repeat:  Z = (rho Y + stft(x)) / (1 + rho) ;  U = U + X - Z ;  V = Z - U ;
           X = V m / (|V| + 1e-16) ;  Y = X + U ;  x = istft(Y)

All arithmetic in the real dtype of `spec`.  Two measures of a case's conditioning come with it, both CPU-only:
`noise32`, the restatement's float32 gradient against its float64 gradient on the same float32 inputs, and `sens64`, the relative
change of its float64 gradient when every input element is multiplied by 1 +- 2^-52 with random signs."""
import functools

import numpy as np
import torch

import _misi_torch as mt
from _agla_torch import phase_init
from _proj_torch import hamming
from _util import hann, rel_l2
from oracle.stftlib import signal_length


def _start(spec, stft_kwargs):
    rdt = spec.real.dtype if spec.is_complex() else spec.dtype
    a, w = mt._setup(spec.shape[1], rdt, stft_kwargs)
    env = mt.envelope(spec.shape[2], a, w)
    C, m = (spec, spec.abs()) if spec.is_complex() else (phase_init(spec, a), spec)
    return a, w, env, C, m


def gla_update(R, P, m, lr):
    """-> (S, Q)"""
    S = R - P * lr
    return S, S * m / (S.abs() + 1e-16)


def admm_update(R, X, U, m, rho):
    """-> (X', U', V, Y')"""
    Z = (rho * (X + U) + R) / (1 + rho)
    Un = U + X - Z
    V = Z - Un
    Xn = V * m / (V.abs() + 1e-16)
    return Xn, Un, V, Xn + Un


def gla(spec, n_iter, alpha, **stft_kwargs):
    """spec (B, F, T) complex or real CPU tensor -> (B, L); differentiable with respect to `spec`"""
    a, w, env, C, m = _start(spec, stft_kwargs)
    lr = alpha / (1 + alpha)
    P, x = C, mt.istft(C, a, w, env)
    for _ in range(n_iter):
        P, Q = gla_update(mt.stft(x, a, w), P, m, lr)
        x = mt.istft(Q, a, w, env)
    return x


def admm(spec, n_iter, rho, **stft_kwargs):
    a, w, env, C, m = _start(spec, stft_kwargs)
    X, U, x = C, torch.zeros_like(C), mt.istft(C, a, w, env)
    for _ in range(n_iter):
        X, U, _, Y = admm_update(mt.stft(x, a, w), X, U, m, rho)
        x = mt.istft(Y, a, w, env)
    return x


METHODS = {"gla": gla, "admm": admm}


def wide(v, compute):
    return v.astype(np.result_type(v.dtype, compute)) if isinstance(v, np.ndarray) else v


def grads(method, spec, w, n_iter, coef, kw, compute=None):
    """Autograd on the restatement of `method`, the inputs computed in `compute` (default: their own precision), loss sum(w y):
    (y, grad spec) as NumPy arrays"""
    compute = compute or w.dtype
    s = torch.from_numpy(wide(spec, compute)).requires_grad_(True)
    y = METHODS[method](s, n_iter, coef, **{k: wide(v, compute) for k, v in kw.items()})
    (y * torch.from_numpy(wide(w, compute))).sum().backward()
    return y.detach().numpy(), s.grad.numpy()


def noise32_of(method, spec, w, n_iter, coef, kw):
    """float32 inputs: the restatement's float32 gradient against its float64 gradient"""
    assert w.dtype == np.float32
    return rel_l2(grads(method, spec, w, n_iter, coef, kw)[1], grads(method, spec, w, n_iter, coef, kw, np.float64)[1])


def ulp_perturbed(v, rng):
    """every element (a complex one: both parts) times 1 +- 2^-52"""
    f = lambda shape: 1.0 + np.where(rng.random(shape) < 0.5, -1.0, 1.0) * 2.0 ** -52                 # noqa: E731
    return v.real * f(v.shape) + 1j * (v.imag * f(v.shape)) if np.iscomplexobj(v) else v * f(v.shape)


def sens64_of(method, spec, w, n_iter, coef, kw, seed=52):
    spec, w = wide(spec, np.float64), wide(w, np.float64)
    g0 = grads(method, spec, w, n_iter, coef, kw, np.float64)[1]
    g1 = grads(method, ulp_perturbed(spec, np.random.default_rng(seed)), w, n_iter, coef, kw, np.float64)[1]
    return rel_l2(g1, g0)


def wellcond(batch, length, seed):
    """The signal construction of make_golden.py::g14_wellcond - chirps, harmonics and a 0.05 noise floor - as float32 (batch, length);
    a third item is a fixed mix of the first two."""
    assert 1 <= batch <= 3
    tt = np.arange(length) / 16000.0
    x = np.stack([
        0.5 * np.sin(2 * np.pi * (300 * tt + 2500 * tt * tt)) + 0.3 * np.sin(2 * np.pi * 1250 * tt + 3 * np.sin(2 * np.pi * 5 * tt)),
        sum(0.4 / k * np.sin(2 * np.pi * 220 * k * tt * (1 + 0.3 * tt)) for k in range(1, 9)),
    ]) + 0.05 * np.random.default_rng(seed).standard_normal((2, length))
    x = np.concatenate([x, 0.6 * x[:1] - 0.8 * x[1:]])
    return x[:batch].astype(np.float32)


def wellcond_spec(batch, n_fft, frames, kw, seed):
    """STFT (float32 arithmetic) of `wellcond` at the given stft kwargs, its length the one that gives `frames` frames, and the same
    magnitudes with the true phase perturbed by 0.5 rad rms: (spec, start) complex64"""
    F = n_fft // 2 + 1 if kw.get("onesided", True) else n_fft
    kw32 = {k: wide(v, np.float32).astype(np.float32) if isinstance(v, np.ndarray) else v for k, v in kw.items()}
    a, w = mt._setup(F, torch.float32, kw32)
    spec = mt.stft(torch.from_numpy(wellcond(batch, signal_length(frames, a), seed)), a, w)
    assert spec.shape == (batch, F, frames)
    phase = torch.angle(spec) + torch.from_numpy((0.5 * np.random.default_rng(seed + 1).standard_normal(spec.shape)).astype(np.float32))
    return spec.numpy(), torch.polar(spec.abs(), phase).numpy()


# ---- the end-to-end cases of tests/test_gpu_autograd.py ----------------------------------------------------------------------------
N_ITER = 3
COEF = {"gla": 0.5, "admm": 0.1}                                   # alpha, rho
# shape name: n_fft, hop, frames, batch, extra stft kwargs (center=False: a Hamming window, its envelope has no zeros)
SHAPES = {
    "128/32x150": (128, 32, 150, 3, {}),
    "512/128x80": (512, 128, 80, 2, {}),
    "1024/256x80": (1024, 256, 80, 2, {}),
    "2048/512x70": (2048, 512, 70, 2, {}),
    "400/160x70": (400, 160, 70, 2, {}),
    "512/100/300x70 two-sided": (512, 100, 70, 2, dict(win_length=300, onesided=False)),
    "4096/1024x12": (4096, 1024, 12, 2, {}),
    "1024/200x40": (1024, 200, 40, 2, {}),
    "1024/256x40 center=False": (1024, 256, 40, 2, dict(center=False)),
}
F64_MAG = ["128/32x150", "512/128x80", "1024/256x80", "2048/512x70", "400/160x70", "512/100/300x70 two-sided"]
F32_COMPLEX = ["512/128x80", "1024/256x80", "2048/512x70", "4096/1024x12", "1024/200x40", "1024/256x40 center=False", "128/32x150"]
F64_COMPLEX = ["1024/256x80"]
# case name: "<method> <shape> <mag|complex>"
CASES_F64_MAG = [f"{m} {s} mag" for s in F64_MAG for m in METHODS]
CASES_F32_COMPLEX = [f"{m} {s} complex" for s in F32_COMPLEX for m in METHODS]
CASES_F64_COMPLEX = [f"{m} {s} complex" for s in F64_COMPLEX for m in METHODS]
# A case's inputs are drawn at seed n_fft + hop + frames unless that misses its admission condition (tests/test_gla_torch_host.py:
# sens64 <= 1e-10 in float64, noise32 <= 1e-3 in float32, under both methods); then at the first seed from 0 that meets it, listed here
# by (shape, start).  A few bins decide either measure and it moves by a factor of two to three between CPUs, so a seed is taken only
# where it stays below half the cap (5e-11, 5e-4; _agla_torch.SEEDS does the same) - at 2048 / 512, where seed 5 gave 4.5e-4 on one
# CPU and 1.4e-3 on another, below a quarter.  Both methods share the inputs.
SEEDS = {("128/32x150", "mag"): 3, ("512/128x80", "complex"): 0, ("1024/256x80", "complex"): 0, ("2048/512x70", "complex"): 13,
         ("4096/1024x12", "complex"): 3, ("1024/256x40 center=False", "complex"): 1}


def split(name):
    method, rest = name.split(" ", 1)
    shape, start = rest.rsplit(" ", 1)
    return method, shape, start


def stft_kwargs(shape, dtype):
    n_fft, hop, frames, batch, extra = SHAPES[shape]
    wl = extra.get("win_length", n_fft)
    win = hamming(wl, dtype) if extra.get("center") is False else hann(wl, dtype)
    return dict(hop_length=hop, window=win, **extra)


def draw(shape, start, dtype, seed):
    n_fft, hop, frames, batch, extra = SHAPES[shape]
    kw = stft_kwargs(shape, dtype)
    spec, init = wellcond_spec(batch, n_fft, frames, kw, seed)
    a, _ = mt._setup(spec.shape[1], torch.float64, {k: wide(v, np.float64) for k, v in kw.items()})
    w = np.random.default_rng(7).standard_normal((batch, signal_length(frames, a))).astype(np.float32)
    s = np.abs(spec) if start == "mag" else init
    return s.astype(np.result_type(s.dtype, dtype)), w.astype(dtype), kw


@functools.lru_cache(maxsize=None)
def _inputs(shape, start, dtype):
    n_fft, hop, frames, _, _ = SHAPES[shape]
    return draw(shape, start, dtype, SEEDS.get((shape, start), n_fft + hop + frames))


def inputs(name, dtype):
    """(spec, w, kw) as NumPy arrays of `dtype`, float32-representable: `spec` (B, F, T) the magnitudes of the well-conditioned signal's
    STFT or its complex start, `w` the fixed random weights of the loss sum(w y)"""
    _, shape, start = split(name)
    return _inputs(shape, start, dtype)


@functools.lru_cache(maxsize=None)
def reference(name, dtype, compute=None):
    """Autograd on the restatement, on the CPU, the inputs of `dtype` computed in `compute` (default: `dtype`): (y, grad spec);
    computed once per case and left unchanged."""
    method = split(name)[0]
    spec, w, kw = inputs(name, dtype)
    y, g = grads(method, spec, w, N_ITER, COEF[method], kw, compute or dtype)
    y.setflags(write=False), g.setflags(write=False)
    return y, g


@functools.lru_cache(maxsize=None)
def noise32(name):
    return rel_l2(reference(name, np.float32)[1], reference(name, np.float32, np.float64)[1])


@functools.lru_cache(maxsize=None)
def sens64(name):
    method = split(name)[0]
    spec, w, kw = inputs(name, np.float64)
    g1 = grads(method, ulp_perturbed(spec, np.random.default_rng(52)), w, N_ITER, COEF[method], kw, np.float64)[1]
    return rel_l2(g1, reference(name, np.float64)[1])
