"""tests/_agla_oracle.py restated in torch with per-iteration parameters, so that autograd differentiates it on the CPU: the
reference of `agla_unfolded`'s gradients.  A helper of the AGLA tests, not a test file.

    C0 = spec (complex)  or  phase_init(spec) ;  c = istft(C0) ;  for n = 1 ... N:  S = stft(c) ;  y = istft(S m / (|S| + 1e-16))
        n = 1:  t = c = d = y
        n > 1:  t' = (1 - gamma_n) d + gamma_n y ;  c = t' + alpha_n (t' - t) ;  d = t' + beta_n (t' - t) ;  t = t'
    result: t

The transforms are tests/_misi_torch.py's.  All arithmetic in the real dtype of `spec`; alpha_n, beta_n, gamma_n and 1 - gamma_n
(formed in float64) are rounded to it once.  The general form is written for every gamma: with gamma_n = 1 the product
(1 - gamma_n) d is exactly 0 and t' = y to the bit, the oracle's form without d - and autograd still sees gamma.  The target m is
|spec| for a complex start and `spec` itself for magnitudes (what the device gets).  `phase_init` is oracle/methods.py's in torch
ops (the time cumsum of a float32 tensor accumulates in float64 on the CPU, as the oracle's does); the peak mask is piecewise
constant, the gradient flows through the parabolic offset and the product with the magnitude."""
import functools
import math

import numpy as np
import torch

from _misi_torch import _setup, envelope, istft, stft
from _util import hann
from oracle.stftlib import signal_length


def phase_advance(mag, a):
    """(B, F, T) real -> (B, F, T): the phase every bin advances by in its frame, the omega of the peak that owns it (0: none)"""
    dt = mag.dtype
    mid, up, dn = mag[:, 1:-1], mag[:, 2:], mag[:, :-2]
    peak = (mid > up) & (mid > dn)
    k = torch.arange(1, mag.shape[1] - 1, dtype=dt)[None, :, None]
    den = torch.where(peak, dn - 2 * mid + up, torch.ones_like(mid))          # (off the peaks: no 0 / 0 for autograd to meet)
    p = 0.5 * (dn - up) / den
    omega = torch.tensor(2 * math.pi, dtype=dt) * (k + p) / a.n_fft * a.hop_length
    om = torch.zeros_like(mag)
    om[:, 1:-1] = torch.where(peak, omega, torch.zeros_like(omega))
    pk = torch.zeros(mag.shape, dtype=torch.bool)
    pk[:, 1:-1] = peak
    z, zb = torch.zeros_like(mag[:, :1]), torch.zeros_like(pk[:, :1])
    below = torch.cat([om[:, 1:], z], 1)                                       # bin f takes omega[f + 1] if f + 1 is a peak ...
    pk_below = torch.cat([pk[:, 1:], zb], 1)
    above = torch.cat([z, om[:, :-1]], 1)                                      # ... omega[f - 1] if f - 1 is one (the later write)
    pk_above = torch.cat([zb, pk[:, :-1]], 1)
    phase = torch.where(pk_below, below, torch.zeros_like(mag))
    phase = torch.where(pk_above, above, phase)
    return torch.where(pk, om, phase)                                          # ... its own if it is one itself


def phase_init(mag, a):
    """(B, F, T) real -> (B, F, T) complex"""
    phi = torch.cumsum(phase_advance(mag, a), dim=2)
    return torch.complex(mag * torch.cos(phi), mag * torch.sin(phi))


def schedule(value, n_iter):
    """a float, a sequence or a tensor -> (n_iter,) float64 tensor (a tensor keeps its graph)"""
    t = value if isinstance(value, torch.Tensor) else torch.tensor(np.atleast_1d(np.asarray(value, np.float64)))
    return t.to(torch.float64).reshape(-1).expand(n_iter)


def agla(spec, n_iter, alpha=0.99, beta=None, gamma=1.0, record=None, **stft_kwargs):
    """spec (B, F, T) complex or real CPU tensor; alpha, beta (None: alpha), gamma floats or (n_iter,) tensors / sequences, element
    n - 1 for iteration n.  Returns t_N (B, L); differentiable with respect to `spec` and the parameter tensors.  `record`, a list,
    receives c_0, t_1, ..., t_N."""
    B, F, T = spec.shape
    rdt = spec.real.dtype if spec.is_complex() else spec.dtype
    a, w = _setup(F, rdt, stft_kwargs)
    env = envelope(T, a, w)
    C, m = (spec, spec.abs()) if spec.is_complex() else (phase_init(spec, a), spec)
    al64 = schedule(alpha, n_iter)
    be64 = al64 if beta is None else schedule(beta, n_iter)
    ga64 = schedule(gamma, n_iter)
    al, be, ga, omg = al64.to(rdt), be64.to(rdt), ga64.to(rdt), (1.0 - ga64).to(rdt)
    c = istft(C, a, w, env)
    if record is not None:
        record.append(c)
    t = d = None
    for n in range(1, n_iter + 1):
        y = project(c, m, a, w, env)
        if n == 1:
            t = c = d = y
        else:
            tn = omg[n - 1] * d + ga[n - 1] * y
            diff = tn - t
            c = tn + al[n - 1] * diff
            d = tn + be[n - 1] * diff
            t = tn
        if record is not None:
            record.append(t)
    return t


def project(c, m, a, w, env):
    """P(c) = istft(S m / (|S| + 1e-16)), S = stft(c): one Griffin-Lim iteration without momentum"""
    S = stft(c, a, w)
    return istft(S * m / (S.abs() + 1e-16), a, w, env)


# ---- the cases of tests/test_gpu_agla_unfolded.py, here so that tests/test_agla_unfolded_host.py can pin their float32 noise ----
N_ITER = 4
# name: n_fft, hop, frames, extra stft kwargs; B = 2
CONFIGS = {
    "128/32": (128, 32, 10, {}),                                               # k_wave_iter
    "400/160": (400, 160, 12, {}),                                             # k_wave_iter, no power of two
    "1024/256": (1024, 256, 16, {}),                                           # chunked: k_fused4, two chunks, chunk tails
    "64/16 two-sided normalized": (64, 16, 11, dict(onesided=False, normalized=True)),
}
# (alpha, beta, gamma): Fast Griffin-Lim at the default momentum, constant; a schedule around (0.5, 1.2, 0.7), all sequences live
SCHEDULES = {
    "fgla": (0.99, None, 1.0),
    "general": ((0.5, 0.45, 0.6, 0.55), (1.2, 1.1, 1.3, 1.25), (0.7, 0.8, 0.65, 0.75)),
}
# The float32 cases, (name, magnitude start): seed.  The seeds are the first at which the restatement's own float32-against-float64
# gradient error stays below 5e-4 under both schedules (tests/test_agla_unfolded_host.py asserts 1e-3).  A magnitude start at
# 400/160 or 1024/256 is no float32 case: phase_init sums phases of thousands of radians over the frames, the float32 start
# then differs from the float64 one by 1e-4 and the gradients by 2e-3 at the best of 200 seeds.
SEEDS = {("128/32", False): 1, ("128/32", True): 9, ("400/160", False): 5, ("1024/256", False): 4,
         ("64/16 two-sided normalized", False): 2, ("64/16 two-sided normalized", True): 5}
FLOAT32_CASES = list(SEEDS)
# 400/160 from magnitudes runs in float64 alone, at the best conditioned of those 200 seeds by the same CPU-only measure (2.1e-3;
# at the default seed a bin of the start passes close to zero and the restatement's float32 gradient is off by 300 %)
SEEDS[("400/160", True)] = 1


@functools.lru_cache(maxsize=None)
def inputs(name, dtype, magnitude_start):
    """(spec, w, L, kw) as NumPy arrays: `spec` (2, F, T) complex or its modulus - mag = rng.random + 0.05 with uniform phases, as
    tests/test_gpu_agla.py draws them - and `w` the fixed random weights of the loss sum(w * y)"""
    n_fft, hop, frames, extra = CONFIGS[name]
    rng = np.random.default_rng(SEEDS.get((name, magnitude_start), n_fft + hop + frames))
    kw = dict(hop_length=hop, window=hann(n_fft, dtype), **extra)
    F = n_fft // 2 + 1 if extra.get("onesided", True) else n_fft
    mag = (rng.random((2, F, frames)) + 0.05).astype(dtype)
    start = (mag * np.exp(1j * rng.uniform(-np.pi, np.pi, mag.shape))).astype(np.complex64 if dtype == np.float32 else np.complex128)
    a, _ = _setup(F, torch.float64, kw)
    L = signal_length(frames, a)
    w = np.random.default_rng(7).standard_normal((2, L)).astype(dtype)
    return (mag if magnitude_start else start), w, L, kw


@functools.lru_cache(maxsize=None)
def reference(name, dtype, magnitude_start, sched, compute=None):
    """Autograd on the restatement, on the CPU, the inputs of `dtype` computed in `compute` (default: `dtype`): (y, grad spec, grad
    alpha, grad beta, grad gamma) as NumPy arrays, the parameter gradients float64 (n_iter,); computed once per case."""
    spec, w, L, kw = inputs(name, dtype, magnitude_start)
    compute = compute or dtype
    wide = lambda x: x.astype(np.result_type(x.dtype, compute))                # noqa: E731
    al, be, ga = SCHEDULES[sched]
    s = torch.from_numpy(wide(spec)).requires_grad_(True)
    par = [schedule(v, N_ITER).clone().requires_grad_(True) for v in (al, al if be is None else be, ga)]
    y = agla(s, N_ITER, *par, **dict(kw, window=wide(kw["window"])))
    (y * torch.from_numpy(wide(w))).sum().backward()
    return (y.detach().numpy(), s.grad.numpy()) + tuple(p.grad.numpy() for p in par)
