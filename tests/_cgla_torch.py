"""tests/_cgla_oracle.py (its split form, what the library computes) restated in torch with per-iteration parameters, so that
autograd differentiates it on the CPU: the reference of `constrained_unfolded`'s gradients.  A helper of the constrained tests, not
a test file.  With M the mask of known bins, K their values, W the mask of known samples, xk their values:

    m = |spec| or spec ;  m_full = where(M, |K|, m) ;  m' = where(M, 0, m)
    start = where(M, K, spec)  (a real spec: where(M, K, phase_init(m_full))) ;  c = istft(start) ;  k = istft(where(M, K, 0))
    for n = 1 ... N:  u = P_m'(c) + k
        n = 1:  t = c = d = where(W, xk, u)
        n > 1:  t' = where(W, xk, (1 - gamma_n) d + gamma_n u) ;  c = t' + alpha_n (t' - t) ;  d = t' + beta_n (t' - t) ;  t = t'
    result: t

`phase_init`, `project` and `schedule` are tests/_agla_torch.py's, the transforms tests/_misi_torch.py's.  All arithmetic in the
real dtype of `spec`; alpha_n, beta_n, gamma_n and 1 - gamma_n (formed in float64) are rounded to it once.  With gamma_n = 1 the
product (1 - gamma_n) d is exactly 0 and the relaxation returns u to the bit, the oracle's form without d.  Differentiable in `spec`,
`known_spec`, `known_wave`, alpha, beta and gamma; the masks are constants."""
import functools

import numpy as np
import torch

import _agla_torch as at
from _misi_torch import _setup, envelope, istft
from _util import hann
from oracle.stftlib import args_helper as np_args, signal_length, stft as np_stft


def cgla(spec, n_iter, known_spec=None, spec_mask=None, known_wave=None, wave_mask=None, alpha=0.99, beta=None, gamma=1.0,
         record=None, **stft_kwargs):
    """spec (B, F, T) complex or real CPU tensor; known_spec (B, F, T) complex with spec_mask, known_wave (B, L) with wave_mask, the
    masks bool and of their values' shapes; alpha, beta (None: alpha), gamma floats or (n_iter,) tensors / sequences, element n - 1
    for iteration n.  Returns t_N (B, L).  `record`, a list, receives c_0, t_1, ..., t_N."""
    B, F, T = spec.shape
    rdt = spec.real.dtype if spec.is_complex() else spec.dtype
    a, w = _setup(F, rdt, stft_kwargs)
    env = envelope(T, a, w)
    m = spec.abs() if spec.is_complex() else spec
    if known_spec is not None:
        M, K = spec_mask, known_spec
        m_full = torch.where(M, K.abs(), m)
        m_free = torch.where(M, torch.zeros_like(m), m)
        start = torch.where(M, K, spec if spec.is_complex() else at.phase_init(m_full, a))
        k = istft(torch.where(M, K, torch.zeros_like(K)), a, w, env)
    else:
        m_free = m
        start = spec if spec.is_complex() else at.phase_init(m, a)
        k = None
    al64 = at.schedule(alpha, n_iter)
    be64 = al64 if beta is None else at.schedule(beta, n_iter)
    ga64 = at.schedule(gamma, n_iter)
    al, be, ga, omg = al64.to(rdt), be64.to(rdt), ga64.to(rdt), (1.0 - ga64).to(rdt)
    c = istft(start, a, w, env)
    if record is not None:
        record.append(c)
    select = (lambda v: v) if known_wave is None else (lambda v: torch.where(wave_mask, known_wave, v))   # noqa: E731
    t = d = None
    for n in range(1, n_iter + 1):
        u = at.project(c, m_free, a, w, env)
        if k is not None:
            u = u + k
        if n == 1:
            t = c = d = select(u)
        else:
            tn = select(omg[n - 1] * d + ga[n - 1] * u)
            diff = tn - t
            c = tn + al[n - 1] * diff
            d = tn + be[n - 1] * diff
            t = tn
        if record is not None:
            record.append(t)
    return t


# ---- the cases of tests/test_gpu_cgla_unfolded.py, here so that tests/test_cgla_unfolded_host.py can pin their float32 noise ----
N_ITER = at.N_ITER
CONFIGS = at.CONFIGS                      # 128/32 x 10 frames, 400/160 x 12, 1024/256 x 16, 64/16 two-sided normalized x 11; B = 2
SCHEDULES = at.SCHEDULES                  # "fgla" and "general"
CONSTRAINTS = ("spec", "wave", "both")    # known bins alone, known samples alone, both
# The float32 cases, (name, magnitude start): seed.  Chosen on the CPU: the first seed at which the restatement's own
# float32-against-float64 gradient error, over the six inputs, the two schedules and the three constraints, stays below 5e-4
# (tests/test_cgla_unfolded_host.py asserts 1e-3).  A magnitude start at 400/160 or 1024/256 is no float32 case, for the reason
# given in tests/_agla_torch.py (phase_init sums phases of thousands of radians over the frames).
SEEDS = {("128/32", False): 0, ("128/32", True): 135, ("400/160", False): 0, ("1024/256", False): 19,
         ("64/16 two-sided normalized", False): 0, ("64/16 two-sided normalized", True): 8}
FLOAT32_CASES = list(SEEDS)
# 400/160 from magnitudes runs in float64 alone, at the best conditioned of the seeds 0 ... 119 by the same CPU-only measure (1.1e-2)
SEEDS[("400/160", True)] = 40


@functools.lru_cache(maxsize=None)
def inputs(name, dtype, magnitude_start, seed=None):
    """A case as NumPy arrays, a dict: `spec` (2, F, T) complex or its modulus, `known_spec` K = STFT of a real test signal (the
    sines of tests/test_gpu_cgla.py plus noise) with `spec_mask`, `known_wave` that signal with `wave_mask`, `w` the fixed random
    weights of the loss sum(w * y), `L` and `kw`.  The signal is scaled so that its largest bin has modulus 1; the target off the mask
    is rng.random + 0.05 with uniform random phases, as tests/_agla_torch.py draws it.
    The masks are tests/test_gpu_cgla.py's: the bins below F / 4 + b plus two whole frames (two-sided: the frames alone, which keeps
    the mask Hermitian); the samples [0, L / 3 + b) plus a run of 37 from an odd index, so that mask edges fall inside a thread's
    vector."""
    n_fft, hop, frames, extra = CONFIGS[name]
    rng = np.random.default_rng(SEEDS[(name, magnitude_start)] if seed is None else seed)
    kw = dict(hop_length=hop, window=hann(n_fft, dtype), **extra)
    onesided = extra.get("onesided", True)
    F = n_fft // 2 + 1 if onesided else n_fft
    a = np_args(F, dtype, **kw)
    L = signal_length(frames, a)
    n = np.arange(L)
    x = np.stack([np.sin(2 * np.pi * (0.013 + 0.007 * b) * n) * (1 + 0.5 * np.sin(2 * np.pi * n / 211)) for b in range(2)])
    x = x + 0.1 * rng.standard_normal(x.shape)
    x = (x / np.abs(np_stft(x.astype(dtype), a)).max()).astype(dtype)           # (the largest known bin has modulus 1)
    K = np_stft(x, a)
    mag = (rng.random(K.shape) + 0.05).astype(dtype)
    start = (mag * np.exp(1j * rng.uniform(-np.pi, np.pi, mag.shape))).astype(K.dtype)
    M = np.zeros((2, F, frames), bool)
    W = np.zeros((2, L), bool)
    for b in range(2):
        if onesided:
            M[b, : F // 4 + b] = True
        M[b, :, [(frames // 2 - 1 + b) % frames, (frames // 2 + b) % frames]] = True
        W[b, : L // 3 + b] = True
        lo = (L // 2 | 1) + 2 * b
        assert lo % 2 == 1 and lo + 37 <= L
        W[b, lo: lo + 37] = True
    w = np.random.default_rng(7).standard_normal((2, L)).astype(dtype)
    return dict(spec=mag if magnitude_start else start, known_spec=K, spec_mask=M, known_wave=x, wave_mask=W, w=w, L=L, kw=kw)


def constraint(c, which):
    """The keyword arguments of a case's constraint: "spec", "wave" or "both" """
    keys = {"spec": ("known_spec", "spec_mask"), "wave": ("known_wave", "wave_mask"),
            "both": ("known_spec", "spec_mask", "known_wave", "wave_mask")}[which]
    return {k: c[k] for k in keys}


GRADS = ("spec", "known_spec", "known_wave", "alpha", "beta", "gamma")


@functools.lru_cache(maxsize=None)
def reference(name, dtype, magnitude_start, sched, which="both", compute=None, seed=None):
    """Autograd on the restatement, on the CPU, the inputs of `dtype` computed in `compute` (default: `dtype`): (y, then the
    gradients in the order of GRADS) as NumPy arrays, None for an input the constraint does not have, the parameter gradients
    float64 (n_iter,); computed once per case."""
    c = inputs(name, dtype, magnitude_start, seed)
    compute = compute or dtype
    wide = lambda x: x if x.dtype == bool else x.astype(np.result_type(x.dtype, compute))                # noqa: E731
    al, be, ga = SCHEDULES[sched]
    s = torch.from_numpy(wide(c["spec"])).requires_grad_(True)
    con = {k: torch.from_numpy(wide(v)) for k, v in constraint(c, which).items()}
    for k in ("known_spec", "known_wave"):
        if k in con:
            con[k].requires_grad_(True)
    par = [at.schedule(v, N_ITER).clone().requires_grad_(True) for v in (al, al if be is None else be, ga)]
    y = cgla(s, N_ITER, alpha=par[0], beta=par[1], gamma=par[2], **con, **dict(c["kw"], window=wide(c["kw"]["window"])))
    (y * torch.from_numpy(wide(c["w"]))).sum().backward()
    g = lambda k: con[k].grad.numpy() if k in con else None                                              # noqa: E731
    return (y.detach().numpy(), s.grad.numpy(), g("known_spec"), g("known_wave")) + tuple(p.grad.numpy() for p in par)
