"""`phase_vocoder(..., phase_lock="pghi")` in NumPy on the CPU, twice: `pghi_ref` is the definition as it is written
(the two clamp recurrences run sequentially, the roots resolved from the codes), `pghi_heap` is a literal per-frame heap on `heapq`
(Prusa & Holighaus 2017 in this package's frame-resampling vocoder), kept only to show that the definition is the heap's result.
Symbols not defined here are tests/_pvoc_torch.py's.

    q(z) = re * re + im * im in float64 from the input's own bits ;  r(z) = sqrt(q(z))
    m_j[k] = fl(fl(a r(S1[k])) + fl(fl(1 - a) r(S0[k]))) ;  floor = tol * sqrt(max q over the item's input)
    live(j, k) iff m_j[k] > 0 and m_j[k] >= floor
    frame 0: psi_0 = theta0 ; code 0 where live, 3 elsewhere
    frame j >= 1: c[k] = m_j[k] if live else -inf ; p[k] = m_{j-1}[k] if live(j-1, k) else -inf
        Lf[0] = -inf, Lf[k] = min(c[k-1], max(p[k-1], Lf[k-1])) ;  Rg[F-1] = -inf, Rg[k] = min(c[k+1], max(p[k+1], Rg[k+1]))
        live bin, b = max(p, Lf, Rg): code 0 if p >= b, else 1 if Lf >= b, else 2 ; not live: 3
        phi_j[k] = psi_{j-1}[k] + d_{j-1}[k]
        root(k) = k for codes 0 and 3 ; root(k+1) for code 2 (resolved first) ; root(k-1) for code 1
        psi_j[k] = phi_j[k] if root(k) = k, else (phi_j[root] - theta0_j[root]) + theta0_j[k]
    P[j][k] = (m cos psi, m sin psi)

Both take one item (F, T) or a batch (B, F, T), complex64 or complex128 as a torch tensor or an array, and return `(P, psi, codes)`:
complex128 not rounded, float64, int8.  `angle_dtype` is the dtype the two angles are taken in (float32 only for complex64 input);
everything after them is float64."""
import heapq
import math

import numpy as np
import torch

from _pvoc_torch import frames_out

NEG = -np.inf


def _parts(s, rate, n_fft, hop, tol, angle_dtype):
    """(m, live, th0, d) of one item s (F, T): float64 (F, T_out) each, live bool"""
    F, T = s.shape
    assert F == n_fft // 2 + 1 and rate > 0 and 0 < tol < 1
    real = np.float32 if s.dtype == np.complex64 else np.float64
    assert angle_dtype == np.float64 or real == np.float32
    n_out = frames_out(T, rate)
    t = np.arange(n_out, dtype=np.float64) * np.float64(rate)
    fl = np.floor(t)
    i = fl.astype(np.int64)
    a = t - fl
    sp = np.concatenate([s, np.zeros((F, 2), s.dtype)], 1)
    re, im = sp.real.astype(np.float64), sp.imag.astype(np.float64)
    q = re * re + im * im
    r = np.sqrt(q)
    m = a * r[:, i + 1] + (1.0 - a) * r[:, i]
    floor = np.float64(tol) * np.sqrt(q.max())
    live = (m > 0) & (m >= floor)
    th = np.arctan2(sp.imag.astype(angle_dtype), sp.real.astype(angle_dtype)).astype(np.float64)
    th0, th1 = th[:, i], th[:, i + 1]
    adv = (2 * math.pi * np.arange(F, dtype=np.float64) * hop / n_fft)[:, None]
    two_pi = 2 * math.pi
    d = th1 - th0 - adv
    d = d - two_pi * np.round(d / two_pi)
    d = d + adv
    return m, live, th0, d


def frame_codes(c, p):
    """the codes of one frame from c and p (-inf where not live)"""
    F = c.shape[0]
    Lf = np.full(F, NEG)
    for k in range(1, F):
        Lf[k] = min(c[k - 1], max(p[k - 1], Lf[k - 1]))
    Rg = np.full(F, NEG)
    for k in range(F - 2, -1, -1):
        Rg[k] = min(c[k + 1], max(p[k + 1], Rg[k + 1]))
    code = np.full(F, 3, np.int8)
    for k in range(F):
        if c[k] > NEG:
            b = max(p[k], Lf[k], Rg[k])
            code[k] = 0 if p[k] >= b else 1 if Lf[k] >= b else 2
    return code


def frame_codes_heap(c, p):
    """the same frame by the heap: seeded with the live bins of the previous frame under p; a popped previous-frame entry sets its
    own bin by time, a popped current-frame entry sets its unset live neighbours k + 1 (code 1) and k - 1 (code 2) and pushes them
    under c; live bins left over get code 0.  Among equal keys Python's tuple order decides: the definition fixes its own rule."""
    F = c.shape[0]
    code = np.full(F, 3, np.int8)
    done = np.zeros(F, bool)
    h = []
    for k in range(F):
        if p[k] > NEG:
            heapq.heappush(h, (-p[k], k, 0))
    while h:
        _, k, cur = heapq.heappop(h)
        if not cur:
            if c[k] > NEG and not done[k]:
                code[k], done[k] = 0, True
                heapq.heappush(h, (-c[k], k, 1))
            continue
        if k + 1 < F and c[k + 1] > NEG and not done[k + 1]:
            code[k + 1], done[k + 1] = 1, True
            heapq.heappush(h, (-c[k + 1], k + 1, 1))
        if k - 1 >= 0 and c[k - 1] > NEG and not done[k - 1]:
            code[k - 1], done[k - 1] = 2, True
            heapq.heappush(h, (-c[k - 1], k - 1, 1))
    for k in range(F):
        if c[k] > NEG and not done[k]:
            code[k] = 0
    return code


def roots(code):
    """root(k) of one frame's codes"""
    F = code.shape[0]
    root = np.arange(F)
    for k in range(F - 2, -1, -1):
        if code[k] == 2:
            root[k] = root[k + 1]
    for k in range(1, F):
        if code[k] == 1:
            root[k] = root[k - 1]
    return root


def _item(s, rate, n_fft, hop, tol, angle_dtype, codes_of):
    m, live, th0, d = _parts(s, rate, n_fft, hop, tol, angle_dtype)
    F, n_out = m.shape
    psi = np.empty((F, n_out), np.float64)
    codes = np.empty((F, n_out), np.int8)
    psi[:, 0] = th0[:, 0]
    codes[:, 0] = np.where(live[:, 0], 0, 3)
    k = np.arange(F)
    for j in range(1, n_out):
        c = np.where(live[:, j], m[:, j], NEG)
        p = np.where(live[:, j - 1], m[:, j - 1], NEG)
        code = codes_of(c, p)
        phi = psi[:, j - 1] + d[:, j - 1]
        root = roots(code)
        psi[:, j] = np.where(root == k, phi, (phi[root] - th0[root, j]) + th0[:, j])
        codes[:, j] = code
    return m * np.cos(psi) + 1j * (m * np.sin(psi)), psi, codes


def _run(spec, rate, n_fft, hop, tol, angle_dtype, codes_of):
    if isinstance(spec, torch.Tensor):
        spec = spec.detach().cpu().resolve_conj().numpy()
    spec = np.asarray(spec)
    assert spec.dtype in (np.complex64, np.complex128) and spec.ndim in (2, 3)
    angle_dtype = {torch.float32: np.float32, torch.float64: np.float64}.get(angle_dtype, angle_dtype)
    if spec.ndim == 2:
        return _item(spec, rate, n_fft, hop, tol, angle_dtype, codes_of)
    res = [_item(s, rate, n_fft, hop, tol, angle_dtype, codes_of) for s in spec]
    return tuple(np.stack(x) for x in zip(*res))


def pghi_ref(spec, rate, n_fft, hop, tol=1e-6, angle_dtype=np.float64):
    return _run(spec, rate, n_fft, hop, tol, angle_dtype, frame_codes)


def pghi_heap(spec, rate, n_fft, hop, tol=1e-6, angle_dtype=np.float64):
    return _run(spec, rate, n_fft, hop, tol, angle_dtype, frame_codes_heap)


def random_spec(F, T, seed, batch=3, dtype=np.complex128, zeros=0.1, quiet=1.0 / 7):
    """(batch, F, T) complex: distinct magnitudes on a geometric grid from 1e-3 to 1 in seeded order at seeded phases, a different
    maximum per item (0.1, 1, 10, ...), a tenth of the bins exact zeros and a seventh scaled by 1e-8, below the default floor"""
    rng = np.random.default_rng(seed)
    items = []
    for b in range(batch):
        mag = np.exp(np.linspace(np.log(1e-3), 0.0, F * T))[rng.permutation(F * T)].reshape(F, T)
        mag[rng.random((F, T)) < quiet] *= 1e-8
        mag[rng.random((F, T)) < zeros] = 0.0
        ph = rng.uniform(-np.pi, np.pi, (F, T))
        items.append(mag * np.exp(1j * ph) * 10.0 ** (b - 1))
    return np.stack(items).astype(dtype)


def signal(name, n, seed=5):
    """the four test signals, float64 (n,)"""
    from _pvoc_lock_torch import harmonic_wave
    if name == "harmonic":
        return harmonic_wave(n, 1, seed)[0]
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64)
    if name == "chirp":
        return torch.sin(2 * math.pi * (0.02 * t + 0.1 * t * t / (2 * n))) + 0.3 * torch.randn(n, generator=g, dtype=torch.float64)
    if name == "noise":
        return torch.randn(n, generator=g, dtype=torch.float64)
    assert name == "clicks"
    x = 0.3 * torch.sin(2 * math.pi * 0.05 * t)
    x[::1500] += 3.0
    return x + 0.001 * torch.randn(n, generator=g, dtype=torch.float64)


def signal_spec(name, n_fft, hop, frames, seed=5):
    """(S, window): the signal's one-sided float64 spectrogram of `frames` frames under the periodic Hann window"""
    x = signal(name, (frames - 1) * hop, seed)
    w = torch.hann_window(n_fft, dtype=torch.float64)
    s = torch.stft(x, n_fft, hop_length=hop, window=w, return_complex=True)
    assert s.shape[-1] == frames
    return s, w
