"""Identity phase locking's definition in torch on the CPU: what `phase_vocoder(..., phase_lock="identity")` is tested
against.  Every symbol not defined here is tests/_pvoc_torch.py's.

For output frame j, S0 = S[i] and S1 = S[i + 1] (frames at and beyond T are +0 + 0i), theta = arg S0 in `angle_dtype`, m and the
unlocked running phase phi exactly those of `pvoc_ref`.

    q[k]   = re * re + im * im of S0[k] in float64 from the input's own bits
    peak   : q[k] > q[k'] for k' = k - 2, k - 1, k + 1, k + 2 - modulo n_fft on a two-sided spectrum, dropped outside 0 .. F - 1 on a
             one-sided one, dropped where k' + k = 0 mod n_fft (the bin's own mirror image)
    p(k)   = the nearest peak of the frame: |k - p|, circular on a two-sided spectrum; ties to the smaller |k_s|, then the lower index
    psi[k] = (phi[p(k)] - theta[p(k)]) + theta[k] ;  psi = phi in a frame without a peak
    P[j]   = m (cos psi + i sin psi)

The owner is found by brute force over all (bin, peak) pairs, a few frames at a time.  `lock_ref` returns complex128, not rounded;
`peaks_and_owners` returns what it decided."""
import math

import torch

from _pvoc_torch import _advance, _sources

_BIG = 1 << 60


def _signed_abs(n_freq, n_fft):
    k = torch.arange(n_freq, dtype=torch.int64)
    return torch.where(k <= n_fft // 2, k, n_fft - k)


def find_peaks(q, n_fft, onesided):
    """q (..., F, T) float64 -> bool (..., F, T)"""
    n_freq = q.shape[-2]
    assert n_freq == (n_fft // 2 + 1 if onesided else n_fft) and n_freq >= 2
    k = torch.arange(n_freq, dtype=torch.int64)
    peak = torch.ones_like(q, dtype=torch.bool)
    for d in (-2, -1, 1, 2):
        if onesided:
            drop = (k + d < 0) | (k + d >= n_freq)
            idx = (k + d).clamp(0, n_freq - 1)
        else:
            drop = (2 * k + d) % n_fft == 0
            idx = (k + d) % n_fft
        peak &= (q > q[..., idx, :]) | drop[:, None]
    return peak


def find_owners(peak, n_fft, onesided):
    """peak (F, T) bool -> owner (F, T) int64, -1 throughout a frame without a peak"""
    n_freq, n_frames = peak.shape
    k = torch.arange(n_freq, dtype=torch.int64)
    dist = (k[:, None] - k[None, :]).abs()                                  # [bin, peak]
    if not onesided:
        dist = torch.minimum(dist, n_fft - dist)
    key = (dist * (n_fft + 1) + _signed_abs(n_freq, n_fft)[None, :]) * n_freq + k[None, :]
    owner = torch.empty(n_freq, n_frames, dtype=torch.int64)
    step = max(1, (1 << 22) // (n_freq * n_freq))
    for t0 in range(0, n_frames, step):
        pk = peak[:, t0:t0 + step]                                          # (peak, t)
        cost = torch.where(pk[None, :, :], key[:, :, None], torch.tensor(_BIG))
        best, arg = cost.min(1)
        owner[:, t0:t0 + step] = torch.where(best < _BIG, arg, torch.tensor(-1))
    return owner


def _parts(spec, rate, n_fft, hop, angle_dtype):
    spec = spec.detach().cpu()
    assert spec.is_complex() and spec.dim() in (2, 3) and rate > 0
    real = torch.float32 if spec.dtype == torch.complex64 else torch.float64
    assert angle_dtype == torch.float64 or real == torch.float32
    s0, s1, a = _sources(spec, rate)
    q = s0.real.to(torch.float64) * s0.real.to(torch.float64) + s0.imag.to(torch.float64) * s0.imag.to(torch.float64)
    th0 = torch.atan2(s0.imag.to(angle_dtype), s0.real.to(angle_dtype)).to(torch.float64)
    th1 = torch.atan2(s1.imag.to(angle_dtype), s1.real.to(angle_dtype)).to(torch.float64)
    s0, s1 = s0.to(torch.complex128), s1.to(torch.complex128)
    m = a * s1.abs() + (1 - a) * s0.abs()
    adv = _advance(spec.shape[-2], n_fft, hop)
    two_pi = 2 * math.pi
    d = th1 - th0 - adv
    d = d - two_pi * torch.round(d / two_pi)
    d = d + adv
    phi = torch.cumsum(torch.cat([th0[..., :1], d[..., :-1]], -1), -1)
    return q, th0, m, phi


def _onesided(spec, n_fft, onesided):
    if onesided is None:
        onesided = spec.shape[-2] != n_fft
    assert spec.shape[-2] == (n_fft // 2 + 1 if onesided else n_fft)
    return onesided


def peaks_and_owners(spec, rate, n_fft, hop, onesided=None):
    """(peak, owner) of every output frame: bool and int64 of the output's shape, owner -1 where the frame has no peak"""
    onesided = _onesided(spec, n_fft, onesided)
    q = _parts(spec, rate, n_fft, hop, torch.float64)[0]
    peak = find_peaks(q, n_fft, onesided)
    flat = peak.reshape((-1,) + peak.shape[-2:])
    owner = torch.stack([find_owners(p, n_fft, onesided) for p in flat]).reshape(peak.shape)
    return peak, owner


def lock_ref(spec, rate, n_fft, hop, angle_dtype=torch.float64, onesided=None, return_phase=False):
    onesided = _onesided(spec, n_fft, onesided)
    q, th0, m, phi = _parts(spec, rate, n_fft, hop, angle_dtype)
    peak = find_peaks(q, n_fft, onesided)
    flat = peak.reshape((-1,) + peak.shape[-2:])
    owner = torch.stack([find_owners(p, n_fft, onesided) for p in flat]).reshape(peak.shape)
    has = owner >= 0
    own = owner.clamp(min=0)
    r = phi - th0
    psi = torch.where(has, torch.gather(r, -2, own) + th0, phi)
    if return_phase:
        return psi
    return torch.complex(m * torch.cos(psi), m * torch.sin(psi))


def inconsistency(p, n_fft, hop, window):
    """|| |STFT(ISTFT(P))| - |P| || / || |P| || of a one-sided P, in float64 on the CPU"""
    p = p.detach().cpu().to(torch.complex128)
    w = window.detach().cpu().to(torch.float64)
    y = torch.istft(p, n_fft, hop_length=hop, window=w)
    s = torch.stft(y, n_fft, hop_length=hop, window=w, return_complex=True)
    assert s.shape == p.shape
    return float(torch.linalg.norm(s.abs() - p.abs()) / torch.linalg.norm(p.abs()))


def harmonic_wave(n, batch, seed, f0=0.031):
    """eight harmonics with 1 % vibrato plus 1 % noise, float64 (batch, n)"""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64)
    inst = 2 * math.pi * f0 * (t + 0.01 / (2 * math.pi * 0.0004) * torch.sin(2 * math.pi * 0.0004 * t))
    x = sum(torch.sin(h * inst + 0.7 * h) / h for h in range(1, 9))
    return x + 0.01 * torch.randn(batch, n, generator=g, dtype=torch.float64)


# The synthetic comb: n_fft 32 one-sided (F = 17), integer magnitudes (comb_spec: times five), a frame per row, and the owners
# they must give.
COMB_N_FFT, COMB_HOP = 32, 8
COMB_MAG = [
    # peaks at bin 0 and bin F - 1, at 4 and 10; bins 2, 7 and 13 lie midway between two peaks and go to the lower one
    [9, 1, 1, 1, 7, 1, 1, 1, 1, 1, 8, 1, 1, 1, 1, 1, 9],
    # a two-bin plateau at 3, 4 (neither is a peak); peaks at 8 and 13
    [1, 1, 1, 5, 5, 1, 1, 1, 6, 1, 1, 1, 1, 7, 1, 1, 1],
    # one peak
    [1, 1, 1, 1, 1, 1, 4, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1],
    # equal values: none
    [3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3, 3],
    # silence: none
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    # bin 2 exceeds its nearest neighbours but not bin 4, two bins away: only 4 is a peak; 15 is one next to the edge
    [1, 1, 5, 1, 6, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 1],
]
COMB_OWNER = [
    [0, 0, 0, 4, 4, 4, 4, 4, 10, 10, 10, 10, 10, 10, 16, 16, 16],
    [8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 8, 13, 13, 13, 13, 13, 13],
    [6] * 17,
    [-1] * 17,
    [-1] * 17,
    [4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 15, 15, 15, 15, 15, 15, 15],
]


def comb_spec(dtype=torch.complex128, seed=11):
    """(F, frames) complex: five times the comb's magnitudes at seeded random phases out of twelve directions with integer
    components, (+-5, 0), (0, +-5), (+-3, +-4), (+-4, +-3) / 5, so that re * re + im * im is exact and equal magnitudes are equal q"""
    g = torch.Generator().manual_seed(seed)
    mag = torch.tensor(COMB_MAG, dtype=torch.float64).T
    dirs = torch.tensor([(5, 0), (-5, 0), (0, 5), (0, -5), (3, 4), (3, -4), (-3, 4), (-3, -4), (4, 3), (4, -3), (-4, 3), (-4, -3)],
                        dtype=torch.float64)
    pick = dirs[torch.randint(0, 12, mag.shape, generator=g)]
    return torch.complex(mag * pick[..., 0], mag * pick[..., 1]).to(dtype)
