"""The phase vocoder's definition in torch on the CPU: what `phase_vocoder` is tested against.

Input S (B, F, T) / (F, T) complex, rate > 0.  T_out is the smallest n >= 1 with float(n) * rate >= T.  For output frame j:
t_j = float(j) * rate, i = floor(t_j), a = t_j - i; frames at and beyond T are +0 + 0i;

    m_j   = a |S[i+1]| + (1 - a) |S[i]|
    d_j   = wrap(arg S[i+1] - arg S[i] - adv) + adv ,  wrap(x) = x - 2 pi round(x / 2 pi) ,  adv = 2 pi k_s hop / n_fft
    phi_0 = arg S[0] ,  phi_j = phi_{j-1} + d_{j-1} ;   P[j] = m_j (cos phi_j + i sin phi_j)

with k_s = k up to n_fft / 2 and k - n_fft above it, and arg z = atan2(im, re), 0 at +0 + 0i.  `pvoc_ref` takes the two angles in
`angle_dtype` from the input's own bits and computes everything after them in float64; the result is complex128, not rounded."""
import math

import torch


def frames_out(n_frames, rate):
    n = 1
    while float(n) * rate < n_frames:
        n += 1
    return n


def _sources(spec, rate):
    """(S0, S1, a): the two source frames of every output frame as complex128 (B, F, T_out), and the second's weight"""
    n_out = frames_out(spec.shape[-1], rate)
    t = torch.arange(n_out, dtype=torch.float64) * rate
    fl = torch.floor(t)
    i = fl.to(torch.int64)
    pad = torch.zeros(spec.shape[:-1] + (2,), dtype=spec.dtype)
    sp = torch.cat([spec, pad], -1)
    return sp[..., i], sp[..., i + 1], t - fl


def _advance(n_freq, n_fft, hop):
    k = torch.arange(n_freq, dtype=torch.float64)
    ks = torch.where(k <= n_fft // 2, k, k - n_fft)
    return (2 * math.pi * ks * hop / n_fft)[:, None]


def pvoc_ref(spec, rate, n_fft, hop, angle_dtype=torch.float64):
    spec = spec.detach().cpu()
    assert spec.is_complex() and spec.dim() in (2, 3) and rate > 0
    s0, s1, a = _sources(spec, rate)
    # the angles from the input's bits in `angle_dtype`; a complex64 input widens exactly, float32 angles of a complex128 input
    # would round the input first and are not asked for
    real = torch.float32 if spec.dtype == torch.complex64 else torch.float64
    assert angle_dtype == torch.float64 or real == torch.float32
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
    return torch.complex(m * torch.cos(phi), m * torch.sin(phi))


def pvoc_chain_f32(spec, rate, n_fft, hop):
    """The same definition as a plain float32 op chain (what a complex64 spectrogram gets from the usual torch implementations):
    every operation after the source frames, the running sum included, in float32.  Returns complex64."""
    spec = spec.detach().cpu()
    assert spec.dtype == torch.complex64
    s0, s1, a = _sources(spec, rate)
    a = a.to(torch.float32)
    th0, th1 = torch.angle(s0), torch.angle(s1)
    m = a * s1.abs() + (1 - a) * s0.abs()
    adv = _advance(spec.shape[-2], n_fft, hop).to(torch.float32)
    two_pi = torch.tensor(2 * math.pi, dtype=torch.float32)
    d = th1 - th0 - adv
    d = d - two_pi * torch.round(d / two_pi)
    d = d + adv
    phi = torch.cumsum(torch.cat([th0[..., :1], d[..., :-1]], -1), -1)
    assert phi.dtype == torch.float32
    return torch.polar(m, phi)


def max_err(p, ref):
    """max |P - P_ref| / max |P_ref|, in float64"""
    p, ref = p.detach().cpu().to(torch.complex128), ref.detach().cpu().to(torch.complex128)
    return float((p - ref).abs().max() / ref.abs().max())
