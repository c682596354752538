"""Sample-rate conversion written out twice, without the package (tests only).

`resample_ref` is the definition of `si.resample` in vectorised NumPy float64 with an exact integer d; `resample_bank` is
torchaudio's algorithm (`sinc_interp_hann`: a bank of `new` filters, a padded conv1d of stride `orig`) restated in torch on the CPU,
float64 by default.  The two agree to 3e-13 of max |y| (tests/test_resample_host.py)."""
import math

import numpy as np
import torch


def reduced(orig_freq, new_freq):
    g = math.gcd(int(orig_freq), int(new_freq))
    return int(orig_freq) // g, int(new_freq) // g


def length_out(n_in, orig_freq, new_freq):
    """ceil(n L / o) in integer arithmetic"""
    o, n = reduced(orig_freq, new_freq)
    return -((-n * int(n_in)) // o)


def taps(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """K = 2 ceil(W o / base) + 1: the most inputs an output reads"""
    o, n = reduced(orig_freq, new_freq)
    return 2 * math.ceil(lowpass_filter_width * o / (min(o, n) * rolloff)) + 1


def gain(orig_freq, new_freq, rolloff=0.99):
    """base / o: the factor in front of the sum"""
    o, n = reduced(orig_freq, new_freq)
    return min(o, n) * rolloff / o


def resample_ref(x, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99):
    """x (L,) / (B, L), any real array -> float64 (L_out,) / (B, L_out):
        y[m] = (base / o) sum_{|tau| < W} sinc(tau) cos^2(pi tau / (2 W)) x[s],  tau = base d / (o n),  d = s n - m o."""
    x = np.asarray(x, dtype=np.float64)
    o, n = reduced(orig_freq, new_freq)
    W = int(lowpass_filter_width)
    base = min(o, n) * float(rolloff)
    L = x.shape[-1]
    n_out = length_out(L, o, n)
    half = math.ceil(W * o / base) + 1
    m = np.arange(n_out, dtype=np.int64)
    c = (m * o) // n                                            # floor(m o / n)
    s = c[:, None] + np.arange(-half, half + 1, dtype=np.int64)[None, :]      # (n_out, taps)
    d = s * n - (m * o)[:, None]                                # exact: int64
    tau = base * d.astype(np.float64) / float(o * n)
    w = np.sinc(tau) * np.cos(np.pi * tau / (2 * W)) ** 2       # np.sinc(t) = sin(pi t) / (pi t), 1 at 0
    w = np.where((np.abs(tau) < W) & (s >= 0) & (s < L), w, 0.0)
    xs = x[..., np.clip(s, 0, max(L - 1, 0))] if L else np.zeros(x.shape[:-1] + s.shape)
    return (base / o) * np.einsum("...mk,mk->...m", xs, w)


def resample_bank(x, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, dtype=torch.float64, kernel=None):
    """torchaudio.functional.resample's computation: x (B, L) torch tensor -> (B, L_out) of `dtype`, on x's device.
    `kernel` takes a bank made by `bank_kernel` (what torchaudio.transforms.Resample keeps between calls)."""
    o, n = reduced(orig_freq, new_freq)
    if kernel is None:
        kernel = bank_kernel(o, n, lowpass_filter_width, rolloff, dtype, x.device)
    width = (kernel.shape[-1] - o) // 2
    xp = torch.nn.functional.pad(x.to(dtype)[:, None], (width, width + o))
    y = torch.nn.functional.conv1d(xp, kernel, stride=o).transpose(1, 2).reshape(x.shape[0], -1)
    return y[..., :length_out(x.shape[-1], o, n)]


def bank_kernel(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, dtype=torch.float64, device="cpu"):
    """the (n, 1, 2 width + o) filter bank of torchaudio's _get_sinc_resample_kernel, built in float64 and rounded to `dtype`"""
    o, n = reduced(orig_freq, new_freq)
    W = int(lowpass_filter_width)
    base = min(o, n) * float(rolloff)
    width = math.ceil(W * o / base)
    idx = torch.arange(-width, width + o, dtype=torch.float64, device=device)[None, None] / o
    t = torch.arange(0, -n, -1, dtype=torch.float64, device=device)[:, None, None] / n + idx
    t = (t * base).clamp(-W, W)
    win = torch.cos(t * math.pi / W / 2) ** 2
    t = t * math.pi
    k = torch.where(t == 0, torch.ones((), dtype=torch.float64, device=device), t.sin() / t) * win * (base / o)
    return k.to(dtype)
