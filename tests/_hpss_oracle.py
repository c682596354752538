"""The definition of hpss (spectrogram_inversion_amd/hpss.py, csrc/kernels_hpss.h) in NumPy float64, on the input's own bits: a
gather through the reflection map, np.median, and the mask formulas.  Arrays are (..., F, T)."""
import numpy as np

TINY = {np.dtype(np.float32): float(np.finfo(np.float32).tiny), np.dtype(np.float64): float(np.finfo(np.float64).tiny)}


def refl(i, n):
    """refl(i, n) = j if j < n else 2 n - 1 - j, j = i mod 2 n (Python's mod), elementwise"""
    j = np.mod(np.asarray(i, dtype=np.int64), 2 * n)
    return np.where(j < n, j, 2 * n - 1 - j)


def magnitude(s):
    """A in float64: the input itself, or sqrt(re^2 + im^2) with every operation in float64"""
    s = np.asarray(s)
    if np.iscomplexobj(s):
        re, im = s.real.astype(np.float64), s.imag.astype(np.float64)
        return np.sqrt(re * re + im * im)
    return s.astype(np.float64)


def _median_last(a, k):
    n = a.shape[-1]
    idx = refl(np.arange(n)[:, None] + np.arange(-(k // 2), k // 2 + 1)[None, :], n)        # (n, k)
    return np.median(a[..., idx], axis=-1)                                                  # (an odd count: an element)


def medians(s, k_h, k_p):
    """(harm, perc) in float64"""
    assert k_h % 2 == 1 and k_p % 2 == 1
    a = magnitude(s)
    harm = _median_last(a, k_h)
    perc = np.swapaxes(_median_last(np.swapaxes(a, -1, -2), k_p), -1, -2)
    return harm, perc


def soft(x, r, power, split, tiny):
    if np.isinf(power):
        return (x > r).astype(np.float64)
    z = np.maximum(x, r)
    small = z < tiny
    zs = np.where(small, 1.0, z)
    qa, qr = x / zs, r / zs
    if power == 1:
        a, b = qa, qr
    elif power == 2:
        a, b = qa * qa, qr * qr
    else:
        a, b = np.power(qa, power), np.power(qr, power)
    den = np.where(small, 1.0, a + b)
    return np.where(small, 0.5 if split else 0.0, a / den)


def masks_of(harm, perc, power=2.0, m_h=1.0, m_p=1.0, real_dtype=np.float64):
    """(M_h, M_p) in float64 from the two medians; `real_dtype` is the real dtype of the input the result stands for (it decides
    `tiny`)"""
    split = m_h == 1 and m_p == 1
    tiny = TINY[np.dtype(real_dtype)]
    return soft(harm, m_h * perc, power, split, tiny), soft(perc, m_p * harm, power, split, tiny)


def masks(s, k_h, k_p, power=2.0, m_h=1.0, m_p=1.0, real_dtype=np.float64):
    return masks_of(*medians(s, k_h, k_p), power, m_h, m_p, real_dtype)


def times(s, mask):
    """S * M in float64 / complex128: each part of S times the float64 mask"""
    s = np.asarray(s)
    if np.iscomplexobj(s):
        return (s.real.astype(np.float64) * mask) + 1j * (s.imag.astype(np.float64) * mask)
    return s.astype(np.float64) * mask
