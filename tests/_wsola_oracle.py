"""The definition of wsola (spectrogram_inversion_amd/tsm.py, csrc/kernels_wsola.h) in NumPy float64 on the input's own bits: a
frame loop with explicit sums and the tie rule.  One item at a time: x is (L,).  `second_form` is the same definition written the
other way round (per output sample instead of per frame, the correlation as a matrix of shifted rows), for the oracle's own test."""
import math

import numpy as np


def n_frames(n_out, N, Hs):
    return (n_out - 1 + N // 2) // Hs + 1


def centres(M, Hs, rate):
    return np.floor(np.arange(M) * Hs * rate + 0.5).astype(np.int64)


def out_length(L, rate, length=None):
    return int(length) if length is not None else max(1, math.ceil(L / rate))


def xz(x, idx):
    """x[idx] where 0 <= idx < L, else 0, elementwise, in float64"""
    idx = np.asarray(idx, dtype=np.int64)
    ok = (idx >= 0) & (idx < len(x))
    out = np.zeros(idx.shape, dtype=np.float64)
    out[ok] = np.asarray(x, dtype=np.float64)[idx[ok]]
    return out


def pick(c, D):
    """the lag of the largest c[d + D]; among equals the smallest |d|; of +-d the negative one"""
    best = -D
    for d in range(-D, D + 1):
        v, b = c[d + D], c[best + D]
        if v > b or (v == b and (abs(d) < abs(best) or (abs(d) == abs(best) and d < best))):
            best = d
    return best


def correlation(x, a_next, u, N, Hs, D):
    """(c, g): c[d + D] = sum_n xz(a_next - N/2 + d + n) p[n] and g[d + D] the same sum of absolute values, p[n] = xz(u + Hs + n)"""
    n = np.arange(N)
    p = xz(x, u + Hs + n)
    c, g = np.zeros(2 * D + 1), np.zeros(2 * D + 1)
    for d in range(-D, D + 1):
        prod = xz(x, a_next - N // 2 + d + n) * p
        s = t = 0.0
        for v in prod:                      # explicit sums, in order
            s += v
            t += abs(v)
        c[d + D], g[d + D] = s, t
    return c, g


def _fast_correlation(x, a_next, u, N, Hs, D):
    """correlation() with the inner sums by np.sum (pairwise): for the large shapes, where the explicit loop takes minutes; the
    two differ by the summation order only, which the margin test covers"""
    n = np.arange(N)
    p = xz(x, u + Hs + n)
    rows = xz(x, a_next - N // 2 + np.arange(-D, D + 1)[:, None] + n[None, :]) * p[None, :]
    return rows.sum(axis=1), np.abs(rows).sum(axis=1)


def ola_given_lags(x, lags, rate, N, Hs, w, length=None, with_scale=False):
    """y (n_out,) in float64 for given lags (M,); with_scale: (y, S), S[j] = sum_m |w[n] xz(...)| / divisor"""
    x = np.asarray(x)
    w = np.asarray(w, dtype=np.float64)
    n_out = out_length(len(x), rate, length)
    M = n_frames(n_out, N, Hs)
    assert len(lags) == M, (len(lags), M)
    a = centres(M, Hs, rate)
    acc, ow, sc = np.zeros(n_out), np.zeros(n_out), np.zeros(n_out)
    n = np.arange(N)
    for m in range(M):                                          # ascending m: each acc[j] takes its frames in that order
        j = m * Hs - N // 2 + n
        ok = (j >= 0) & (j < n_out)
        term = w * xz(x, a[m] + int(lags[m]) - N // 2 + n)
        acc[j[ok]] += term[ok]
        sc[j[ok]] += np.abs(term[ok])
        ow[j[ok]] += w[ok]
    div = np.where(ow >= 1e-3, ow, 1.0)
    return (acc / div, sc / np.abs(div)) if with_scale else acc / div


def wsola_ref(x, rate, N, Hs, D, w, length=None, fast=False):
    """(y, lags, S, margins): y float64 (n_out,), lags int64 (M,), S the output scale, and margins (M - 1, 2), per step
    m = 0 ... M - 2 the largest c minus the runner-up next to G[m] = max_d sum_n |xz(...) p[n]| (zeros for D = 0: no step is run)"""
    x = np.asarray(x)
    n_out = out_length(len(x), rate, length)
    M = n_frames(n_out, N, Hs)
    a = centres(M, Hs, rate)
    lags = np.zeros(M, dtype=np.int64)
    margins, G = np.zeros(M - 1), np.zeros(M - 1)
    if D > 0:
        corr = _fast_correlation if fast else correlation
        for m in range(M - 1):
            u = a[m] + lags[m] - N // 2
            c, g = corr(x, a[m + 1], u, N, Hs, D)
            lags[m + 1] = pick(c, D)
            top = np.sort(c)
            margins[m] = top[-1] - top[-2]
            G[m] = g.max()
    y, S = ola_given_lags(x, lags, rate, N, Hs, w, length, with_scale=True)
    return y, lags, S, np.stack([margins, G], axis=1)


def second_form(x, rate, N, Hs, D, w, length=None):
    """(y, lags) once more, independently: the correlation by np.dot over a zero-padded copy, the overlap-add per output sample"""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    L = len(x)
    n_out = out_length(L, rate, length)
    M = 0
    while M * Hs - N // 2 < n_out:                              # frames whose support starts before the output ends
        M += 1
    a = [int(math.floor(m * Hs * rate + 0.5)) for m in range(M)]
    pad = 2 * N + 2 * D + Hs + max(0, max(a) - L) + 8
    xp = np.concatenate([np.zeros(pad), x, np.zeros(pad)])      # xp[pad + i] = xz(i) wherever it is read

    lags = [0]
    for m in range(M - 1):
        if D == 0:
            lags.append(0)
            continue
        start = pad + a[m] + lags[m] - N // 2 + Hs
        p = xp[start:start + N]
        best, best_c = None, None
        for mag in range(D + 1):                                # by growing |d|, the negative first: a later one must be larger
            for d in ((0,) if mag == 0 else (-mag, mag)):
                s0 = pad + a[m + 1] - N // 2 + d
                c = float(np.dot(xp[s0:s0 + N], p))
                if best is None or c > best_c:
                    best, best_c = d, c
        lags.append(best)
    y = np.zeros(n_out)
    for j in range(n_out):
        acc = ow = 0.0
        for m in range(M):
            n = j - m * Hs + N // 2
            if 0 <= n < N:
                acc += w[n] * xp[pad + a[m] + lags[m] - N // 2 + n]
                ow += w[n]
        y[j] = acc / (ow if ow >= 1e-3 else 1.0)
    return y, np.array(lags, dtype=np.int64)
