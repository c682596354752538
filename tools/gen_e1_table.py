#!/usr/bin/env python
"""Writes spectrogram_inversion_amd/csrc/enhance_e1_table.h: the coefficients with which k_enhance evaluates the exponential
integral E1.  Needs mpmath; the header is committed, so a build does not.

    python tools/gen_e1_table.py [--check]

Scheme.  v <= 1:  E1(v) = -gamma - ln v + sum_{k=1}^{K} c_k v^k,  c_k = (-1)^(k+1) / (k k!), K = 18 (the first term left out is
below 4.3e-19).  1 < v <= 1024:  E1(v) = exp(-v) / v * R(v), R(v) = v e^v E1(v) in [0.596, 1); on each octave [2^j, 2^(j+1)),
j = 0 ... 6, and on [128, 1024] R is a Chebyshev sum of degree D in x = (2 / v - (1/a + 1/b)) / (1/a - 1/b), the interval [a, b]
mapped through 1 / v onto [-1, 1].  The coefficients are the interpolant at D + 1 Chebyshev nodes of 50-digit values.
--check prints the largest relative error of the float64 evaluation of the scheme against 50-digit values on a dense grid.
"""
import os
import sys

import mpmath as mp
import numpy as np

mp.mp.dps = 50
K_SERIES = 18
DEGREE = 15
EDGES = [1, 2, 4, 8, 16, 32, 64, 128, 1024]
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "spectrogram_inversion_amd", "csrc", "enhance_e1_table.h")


def ratio(v):
    v = mp.mpf(v)
    return v * mp.exp(v) * mp.e1(v)


def cheb_coeffs(a, b, deg):
    n = deg + 1
    ia, ib = 1 / mp.mpf(a), 1 / mp.mpf(b)
    nodes = [mp.cos(mp.pi * (k + mp.mpf(1) / 2) / n) for k in range(n)]
    vals = [ratio(2 / (x * (ia - ib) + (ia + ib))) for x in nodes]
    out = []
    for j in range(n):
        s = sum(vals[k] * mp.cos(mp.pi * j * (k + mp.mpf(1) / 2) / n) for k in range(n)) * 2 / n
        out.append(s / 2 if j == 0 else s)
    return [float(c) for c in out]


def series_coeffs():
    return [float(mp.mpf((-1) ** (k + 1)) / (k * mp.factorial(k))) for k in range(1, K_SERIES + 1)]


def interval_maps():
    """per interval [a, b]: 1/a + 1/b and 1 / (1/a - 1/b), so that x = (2 / v - mid) * scale"""
    mid = [1.0 / a + 1.0 / b for a, b in zip(EDGES[:-1], EDGES[1:])]
    scale = [1.0 / (1.0 / a - 1.0 / b) for a, b in zip(EDGES[:-1], EDGES[1:])]
    return mid, scale


def evaluate(v, series, tables):
    """the scheme in float64, operation for operation as the kernel runs it"""
    v = np.asarray(v, dtype=np.float64)
    out = np.zeros_like(v)
    lo = v <= 1.0
    x = v[lo]
    s = np.full_like(x, series[-1])
    for c in series[-2::-1]:
        s = s * x + c
    out[lo] = (s * x - np.log(x)) - 0.57721566490153286061
    hi = ~lo & (v <= 1024.0)
    x = v[hi]
    j = np.minimum(np.frexp(x)[1] - 1, len(tables) - 1)
    mid, scale = interval_maps()
    rv = 1.0 / x
    t = (2.0 * rv - np.asarray(mid)[j]) * np.asarray(scale)[j]
    tab = np.asarray(tables)[j]                     # (n, D + 1)
    b1 = np.zeros_like(x)
    b2 = np.zeros_like(x)
    for k in range(tab.shape[1] - 1, 0, -1):
        b1, b2 = tab[:, k] + (2.0 * t * b1 - b2), b1
    r = tab[:, 0] + (t * b1 - b2)
    out[hi] = np.exp(-x) * rv * r
    return out


def main():
    series = series_coeffs()
    tables = [cheb_coeffs(a, b, DEGREE) for a, b in zip(EDGES[:-1], EDGES[1:])]
    if "--check" in sys.argv:
        grid = np.concatenate([np.logspace(-12, 0, 1500), np.logspace(0, np.log10(1024.0), 6000)[1:],
                               np.nextafter(np.asarray(EDGES[1:-1], dtype=np.float64), 0), np.asarray(EDGES, dtype=np.float64)])
        got = evaluate(grid, series, tables)
        worst = 0.0
        for g, y in zip(grid, got):
            if g > 700:
                continue
            ref = mp.e1(mp.mpf(float(g)))
            worst = max(worst, float(abs(mp.mpf(float(y)) - ref) / ref))
        print(f"largest relative error on [1e-12, 700]: {worst:.3e}; last coefficients "
              f"{max(abs(t[-1]) for t in tables):.2e}")
        return
    lines = ["// Written by tools/gen_e1_table.py: do not edit.  E1 for k_enhance (DESIGN 3.30): the series' coefficients",
             "// (-1)^(k+1) / (k k!), k = 1 ... kE1Series, and per interval of v the Chebyshev coefficients of v e^v E1(v) in 1 / v.",
             "#pragma once", "", "namespace specinv {", "",
             f"constexpr int kE1Series = {K_SERIES};", f"constexpr int kE1Degree = {DEGREE};",
             f"constexpr int kE1Intervals = {len(tables)};", "",
             "__device__ constexpr double kE1SeriesCoef[kE1Series] = {"]
    lines += [f"    {c!r}," for c in series]
    mid, scale = interval_maps()
    lines += ["};", "", "// the intervals [a, b) = [1, 2), [2, 4), ... [64, 128), [128, 1024]: x = (2 / v - kE1Mid) * kE1Scale with",
              "// kE1Mid = 1 / a + 1 / b and kE1Scale = 1 / (1 / a - 1 / b)",
              "__device__ constexpr double kE1Mid[kE1Intervals] = {" + ", ".join(repr(m) for m in mid) + "};",
              "__device__ constexpr double kE1Scale[kE1Intervals] = {" + ", ".join(repr(m) for m in scale) + "};", "",
              "__device__ constexpr double kE1Cheb[kE1Intervals][kE1Degree + 1] = {"]
    for t in tables:
        lines.append("    {" + ", ".join(repr(c) for c in t) + "},")
    lines += ["};", "", "}  // namespace specinv", ""]
    with open(OUT, "w") as fh:
        fh.write("\n".join(lines))
    print(os.path.normpath(OUT))


if __name__ == "__main__":
    main()
