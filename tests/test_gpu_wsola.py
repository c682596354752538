"""wsola and ola on the device against the definition in NumPy float64 (tests/_wsola_oracle.py) on the input's own bits.

Inputs are three sinusoids plus noise at 0.1, seeded.  k_wsola_lags gives a lane 9 consecutive lags and cuts the n axis into
slices of a multiple of 9; none of N, Hs, 2 D + 1 below is a multiple of 9, so every case has a ragged last lag group and a ragged
last slice, 64 / 32 / 96 has more lags than n, 2048 / 2048 / 1024 is the largest region the kernel stages and the only case with
fewer than two slices to spare, and 128 / 64 / 64 on 40 samples clips every read.

Bounds (none measured into being):
  lags: exact.  Two orders of summation of the N products of one c[d] differ by at most (N - 1) 2^-53 G each (G the sum of the
    products' magnitudes, first order), the kernel's fmas round once where the oracle rounds twice: under 2 N 2^-53 G per value,
    4 N 2^-53 G for a difference of two.  Each case first asserts on the oracle alone that the largest c leads the runner-up by more
    than that at every step, so that the arg-max does not depend on the order.  A step with G = 0 (both operands silent: the
    frames past the input's end) has every product zero in any order, c = 0 exactly and the tie rule decides: it needs no margin.
  output, against ola_given_lags on the kernel's own lags: |y - ref| <= (2 K + 4) 2^-53 S[j], K = ceil(N / Hs) + 1 the most
    frames a sample has (K products, K - 1 additions of acc, K - 1 of ow, one quotient, and slack), plus the one rounding to
    the output dtype: 2^-24 |ref| for float32; 2^-24 |ref| and the half's own unit roundoff (2^-11 float16, 2^-8 bfloat16) for the
    halves, which are computed as float32 and rounded twice.
"""
import math

import numpy as np
import pytest
import torch

import spectrogram_inversion_amd as si
from _wsola_oracle import centres, correlation, n_frames, ola_given_lags, out_length, wsola_ref

pytestmark = pytest.mark.gpu

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
DEV = "cuda"
NAME = {F16: "f16", BF16: "bf16", F32: "f32", F64: "f64"}
ROUND = {F64: 0.0, F32: 2.0 ** -24, F16: 2.0 ** -24 + 2.0 ** -11, BF16: 2.0 ** -24 + 2.0 ** -8}
RATES = (0.5, 0.8, 1.0, 1.25, 2.0)

# name -> (N, Hs, D, L, B, seed)
CASES = {"main": (64, 32, 16, 600, 3, 1), "overlap4": (256, 64, 0, 3000, 2, 2), "tol_above_n": (64, 32, 96, 800, 2, 3),
         "hop_is_n": (64, 64, 8, 500, 2, 4), "clipped": (128, 64, 64, 40, 1, 5), "limits": (2048, 2048, 1024, 12000, 1, 6)}


def signal(B, L, seed, dtype):
    """(B, L) CPU tensor of `dtype`: per item three sinusoids of seeded frequency and phase plus noise at 0.1"""
    rng = np.random.default_rng(seed)
    t = np.arange(L)
    rows = []
    for _ in range(B):
        f = rng.uniform(0.02, 1.5, 3)
        ph = rng.uniform(0, 2 * np.pi, 3)
        rows.append(sum(a * np.sin(f[i] * t + ph[i]) for i, a in enumerate((1.0, 0.5, 0.25))) + 0.1 * rng.standard_normal(L))
    return torch.from_numpy(np.stack(rows)).to(dtype)


def window_of(N, dtype):
    work = F64 if dtype == F64 else F32
    return torch.hann_window(N, dtype=work).double().numpy()


_REFS = {}


def reference(case, dtype, rate, length=None):
    """(x (B, L) CPU tensor, [wsola_ref(item) ...]) of a case, computed once"""
    key = (case, dtype, rate, length)
    if key not in _REFS:
        N, Hs, D, L, B, seed = CASES[case]
        x = signal(B, L, seed, dtype)
        refs = [wsola_ref(row.double().numpy(), rate, N, Hs, D, window_of(N, dtype), length, fast=N > 256) for row in x]
        _REFS[key] = (x, refs)
    return _REFS[key]


def margins_hold(refs, N):
    for _, _, _, margins in refs:
        ok = (margins[:, 0] > 4 * N * 2.0 ** -53 * margins[:, 1]) | (margins[:, 1] == 0)
        assert ok.all(), np.flatnonzero(~ok)


def check_output(y, x_row, lags, rate, N, Hs, dtype, length=None):
    """one item: y (n_out,) tensor against the overlap-add of the definition with the kernel's own lags"""
    work = x_row.double().numpy()
    ref, S = ola_given_lags(work, lags, rate, N, Hs, window_of(N, dtype), length, with_scale=True)
    K = math.ceil(N / Hs) + 1
    bound = (2 * K + 4) * 2.0 ** -53 * S + ROUND[dtype] * np.abs(ref)
    err = np.abs(y.double().cpu().numpy() - ref)
    assert y.shape == ref.shape and (err <= bound).all(), (int(np.argmax(err - bound)), float((err - bound).max()))


def run_case(case, dtype, rate, length=None, unbatched=False):
    N, Hs, D, L, B, _ = CASES[case]
    x, refs = reference(case, dtype, rate, length)
    margins_hold(refs, N)
    xin = x[0] if unbatched else x
    y, lags = si.wsola(xin.to(DEV), rate, N, Hs, D, length=length, return_lags=True)
    n_out = out_length(L, rate, length)
    M = n_frames(n_out, N, Hs)
    assert y.dtype == dtype and y.device.type == "cuda" and lags.dtype == torch.int32
    assert y.shape == xin.shape[:-1] + (n_out,) and lags.shape == xin.shape[:-1] + (M,)       # no frame is left out
    y2, l2 = y.reshape(-1, n_out).cpu(), lags.reshape(-1, M).cpu().numpy()
    for b in range(y2.shape[0]):
        assert np.array_equal(l2[b], refs[b][1]), (b, np.flatnonzero(l2[b] != refs[b][1]))
        check_output(y2[b], x[b], l2[b], rate, N, Hs, dtype, length)
    return y, lags


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("dtype", (F32, F64), ids=NAME.get)
def test_main_sweep(dtype, rate):
    _, lags = run_case("main", dtype, rate)
    if rate != 1.0:
        assert lags.any()                                           # (the search does something)


@pytest.mark.parametrize("case,rate", (("overlap4", 0.8), ("tol_above_n", 1.25), ("hop_is_n", 0.8), ("clipped", 0.5), ("limits", 0.8)))
@pytest.mark.parametrize("dtype", (F32, F64), ids=NAME.get)
def test_shapes(dtype, case, rate):
    run_case(case, dtype, rate)


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("dtype", (F32, F64), ids=NAME.get)
def test_unbatched(dtype, rate):
    run_case("main", dtype, rate, unbatched=True)


@pytest.mark.parametrize("length", (1, 255, 256, 257, "past"))
@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("dtype", (F32, F64), ids=NAME.get)
def test_explicit_length(dtype, rate, length):
    if length == "past":
        length = out_length(600, rate) + 500                        # the last frames lie past the input's end
    run_case("main", dtype, rate, length=length)


@pytest.mark.parametrize("dtype", (F16, BF16), ids=NAME.get)
def test_halves_are_float32_rounded_back(dtype):
    N, Hs, D, L, B, seed = CASES["main"]
    x = signal(B, L, seed, dtype)
    y, lags = si.wsola(x.to(DEV), 0.8, N, Hs, D, return_lags=True)
    y32, lags32 = si.wsola(x.float().to(DEV), 0.8, N, Hs, D, return_lags=True)
    assert y.dtype == dtype and torch.equal(lags, lags32) and torch.equal(y, y32.to(dtype))
    for b in range(B):
        check_output(y[b].cpu(), x[b], lags[b].cpu().numpy(), 0.8, N, Hs, dtype)


@pytest.mark.parametrize("dtype", (F32, F64), ids=NAME.get)
def test_a_tie_prone_input_is_checked_by_optimality(dtype):
    """a sinusoid of period 16: c[d] and c[d +- 16] are equal up to rounding wherever no read is clipped, so the lags are not pinned;
    with the kernel's own del_m, the oracle's c at the kernel's del_{m+1} is within 4 N 2^-53 G[m] of the oracle's maximum"""
    N, Hs, D, L, rate = 64, 32, 16, 600, 0.8
    x = torch.sin(2 * np.pi * torch.arange(L, dtype=F64) / 16).to(dtype)
    y, lags = si.wsola(x.to(DEV), rate, N, Hs, D, return_lags=True)
    lags = lags.cpu().numpy()
    work = x.double().numpy()
    M = n_frames(out_length(L, rate), N, Hs)
    a = centres(M, Hs, rate)
    assert lags.shape == (M,) and lags[0] == 0 and (np.abs(lags) <= D).all()
    for m in range(M - 1):
        c, g = correlation(work, a[m + 1], a[m] + int(lags[m]) - N // 2, N, Hs, D)
        assert c.max() - c[lags[m + 1] + D] <= 4 * N * 2.0 ** -53 * g.max(), m
    check_output(y.cpu(), x, lags, rate, N, Hs, dtype)


@pytest.mark.parametrize("dtype", (F32, F64), ids=NAME.get)
def test_silence_is_exact(dtype):
    y, lags = si.wsola(torch.zeros(2, 600, dtype=dtype, device=DEV), 0.8, 64, 32, 16, return_lags=True)
    assert not lags.any() and torch.equal(y, torch.zeros(2, 750, dtype=dtype, device=DEV))
    assert not torch.signbit(y).any()
    # 300 zeros, then signal: the lag is 0 while both operands are silent
    N, Hs, D, rate = 64, 32, 16, 0.8
    x = torch.cat([torch.zeros(2, 300, dtype=dtype), signal(2, 300, 7, dtype)], dim=1)
    y, lags = si.wsola(x.to(DEV), rate, N, Hs, D, return_lags=True)
    lags = lags.cpu().numpy()
    M = lags.shape[-1]
    a = centres(M, Hs, rate)
    # step m reads p from a_m + del_m - N/2 + Hs ... + N and the region up to a_{m+1} + N/2 + D: silent while that ends by 300
    silent = [m + 1 for m in range(M - 1) if a[m] + D + Hs + N // 2 <= 300 or a[m + 1] + N // 2 + D <= 300]
    assert len(silent) >= 5 and not lags[:, silent].any() and lags.any()
    for b in range(2):
        check_output(y[b].cpu(), x[b], lags[b], rate, N, Hs, dtype)


@pytest.mark.parametrize("dtype", (F32, F64), ids=NAME.get)
def test_ola_is_wsola_without_a_search(dtype):
    x = signal(2, 3000, 8, dtype).to(DEV)
    for N, Hs in ((256, None), (256, 64), (64, 64)):
        y, lags = si.wsola(x, 0.8, N, Hs, 0, return_lags=True)
        assert not lags.any() and lags.shape == (2, n_frames(3750, N, Hs or N // 2))
        assert torch.equal(si.ola(x, 0.8, N, Hs), y)
    assert torch.equal(si.ola(x, 0.8), si.wsola(x, 0.8, 256, tolerance=0))


@pytest.mark.parametrize("dtype", (F32, F64), ids=NAME.get)
def test_rate_one_without_a_search_returns_the_input(dtype):
    """Hann at Hs = N/2: ow = 1 up to rounding and every frame reads its own position, so S = |x| and the output bound is on x"""
    x = signal(2, 1000, 9, dtype)
    y = si.ola(x.to(DEV), 1.0, 64).cpu()
    K = 3
    bound = ((2 * K + 4) * 2.0 ** -53 * (1 + 2.0 ** -50) + ROUND[dtype]) * x.double().abs()
    assert y.shape == x.shape and ((y.double() - x.double()).abs() <= bound).all()
    for b in range(2):
        check_output(y[b], x[b], np.zeros(n_frames(1000, 64, 32), dtype=np.int64), 1.0, 64, 32, dtype)


def test_a_side_stream_and_a_cpu_input():
    x, refs = reference("main", F32, 0.8)
    N, Hs, D = CASES["main"][:3]
    want_y, want_l = si.wsola(x.to(DEV), 0.8, N, Hs, D, return_lags=True)
    stream = torch.cuda.Stream()
    xd = x.to(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        y, lags = si.wsola(xd, 0.8, N, Hs, D, return_lags=True)
    stream.synchronize()
    assert torch.equal(y, want_y) and torch.equal(lags, want_l)
    y, lags = si.wsola(x, 0.8, N, Hs, D, return_lags=True)
    assert y.device.type == "cpu" and lags.device.type == "cpu"
    assert torch.equal(y, want_y.cpu()) and torch.equal(lags, want_l.cpu())
    assert torch.equal(si.wsola(xd, 0.8, N, Hs, D, window=torch.hann_window(N)), want_y)      # the default window
    w64 = torch.hann_window(N, dtype=F64).sqrt()                    # an explicit window is rounded to the dtype computed in
    y = si.wsola(xd, 0.8, N, Hs, D, window=w64)
    assert torch.equal(y, si.wsola(xd, 0.8, N, Hs, D, window=w64.float().to(DEV))) and not torch.equal(y, want_y)
