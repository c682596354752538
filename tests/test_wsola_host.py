"""wsola, ola and time_stretch_hpss without a GPU: the definition (tests/_wsola_oracle.py) against its own properties and a second
form, the frame count and the centres worked by hand, and the argument errors of the three functions and of specinv_wsola, all
raised before the device is touched."""
import ctypes as C

import numpy as np
import pytest
import torch

import spectrogram_inversion_amd as si
from _wsola_oracle import centres, n_frames, ola_given_lags, second_form, wsola_ref
from spectrogram_inversion_amd import _lib, build, tsm


def _hann(n):
    return torch.hann_window(n, dtype=torch.float64).numpy()


def _signal(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return (np.sin(0.05 * t) + 0.5 * np.sin(0.31 * t + 1) + 0.25 * np.sin(1.3 * t + 2) + 0.1 * rng.standard_normal(n))


def test_oracle_at_rate_one_without_a_search_returns_the_input():
    """Hann at Hs = N/2 sums to one (w[n] + w[n + N/2] = 1 up to rounding) and every frame reads its own position: y = x[:n_out]
    to 4 * 2^-52 |x| (two products, one sum and one quotient by 1 +- 2^-52)"""
    x = _signal(700, 0)
    for n_out in (700, 333):
        y, lags, S, _ = wsola_ref(x, 1.0, 64, 32, 0, _hann(64), n_out)
        assert not lags.any()
        assert (np.abs(y - x[:n_out]) <= 4 * 2.0 ** -52 * np.abs(x[:n_out])).all()
        assert (np.abs(S - np.abs(x[:n_out])) <= 4 * 2.0 ** -52 * np.abs(x[:n_out])).all()


def test_oracle_on_silence_keeps_every_lag_at_zero():
    y, lags, S, margins = wsola_ref(np.zeros(500), 0.8, 64, 32, 16, _hann(64))
    assert not lags.any() and not y.any() and not S.any() and not margins.any()
    assert len(y) == 625 and len(lags) == n_frames(625, 64, 32)


@pytest.mark.parametrize("shape", ((300, 0.8, 32, 16, 8, None), (260, 1.3, 48, 12, 20, 333), (200, 0.7, 16, 16, 0, None)), ids=str)
def test_oracle_against_a_second_form(shape):
    L, rate, N, Hs, D, length = shape
    x = _signal(L, L)
    w = _hann(N)
    y, lags, _, margins = wsola_ref(x, rate, N, Hs, D, w, length)
    if D:
        # np.dot sums in another order; past the input's end (length 333) both operands are silent, c = 0 in any order
        assert ((margins[:, 0] > 4 * N * 2.0 ** -53 * margins[:, 1]) | (margins[:, 1] == 0)).all()
        assert (margins[:, 1] > 0).sum() >= 10
    y2, lags2 = second_form(x, rate, N, Hs, D, w, length)
    assert np.array_equal(lags, lags2)
    assert np.abs(y - y2).max() <= 16 * 2.0 ** -52 * np.abs(x).max()
    assert np.array_equal(ola_given_lags(x, lags, rate, N, Hs, w, length), y)


def test_the_tie_rule():
    from _wsola_oracle import pick
    assert pick(np.array([1.0, 1.0, 1.0, 1.0, 1.0]), 2) == 0
    assert pick(np.array([2.0, 1.0, 0.0, 1.0, 2.0]), 2) == -2
    assert pick(np.array([2.0, 3.0, 0.0, 3.0, 2.0]), 2) == -1
    assert pick(np.array([0.0, 0.0, 0.0, 3.0, 3.0]), 2) == 1


def test_frame_count_and_centres_by_hand():
    # frame m covers [m Hs - N/2, m Hs + N/2)
    assert n_frames(1, 64, 32) == 2                     # [-32, 32) and [0, 64); [32, 96) starts beyond sample 0
    assert n_frames(600, 64, 32) == 20                  # 19 * 32 - 32 = 576 < 600 <= 20 * 32 - 32
    assert n_frames(256, 256, 64) == 6                  # 5 * 64 - 128 = 192 < 256 <= 6 * 64 - 128
    assert n_frames(500, 64, 64) == 9                   # 8 * 64 - 32 = 480 < 500 <= 9 * 64 - 32
    assert n_frames(32, 64, 32) == 2 and n_frames(33, 64, 32) == 3
    for n_out, N, Hs in ((1, 64, 32), (600, 64, 32), (256, 256, 64), (500, 64, 64), (33, 64, 32)):
        assert tsm.wsola_frames(n_out, N, Hs) == n_frames(n_out, N, Hs)
    assert centres(5, 32, 0.8).tolist() == [0, 26, 51, 77, 102]          # 25.6 m + 0.5: 0.5, 26.1, 51.7, 77.3, 102.9
    assert centres(3, 32, 1.25).tolist() == [0, 40, 80]
    assert centres(5, 3, 0.5).tolist() == [0, 2, 3, 5, 6]                # 1.5 m + 0.5: 0.5, 2.0, 3.5, 5.0, 6.5
    for M, Hs, rate in ((5, 32, 0.8), (3, 32, 1.25), (5, 3, 0.5), (40, 512, 1.0 / 3)):
        got = tsm.wsola_centres(M, Hs, rate)
        assert got.dtype == np.int64 and np.array_equal(got, centres(M, Hs, rate))


X = torch.zeros(2, 600)
KW = dict(n_fft=128, hop_length=32, window=torch.hann_window(128))


def test_argument_errors_come_before_the_device():
    for bad in (dict(frame_length=0), dict(frame_length=63), dict(frame_length=2050), dict(frame_length=4096), dict(frame_length=64.0),
                dict(frame_length=True), dict(frame_length=None), dict(frame_length=-64),
                dict(frame_length=64, hop_length=0), dict(frame_length=64, hop_length=65), dict(frame_length=64, hop_length=32.0),
                dict(frame_length=64, hop_length=True),
                dict(frame_length=64, window=torch.ones(63)), dict(frame_length=64, window=torch.ones(2, 64)),
                dict(length=0), dict(length=-5), dict(length=10.0), dict(length=True)):
        for fn in (si.wsola, si.ola):
            with pytest.raises(ValueError):
                fn(X, 0.8, **bad)
    for bad in (dict(tolerance=-1), dict(tolerance=1025), dict(tolerance=8.0), dict(tolerance=True)):
        with pytest.raises(ValueError):
            si.wsola(X, 0.8, 64, **bad)
    for rate in (0, 0.0, -1.0, float("nan"), float("inf"), "1", None, True):
        for call in (lambda: si.wsola(X, rate), lambda: si.ola(X, rate), lambda: si.time_stretch_hpss(X, rate, **KW)):
            with pytest.raises(ValueError):
                call()
    for x in (torch.zeros(2, 2, 600), torch.zeros(()), torch.zeros(3, 0)):
        for fn in (si.wsola, si.ola):
            with pytest.raises(ValueError):
                fn(x, 0.8)
    with pytest.raises(ValueError):
        si.time_stretch_hpss(torch.zeros(2, 2, 2, 600), 0.8, **KW)
    for x in (np.zeros((2, 600)), torch.zeros(2, 600, dtype=torch.int32), torch.zeros(2, 600, dtype=torch.complex64)):
        for call in (lambda: si.wsola(x, 0.8), lambda: si.ola(x, 0.8), lambda: si.time_stretch_hpss(x, 0.8, **KW)):
            with pytest.raises(TypeError):
                call()
    for window in (np.ones(64), [1.0] * 64, torch.ones(64, dtype=torch.int64), torch.ones(64, dtype=torch.complex64)):
        for fn in (si.wsola, si.ola):
            with pytest.raises(TypeError):
                fn(X, 0.8, 64, window=window)
    g = torch.zeros(2, 600, requires_grad=True)
    for name, call in (("wsola", lambda: si.wsola(g, 0.8)), ("ola", lambda: si.ola(g, 0.8)),
                       ("time_stretch_hpss", lambda: si.time_stretch_hpss(g, 0.8, **KW))):
        with pytest.raises(NotImplementedError, match=f"{name} is not differentiable; detach the input"):
            call()
    with torch.no_grad():                                # (without grad mode the flag is not an error: the device is asked for)
        if not torch.cuda.is_available():
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                si.ola(g, 0.8)


def test_time_stretch_hpss_argument_errors_come_before_the_device():
    with pytest.raises(ValueError, match="center"):
        si.time_stretch_hpss(X, 0.8, center=False, **KW)
    for bad in (dict(perc_frame=0), dict(perc_frame=255), dict(perc_frame=4096), dict(perc_frame=256.0), dict(perc_hop=0),
                dict(perc_hop=257), dict(perc_frame=64, perc_hop=65), dict(perc_hop=1.5),
                dict(method="L_BFGS"), dict(method=None), dict(max_iter=-1), dict(max_iter=2.0), dict(max_iter=True),
                dict(hpss_iter=-1), dict(hpss_iter=1.0), dict(kernel_size=30), dict(kernel_size=129), dict(power=0),
                dict(phase_lock=None)):
        with pytest.raises(ValueError):
            si.time_stretch_hpss(X, 0.8, **bad, **KW)
    for name in ("wsola", "ola", "time_stretch_hpss"):
        assert callable(getattr(si, name)) and name in tsm.__all__


def test_an_empty_batch_needs_no_device():
    for dtype in (torch.float32, torch.float64, torch.float16, torch.bfloat16):
        e = torch.zeros(0, 600, dtype=dtype)
        y, lags = si.wsola(e, 0.8, 64, return_lags=True)
        assert y.shape == (0, 750) and y.dtype == dtype
        assert lags.shape == (0, n_frames(750, 64, 32)) and lags.dtype == torch.int32
        assert si.wsola(e, 0.8, 64).shape == (0, 750)
        assert si.ola(e, 2.0, length=17).shape == (0, 17) and si.ola(e, 2.0).dtype == dtype
        assert si.ola(e, 2.0).shape == (0, 300)


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def test_abi_argument_errors_do_not_need_a_gpu(lib):
    assert lib.specinv_abi_version() == 1
    buf = (C.c_double * 512)()
    base = C.addressof(buf)
    px, pc, pw, pl, py = (base + 512 * i for i in range(5))

    def call(x=px, centres=pc, window=pw, lags=pl, y=py, batch=1, n_in=40, n_out=50, n_frames=None, frame=16, hop=8, tol=4,
             dtype=_lib.F32):
        if n_frames is None:
            n_frames = n_frames_of(n_out, frame, hop)
        return lib.specinv_wsola(x, centres, window, lags, y, batch, n_in, n_out, n_frames, frame, hop, tol, dtype, 0, None)

    def n_frames_of(n_out, frame, hop):
        return (n_out - 1 + frame // 2) // hop + 1 if hop > 0 and n_out > 0 else 1

    for kw, word in ((dict(x=None), b"NULL x"), (dict(centres=None), b"NULL centres"), (dict(window=None), b"NULL window"),
                     (dict(lags=None), b"NULL lags"), (dict(y=None), b"NULL y"), (dict(y=px), b"alias x"),
                     (dict(batch=0), b"batch"), (dict(n_in=0), b"n_in"), (dict(n_out=0), b"n_out"), (dict(n_out=-3), b"n_out"),
                     (dict(frame=0), b"frame must"), (dict(frame=15), b"frame must"), (dict(frame=2050), b"frame must"),
                     (dict(frame=-16), b"frame must"), (dict(hop=0), b"hop must"), (dict(hop=17), b"hop must"),
                     (dict(hop=-1), b"hop must"), (dict(tol=-1), b"tol must"), (dict(tol=1025), b"tol must"),
                     (dict(n_frames=7), b"n_frames is"), (dict(n_frames=9), b"n_frames is"), (dict(n_frames=0), b"n_frames is"),
                     (dict(dtype=7), b"dtype"), (dict(dtype=-1), b"dtype"),
                     # the documented order: the earlier error is the one reported
                     (dict(x=None, y=None, batch=0), b"NULL x"), (dict(y=px, batch=0), b"alias x"), (dict(batch=0, frame=15), b"batch"),
                     (dict(frame=15, hop=0), b"frame must"), (dict(hop=0, tol=-1), b"hop must"), (dict(tol=-1, n_frames=1), b"tol must"),
                     (dict(n_frames=1, dtype=7), b"n_frames is")):
        assert call(**kw) == _lib.EINVAL, kw
        assert word in lib.specinv_last_error(), (kw, lib.specinv_last_error())
    assert n_frames_of(50, 16, 8) == 8
