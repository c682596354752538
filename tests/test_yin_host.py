"""YIN without a GPU: the oracle of tests/_yin_oracle.py against a second literal implementation and against the properties of the
definition, `yin_frames`, `envelope_order_for_f0`, and the argument errors of the public functions and of specinv_yin, all raised
before the device is touched.

Measured with this oracle: three harmonics of period 50.37 / 72.37 / 100.37 samples, frames of 512 ... 2048, give tau* = 50 / 72 /
100 in every frame and a refined period within 0.0087 / 0.0079 / 0.0060 samples of the truth (the parabola through three points of
a minimum that is not a parabola), against the 0.37 of the integer lag."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import spectrogram_inversion_amd as si
import _yin_oracle as o
from spectrogram_inversion_amd import _lib, build


def _literal_cmnd(f):
    """d' of one frame, written out with plain loops"""
    n = len(f)
    w = n // 2
    out, run = [1.0], 0.0
    for tau in range(1, w + 1):
        d = 0.0
        for j in range(w):
            d += (f[j] - f[j + tau]) ** 2
        run += d
        out.append(d * tau / run if run > 0 else 1.0)
    return np.array(out)


def test_the_oracle_against_a_second_literal_implementation():
    rng = np.random.default_rng(0)
    x = rng.standard_normal(700)
    for n, hop, center in ((64, 16, True), (64, 50, False), (256, 100, True)):
        f = o.frames(x, n, hop, center)
        assert f.shape == (o.n_frames(700, n, hop, center), n)
        if center:
            assert (f[0, :n // 2] == 0).all() and (f[0, n // 2:] == x[:n // 2]).all()
        else:
            assert (f[1] == x[hop:hop + n]).all()
        got = o.cmnd(x, n, hop, center)
        for m in (0, 1, len(f) // 2, len(f) - 1):
            assert np.abs(got[m] - _literal_cmnd(f[m])).max() <= 1e-12
    # the identity the kernel uses: d = E(0) + E(tau) - 2 r(tau)
    f = o.frames(x, 64, 16, False)
    w = 32
    e = np.array([[(row[t:t + w] ** 2).sum() for t in range(w + 1)] for row in f])
    r = np.array([[(row[:w] * row[t:t + w]).sum() for t in range(w + 1)] for row in f])
    assert np.abs(o.difference(f) - (e[:, :1] + e - 2 * r)).max() <= 1e-11
    # and its float32 restatement stays close on plain noise
    assert np.abs(o.cmnd_f32(x, 256, 64) - o.cmnd(x.astype(np.float32), 256, 64)).max() <= 1e-5


def test_an_integer_period_is_an_exact_zero():
    rng = np.random.default_rng(1)
    for n, p in ((256, 37), (512, 100), (1024, 211)):
        x = np.tile(rng.standard_normal(p), 6 * n // p + 2)[:6 * n]
        dp = o.cmnd(x, n, n // 4, center=False)
        assert (dp[:, p] == 0).all() and (dp[:, 0] == 1).all()
        f0, voiced, ap, tau = o.yin(x, o.SR, o.SR / (n // 2 - 1), 1000.0, n, n // 4, center=False)
        assert (tau == p).all() and voiced.all() and (ap == 0).all()
        assert np.abs(o.SR / f0 - p).max() < 0.5             # (the parabola through unequal neighbours moves off an exact zero)


def test_the_refinement_recovers_a_fractional_period():
    for n in (512, 1024, 2048):
        for p in (50.37, 72.37, 100.37):
            i = np.arange(4 * n)
            x = sum(np.sin(2 * np.pi * h * i / p) / h for h in range(1, 4))
            f0, voiced, _, tau = o.yin(x, o.SR, 60.0, 1000.0, n, n // 4, center=False)
            err = np.abs(o.SR / f0 - p).max()
            print(f"N {n} period {p}: tau* {tau[0]}, refined period off by {err:.4f} samples")
            assert voiced.all() and (tau == math.floor(p)).all()
            assert err <= 0.02                       # measured 0.0087 at the worst (module docstring); the integer lag is 0.37 off


def test_silence_is_one_everywhere_and_unvoiced():
    x = np.zeros(2048)
    dp = o.cmnd(x, 512, 128)
    assert (dp == 1).all() and (o.cmnd_f32(x, 512, 128) == 1).all()
    f0, voiced, ap, tau = o.yin(x, o.SR, 60.0, 1000.0, 512, 128)
    assert (tau == 8).all() and not voiced.any() and (ap == 1).all() and (f0 == o.SR / 8).all()
    assert o.tie_margin(dp[0], 8, 134, 0.1) == math.inf


def test_tie_margin_names_the_closest_comparison():
    dp = np.ones(20)
    dp[5:9] = (0.3, 0.09, 0.05, 0.0507)
    assert o.pick(dp, 2, 15, 0.1) == 7
    assert abs(o.tie_margin(dp, 2, 15, 0.1) - 0.0007) <= 1e-12          # the stop of the descent
    dp[8] = 0.2
    assert abs(o.tie_margin(dp, 2, 15, 0.1) - 0.01) <= 1e-12            # d'(tau0) against the threshold
    dp[5:9] = (0.3, 0.25, 0.2504, 0.4)
    assert o.pick(dp, 2, 15, 0.1) == 6
    assert abs(o.tie_margin(dp, 2, 15, 0.1) - 0.0004) <= 1e-12          # the runner-up of the arg-min


def test_yin_frames_agrees_with_the_oracle():
    for n in (256, 2048):
        for hop in (1, 100, n // 4, n):
            for length in (1, 5, hop - 1, hop, hop + 1, n - 1, n, n + 1, 8 * n + 37):
                if length < 1:
                    continue
                assert si.yin_frames(length, n, hop) == o.n_frames(length, n, hop) == len(o.frames(np.zeros(length), n, hop))
                if length >= n:
                    assert si.yin_frames(length, n, hop, center=False) == o.n_frames(length, n, hop, False)
                else:
                    with pytest.raises(ValueError, match="center=False"):
                        si.yin_frames(length, n, hop, center=False)
    assert si.yin_frames(5, 2048, 512) == 1 and si.yin_frames(5, 2048) == 1 and si.yin_frames(2048, 2048, None, False) == 1
    for bad in (dict(length=0), dict(length=2.0), dict(length=True), dict(hop_length=0), dict(hop_length=257), dict(hop_length=64.0),
                dict(frame_length=0), dict(frame_length="256"), dict(frame_length=256.0)):
        args = dict(length=1000, frame_length=256, hop_length=64)
        args.update(bad)
        with pytest.raises(ValueError):
            si.yin_frames(**args)
    with pytest.raises(NotImplementedError, match="256, 512, 1024, 2048"):
        si.yin_frames(1000, 4096, 64)


def test_the_envelope_order_follows_f0():
    for sr in (8000, 16000, 22050.0, 44100, 100):
        assert si.envelope_order_for_f0(sr, 300) == si.default_envelope_order(sr)
    assert si.envelope_order_for_f0(16000, 100.0) == 80 and si.envelope_order_for_f0(16000, 800) == 10
    assert si.envelope_order_for_f0(8000, 1e6) == 1
    for bad in (0, -1.0, float("nan"), float("inf"), "300", None, True):
        with pytest.raises(ValueError, match="f0"):
            si.envelope_order_for_f0(16000, bad)
        with pytest.raises(ValueError, match="sample_rate"):
            si.envelope_order_for_f0(bad, 300)


def _refuse_load(monkeypatch):
    def refuse():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", refuse)


def test_argument_errors_come_before_the_device(monkeypatch):
    _refuse_load(monkeypatch)
    x = torch.zeros(2, 5000)
    good = dict(sample_rate=8000, fmin=60, fmax=1000)
    for bad in (dict(sample_rate=0), dict(sample_rate=float("nan")), dict(sample_rate="8000"), dict(sample_rate=None),
                dict(sample_rate=True), dict(fmin=0), dict(fmin=-60), dict(fmin=float("inf")), dict(fmin=None), dict(fmin="60"),
                dict(fmax=0), dict(fmax=float("nan")), dict(fmax=None), dict(fmax=60), dict(fmax=50),
                dict(fmax=9000),                                                    # tau_min = 0
                dict(threshold=0), dict(threshold=-0.1), dict(threshold=float("nan")), dict(threshold=float("inf")),
                dict(threshold=None), dict(threshold="0.1"), dict(threshold=True),
                dict(hop_length=0), dict(hop_length=2049), dict(hop_length=512.0), dict(hop_length=True),
                dict(frame_length=0), dict(frame_length=2048.0), dict(frame_length=None), dict(frame_length=True)):
        args = dict(good)
        args.update(bad)
        with pytest.raises(ValueError):
            si.yin(x, **args)
    # the lags must fit the frame: the message names the smallest fmin that does
    for n, fmin in ((2048, 7.0), (1024, 15.0), (512, 31.0), (256, 62.9)):
        with pytest.raises(ValueError, match="smallest fmin") as info:
            si.yin(x, 8000, fmin, 1000, frame_length=n)
        assert repr(8000 / (n // 2 - 1)) in str(info.value)
    for n in (128, 4096, 300, 1000):
        with pytest.raises(NotImplementedError, match="256, 512, 1024, 2048"):
            si.yin(x, frame_length=n, **good)
        with pytest.raises(NotImplementedError, match="256, 512, 1024, 2048"):
            si.yin_cmnd(x, frame_length=n)
    for fn in (lambda t, **kw: si.yin(t, **good, **kw), si.yin_cmnd):
        with pytest.raises(TypeError):
            fn(np.zeros(5000))
        with pytest.raises(TypeError):
            fn(torch.zeros(5000, dtype=torch.int32))
        with pytest.raises(TypeError):
            fn(torch.zeros(5000, dtype=torch.complex64))
        with pytest.raises(NotImplementedError, match="float32"):
            fn(torch.zeros(5000, dtype=torch.float64))
        for shape in ((), (2, 2, 5000), (2, 0)):
            with pytest.raises(ValueError):
                fn(torch.zeros(shape))
        with pytest.raises(ValueError, match="center=False"):
            fn(torch.zeros(2, 2047), center=False)
        with pytest.raises(NotImplementedError, match="not differentiable; detach the input"):
            fn(torch.zeros(5000, requires_grad=True))
        with pytest.raises(ValueError):
            fn(x, hop_length=-1)


def test_an_empty_batch_needs_no_device(monkeypatch):
    _refuse_load(monkeypatch)
    for dtype in (torch.float32, torch.float16):
        f0, voiced, ap, tau = si.yin(torch.zeros(0, 5000, dtype=dtype), 8000, 60, 1000, 512, 100, return_tau=True)
        assert f0.shape == voiced.shape == ap.shape == tau.shape == (0, 51)
        assert (f0.dtype, voiced.dtype, ap.dtype, tau.dtype) == (torch.float32, torch.bool, torch.float32, torch.int32)
        dp = si.yin_cmnd(torch.zeros(0, 5000, dtype=dtype), 512, 100, center=False)
        assert dp.shape == (0, 45, 257) and dp.dtype == torch.float32


def test_pitch_shift_takes_the_word_f0_and_no_other(monkeypatch):
    _refuse_load(monkeypatch)
    x = torch.zeros(2, 4096)
    kw = dict(n_fft=512, hop_length=128, window=torch.hann_window(512), max_iter=2, verbose=False)
    for preserve in (True, False):
        for bad in ("F0", "yin", "", "27"):
            with pytest.raises(ValueError, match="formant_order"):
                si.pitch_shift(x, 16000, 4, preserve_formants=preserve, formant_order=bad, **kw)


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def test_abi_argument_errors_do_not_need_a_gpu(lib):
    buf = (C.c_double * 512)()
    base = C.addressof(buf)
    p, q, r, s, t = (base + 512 * i for i in range(5))

    def call(x=p, period=q, aper=r, tau=s, cmnd=t, batch=1, length=5000, frame=512, hop=128, center=1, tau_min=8, tau_max=134,
             threshold=0.1, dtype=_lib.F32):
        return lib.specinv_yin(x, period, aper, tau, cmnd, batch, length, frame, hop, center, tau_min, tau_max, threshold, dtype, 0,
                               None)

    nan, inf = float("nan"), float("inf")
    for kw, code, word in ((dict(x=None), _lib.EINVAL, b"NULL x"), (dict(period=None), _lib.EINVAL, b"NULL period_out"),
                           (dict(aper=None), _lib.EINVAL, b"NULL aper_out"),
                           (dict(period=p), _lib.EINVAL, b"period_out must not alias x"),
                           (dict(aper=q), _lib.EINVAL, b"aper_out must not alias period_out"),
                           (dict(tau=p), _lib.EINVAL, b"tau_out must not alias x"),
                           (dict(cmnd=s), _lib.EINVAL, b"cmnd_out must not alias tau_out"),
                           (dict(cmnd=r), _lib.EINVAL, b"cmnd_out must not alias aper_out"),
                           (dict(batch=0), _lib.EINVAL, b"batch"), (dict(batch=-3), _lib.EINVAL, b"batch"),
                           (dict(dtype=7), _lib.EINVAL, b"dtype"), (dict(dtype=_lib.F64), _lib.EUNSUPPORTED, b"float32"),
                           (dict(frame=128), _lib.EUNSUPPORTED, b"frame"), (dict(frame=4096), _lib.EUNSUPPORTED, b"frame"),
                           (dict(frame=500), _lib.EUNSUPPORTED, b"frame"),
                           (dict(hop=0), _lib.EINVAL, b"hop"), (dict(hop=513), _lib.EINVAL, b"hop"),
                           (dict(length=0), _lib.EINVAL, b"length"), (dict(length=511, center=0), _lib.EINVAL, b"length"),
                           (dict(tau_min=0), _lib.EINVAL, b"tau_min"), (dict(tau_max=256), _lib.EINVAL, b"tau_min"),
                           (dict(tau_min=134), _lib.EINVAL, b"tau_min"), (dict(tau_min=200, tau_max=100), _lib.EINVAL, b"tau_min"),
                           (dict(threshold=0.0), _lib.EINVAL, b"threshold"), (dict(threshold=-1.0), _lib.EINVAL, b"threshold"),
                           (dict(threshold=nan), _lib.EINVAL, b"threshold"), (dict(threshold=inf), _lib.EINVAL, b"threshold"),
                           # the documented order: the earlier error is the one reported
                           (dict(x=None, period=p), _lib.EINVAL, b"NULL x"), (dict(period=p, batch=0), _lib.EINVAL, b"alias"),
                           (dict(batch=0, dtype=7), _lib.EINVAL, b"batch"), (dict(dtype=7, frame=500), _lib.EINVAL, b"dtype"),
                           (dict(dtype=_lib.F64, frame=500), _lib.EUNSUPPORTED, b"float32"),
                           (dict(frame=500, hop=0), _lib.EUNSUPPORTED, b"frame"), (dict(hop=0, length=0), _lib.EINVAL, b"hop"),
                           (dict(length=0, tau_min=0), _lib.EINVAL, b"length"),
                           (dict(tau_min=0, threshold=nan), _lib.EINVAL, b"tau_min")):
        assert call(**kw) == code, kw
        assert word in lib.specinv_last_error(), (kw, lib.specinv_last_error())
