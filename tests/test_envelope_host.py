"""The spectral envelope without a GPU: the identities of its definition (tests/_envelope_oracle.py), what the true-envelope
iteration buys over plain cepstral smoothing, the formant property in float64, and the argument errors of the public functions and
of specinv_spectral_envelope, all raised before the device is touched.

The voice: harmonics of 150 Hz under three resonances, 8192 samples at 16 kHz, frames of 512 every 128, order 27.  Measured with
this oracle: the mean gap between the strong spectral peaks and the envelope is 13.0 dB at n_iter 0, 2.5 at 4, 0.9 at 8 and 0.02
at 16; an ideal shifter (pitch and resonances moved together) leaves the envelope 4.85 / 4.36 / 6.15 dB from the original at
+4 / -4 / +7 semitones, and imposing the original's envelope at n_iter 16 brings that to 0.38 / 0.07 / 1.70 dB (n_iter 0: 7.07 /
5.63 / 9.61 dB - plain smoothing makes it worse)."""
import ctypes as C

import numpy as np
import pytest
import torch

import spectrogram_inversion_amd as si
from _envelope_oracle import (DB, envelope, envelope_distance_db, impose, log_envelope, log_floor, peak_gap_db, smooth, stft,
                              voice)
from spectrogram_inversion_amd import _lib, build

N_FFT, HOP, ORDER, SR = 512, 128, 27, 16000


@pytest.fixture(scope="module")
def spoken():
    x = voice(150.0, 1.0, 8192, SR)
    return x, stft(x, N_FFT, HOP)


def test_full_order_is_the_identity_and_order_zero_the_mean():
    rng = np.random.default_rng(0)
    for n_fft in (16, 256, 512):
        S = np.abs(rng.standard_normal((2, n_fft // 2 + 1, 5))) + 1e-3
        a0 = log_floor(S)
        assert np.abs(log_envelope(S, n_fft // 2, 0) - a0).max() <= 1e-12
        assert np.abs(log_envelope(S, n_fft // 2, 7) - a0).max() <= 1e-12
        mean = (a0[:, :1] + a0[:, -1:] + 2 * a0[:, 1:-1].sum(axis=1, keepdims=True)) / n_fft
        assert np.abs(log_envelope(S, 0, 0) - mean).max() <= 1e-12
        assert np.abs(smooth(a0, 3) - smooth(smooth(a0, 3), 3)).max() <= 1e-12          # C is a projection


def test_the_iteration_never_sinks():
    """V_i = C(max(a0, V_{i-1})) smooths something that is nowhere below what V_{i-1} smoothed, but C is not monotone; what does
    hold is that the mean (quefrency 0) never falls"""
    S = np.abs(np.random.default_rng(1).standard_normal((129, 6))) + 1e-3
    means = [smooth(log_envelope(S, 10, i), 0)[0] for i in range(6)]
    for a, b in zip(means, means[1:]):
        assert (b >= a - 1e-12).all()


def test_silence_is_finite():
    rng = np.random.default_rng(2)
    S = np.abs(rng.standard_normal((2, 129, 7)))
    S[0] = 0                                  # an all-zero item beside a loud one
    S[1, :, 3] = 0                            # one silent frame inside a signal
    v = log_envelope(S, 12, 16)
    assert np.isfinite(v).all()
    assert (v[0] == 0).all() and (envelope(S, 12, 16)[0] == 1).all()
    amin = 1e-6 * S[1].max()
    assert np.abs(v[1, :, 3] - np.log(amin)).max() <= 1e-9               # a flat frame is its own envelope


def test_true_envelope_against_smoothing(spoken):
    _, S = spoken
    a0 = log_floor(S)
    gaps = {n: peak_gap_db(a0, log_envelope(S, ORDER, n)) for n in (0, 4, 16)}
    print("mean gap at strong peaks, dB:", {n: round(g, 2) for n, g in gaps.items()})
    assert gaps[0] > 10
    assert -1 <= gaps[16] <= 1
    assert gaps[0] > gaps[4] > gaps[16]


@pytest.mark.parametrize("steps,before,after", ((4, 4.0, 1.0), (-4, 4.0, 1.0), (7, None, 2.0)), ids=("+4", "-4", "+7"))
def test_formant_property_in_float64(spoken, steps, before, after):
    x, _ = spoken
    r = 2.0 ** (steps / 12)
    y0 = voice(150.0 * r, r, 8192, SR)
    d0 = envelope_distance_db(y0, x, N_FFT, HOP, ORDER, r)
    d1 = envelope_distance_db(impose(y0, x, N_FFT, HOP, ORDER, 16), x, N_FFT, HOP, ORDER, r)
    print(f"{steps:+d} semitones: envelope distance {d0:.2f} dB -> {d1:.2f} dB")
    if before is not None:
        assert d0 > before
    assert d1 < after and d1 < d0


def test_default_order():
    assert si.default_envelope_order(16000) == 27 and si.default_envelope_order(44100) == 74
    assert si.default_envelope_order(100) == 1 and si.default_envelope_order(22050.0) == 37
    for bad in (0, -1, float("nan"), float("inf"), "16000", None, True):
        with pytest.raises(ValueError):
            si.default_envelope_order(bad)


def _refuse_load(monkeypatch):
    def refuse():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", refuse)


def test_argument_errors_come_before_the_device(monkeypatch):
    _refuse_load(monkeypatch)
    spec, x = torch.ones(257, 6), torch.zeros(2, 4096)
    kw = dict(n_fft=512, hop_length=128, window=torch.hann_window(512))
    for bad in (dict(order=-1), dict(order=257), dict(order=3.0), dict(order=True), dict(order=None), dict(order="3"),
                dict(n_iter=-1), dict(n_iter=257), dict(n_iter=2.0), dict(n_iter=True), dict(n_iter=None),
                dict(floor=0), dict(floor=-1e-6), dict(floor=float("nan")), dict(floor=float("inf")), dict(floor="1e-6"),
                dict(floor=None), dict(floor=True)):
        args = dict(order=27)
        args.update(bad)
        with pytest.raises(ValueError):
            si.spectral_envelope(spec, **args)
        with pytest.raises(ValueError):
            si.spectral_envelope(spec.T.contiguous(), frame_major=True, **args)
        if "order" not in bad or bad["order"] not in (None, 257):        # impose_envelope: None is a default, 257 is met after the STFT
            with pytest.raises(ValueError):
                si.impose_envelope(x, x, **kw, **args)
    for bad in (dict(max_gain_db=-1), dict(max_gain_db=float("nan")), dict(max_gain_db="40"), dict(max_gain_db=None)):
        with pytest.raises(ValueError):
            si.impose_envelope(x, x, order=27, **kw, **bad)
    with pytest.raises(ValueError):
        si.impose_envelope(x, x[:, :-1], order=27, **kw)
    for shape in ((257,), (2, 2, 257, 6), (3, 257, 0), (3, 1, 4)):
        with pytest.raises(ValueError):
            si.spectral_envelope(torch.ones(shape), 27)
    with pytest.raises(TypeError):
        si.spectral_envelope(np.ones((257, 6)), 27)
    with pytest.raises(TypeError):
        si.spectral_envelope(torch.ones(257, 6, dtype=torch.int32), 27)
    for dtype in (torch.float64, torch.complex128):
        with pytest.raises(NotImplementedError, match="float32"):
            si.spectral_envelope(torch.ones(257, 6, dtype=dtype), 27)
    with pytest.raises(NotImplementedError, match="float32"):
        si.impose_envelope(x.double(), x.double(), order=27, **kw)
    for n_freq in (256, 512, 1024, 2048):
        with pytest.raises(NotImplementedError, match="two-sided"):
            si.spectral_envelope(torch.ones(n_freq, 6), 27)
    for n_freq in (65, 33, 2049, 200, 258):
        with pytest.raises(NotImplementedError, match="n_fft 256, 512, 1024, 2048"):
            si.spectral_envelope(torch.ones(n_freq, 6), 27)
        with pytest.raises(NotImplementedError, match="n_fft 256, 512, 1024, 2048"):
            si.spectral_envelope(torch.ones(2, 6, n_freq), 27, frame_major=True)
    with pytest.raises(NotImplementedError, match="spectral_envelope is not differentiable; detach the input"):
        si.spectral_envelope(torch.ones(257, 6, requires_grad=True), 27)
    with pytest.raises(NotImplementedError, match="impose_envelope is not differentiable"):
        si.impose_envelope(x.clone().requires_grad_(), x, order=27, **kw)


def test_pitch_shift_checks_the_formant_arguments_before_any_work(monkeypatch):
    _refuse_load(monkeypatch)
    x = torch.zeros(2, 4096)
    kw = dict(n_fft=512, hop_length=128, window=torch.hann_window(512), max_iter=2, verbose=False)
    for preserve in (True, False):
        for bad in (dict(formant_order=-1), dict(formant_order=257), dict(formant_order=3.0), dict(formant_order=True),
                    dict(formant_iter=-1), dict(formant_iter=257), dict(formant_iter=1.5), dict(formant_iter=None)):
            with pytest.raises(ValueError, match="formant_"):
                si.pitch_shift(x, SR, 4, preserve_formants=preserve, **kw, **bad)
    with pytest.raises(ValueError, match="formant_order"):                      # n_fft read from the window, as stft does
        si.pitch_shift(x, SR, 4, hop_length=64, window=torch.hann_window(256), preserve_formants=True, formant_order=129)
    import inspect
    names = set(inspect.signature(si.pitch_shift).parameters)
    assert {"preserve_formants", "formant_order", "formant_iter"} <= names
    assert not {"preserve_formants", "formant_order", "formant_iter"} & set(inspect.signature(si.time_stretch).parameters)


def test_an_empty_batch_needs_no_device(monkeypatch):
    _refuse_load(monkeypatch)
    for dtype, real in ((torch.float32, torch.float32), (torch.complex64, torch.float32), (torch.float16, torch.float16)):
        out = si.spectral_envelope(torch.zeros(0, 257, 7, dtype=dtype), 27)
        assert out.shape == (0, 257, 7) and out.dtype == real


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def test_abi_argument_errors_do_not_need_a_gpu(lib):
    buf = (C.c_double * 96)()
    p, q, r = C.addressof(buf), C.addressof(buf) + 256, C.addressof(buf) + 512

    def call(spec=p, out=q, amin=r, batch=1, n_freq=257, n_frames=3, order=27, n_iter=16, out_log=0, is_complex=0, frame_major=0,
             dtype=_lib.F32):
        return lib.specinv_spectral_envelope(spec, out, amin, batch, n_freq, n_frames, order, n_iter, out_log, is_complex,
                                             frame_major, dtype, 0, None)

    for kw, code, word in ((dict(spec=None), _lib.EINVAL, b"NULL spec"), (dict(out=None), _lib.EINVAL, b"NULL out"),
                           (dict(amin=None), _lib.EINVAL, b"NULL amin"), (dict(out=p), _lib.EINVAL, b"alias"),
                           (dict(batch=0), _lib.EINVAL, b"batch"), (dict(n_frames=0), _lib.EINVAL, b"n_frames"),
                           (dict(n_iter=-1), _lib.EINVAL, b"n_iter"), (dict(n_iter=257), _lib.EINVAL, b"n_iter"),
                           (dict(dtype=7), _lib.EINVAL, b"dtype"), (dict(dtype=_lib.F64), _lib.EUNSUPPORTED, b"float32"),
                           (dict(n_freq=65), _lib.EUNSUPPORTED, b"n_freq"), (dict(n_freq=512), _lib.EUNSUPPORTED, b"n_freq"),
                           (dict(n_freq=2049), _lib.EUNSUPPORTED, b"n_freq"), (dict(order=-1), _lib.EINVAL, b"order"),
                           (dict(order=257), _lib.EINVAL, b"order"),
                           # the documented order: the earlier error is the one reported
                           (dict(spec=None, batch=0), _lib.EINVAL, b"NULL spec"), (dict(out=p, batch=0), _lib.EINVAL, b"alias"),
                           (dict(batch=0, n_iter=-1), _lib.EINVAL, b"batch"), (dict(n_iter=-1, dtype=7), _lib.EINVAL, b"n_iter"),
                           (dict(dtype=_lib.F64, n_freq=65), _lib.EUNSUPPORTED, b"float32"),
                           (dict(n_freq=65, order=-1), _lib.EUNSUPPORTED, b"n_freq")):
        assert call(**kw) == code, kw
        assert word in lib.specinv_last_error(), (kw, lib.specinv_last_error())
