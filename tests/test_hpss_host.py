"""hpss without a GPU: the definition (tests/_hpss_oracle.py) against scipy's median filter where scipy's is defined, the
properties of the masks, and the argument errors of the five public functions and of specinv_hpss, all raised before the device is
touched."""
import ctypes as C

import numpy as np
import pytest
import torch

import spectrogram_inversion_amd as si
from _hpss_oracle import masks, medians, refl
from spectrogram_inversion_amd import _lib, build

SHAPES = ((3, 5), (17, 40), (33, 129))
SIZES = (1, 3, 5, 17, 31)


def test_refl_is_the_symmetric_extension_continued_periodically():
    assert refl(np.arange(-7, 8), 3).tolist() == [0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1]
    assert refl(np.arange(-3, 4), 1).tolist() == [0] * 7
    x = np.arange(5.0)
    assert np.array_equal(x[refl(np.arange(-5, 10), 5)], np.pad(x, 5, mode="symmetric"))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_oracle_medians_are_scipys_where_the_window_reaches_no_further_than_the_axis(shape):
    """compared for k // 2 <= the axis length only: beyond it scipy 1.15.3's own extension is wrong
    (median_filter([1., 2.], size=17, mode='reflect') is zeros)"""
    from scipy.ndimage import median_filter
    a = np.abs(np.random.default_rng(shape[0]).standard_normal(shape))
    a[::3] = np.round(4 * a[::3]) / 4                                  # ties
    for k in SIZES:
        harm, perc = medians(a, k, k)
        if k // 2 <= shape[1]:
            assert np.array_equal(harm, median_filter(a, size=(1, k), mode="reflect")), k
        if k // 2 <= shape[0]:
            assert np.array_equal(perc, median_filter(a, size=(k, 1), mode="reflect")), k
    assert np.array_equal(median_filter(np.array([1.0, 2.0]), size=17, mode="reflect"), np.zeros(2))
    assert np.array_equal(medians(np.array([[1.0, 2.0]]), 17, 1)[0], np.array([[1.0, 2.0]]))     # 9 of the 17 are the bin's own value


def test_oracle_medians_are_window_elements_and_complex_takes_the_float64_magnitude():
    rng = np.random.default_rng(0)
    a = rng.standard_normal((7, 9)).astype(np.float32)
    a = np.abs(a)
    for got in medians(a, 5, 3):
        assert np.isin(got, a.astype(np.float64)).all()
    s = (rng.standard_normal((7, 9)) + 1j * rng.standard_normal((7, 9))).astype(np.complex64)
    mag = np.sqrt(s.real.astype(np.float64) ** 2 + s.imag.astype(np.float64) ** 2)
    assert np.array_equal(medians(s, 5, 3)[0], medians(mag, 5, 3)[0])


@pytest.mark.parametrize("power", (1, 2, 0.5, 3))
def test_oracle_masks_sum_to_one_at_margin_one(power):
    a = np.abs(np.random.default_rng(1).standard_normal((17, 40)))
    mh, mp = masks(a, 5, 7, power)
    assert np.abs(mh + mp - 1).max() <= 2 * 2.0 ** -52
    assert mh.min() >= 0 and mh.max() <= 1 and mp.min() >= 0 and mp.max() <= 1


def test_oracle_masks_of_silence_and_binary_masks():
    z = np.zeros((6, 8))
    for power in (1, 2, 0.5, 3):
        mh, mp = masks(z, 3, 3, power)
        assert (mh == 0.5).all() and (mp == 0.5).all()
        mh, mp = masks(z, 3, 3, power, 2.0, 1.0)
        assert (mh == 0).all() and (mp == 0).all()
    # below float32's smallest normal number is silence for a float32 input and is not for a float64 one
    q = np.full((4, 4), 1e-39)
    assert (masks(q, 3, 3, 2.0, real_dtype=np.float32)[0] == 0.5).all()
    a = np.abs(np.random.default_rng(2).standard_normal((17, 40)))
    a[::3] = 0
    for m_h, m_p in ((1, 1), (2, 1), (1, 3.5)):
        mh, mp = masks(a, 5, 7, float("inf"), m_h, m_p)
        assert np.isin(mh, (0.0, 1.0)).all() and np.isin(mp, (0.0, 1.0)).all()
        assert not (mh * mp).any()                                    # never both


KW = dict(n_fft=128, hop_length=32, window=torch.hann_window(128))


def _spec_calls(spec, **kw):
    """the three functions that take a spectrogram, with whichever of **kw each one has"""
    yield lambda: si.hpss(spec, **kw)
    yield lambda: si.hpss(spec, mask=True, **kw)
    if not set(kw) - {"kernel_size"}:
        yield lambda: si.hpss_medians(spec, **kw)


def _audio_calls(x, **kw):
    for fn in (si.hpss_audio, si.harmonic, si.percussive):
        yield lambda fn=fn: fn(x, **KW, **kw)


def test_argument_errors_come_before_the_device():
    spec, x = torch.ones(4, 6), torch.zeros(2, 1024)
    for bad in (dict(kernel_size=0), dict(kernel_size=4), dict(kernel_size=30), dict(kernel_size=129), dict(kernel_size=(31, 4)),
                dict(kernel_size=(0, 31)), dict(kernel_size=-3), dict(kernel_size=3.0), dict(kernel_size=True),
                dict(kernel_size=(3, 3, 3)), dict(kernel_size=None),
                dict(margin=0.5), dict(margin=(1.0, 0.5)), dict(margin=(0.99, 1.0)), dict(margin=float("inf")),
                dict(margin=float("nan")), dict(margin="1"), dict(margin=(1, 1, 1)),
                dict(power=0), dict(power=0.0), dict(power=-1.0), dict(power=float("nan")), dict(power="2"), dict(power=None)):
        calls = list(_spec_calls(spec, **bad)) + list(_audio_calls(x, **bad))
        assert len(calls) >= 5
        for call in calls:
            with pytest.raises(ValueError):
                call()
    for call in list(_spec_calls(torch.ones(4, 6, dtype=torch.int32))) + list(_audio_calls(torch.zeros(2, 1024, dtype=torch.int32))):
        with pytest.raises(TypeError):
            call()
    for call in list(_spec_calls(np.ones((4, 6)))) + list(_audio_calls(np.zeros((2, 1024)))):
        with pytest.raises(TypeError):
            call()
    for shape in ((6,), (2, 2, 4, 6), (), (3, 0, 4), (3, 4, 0)):
        for call in _spec_calls(torch.ones(shape)):
            with pytest.raises(ValueError):
                call()
    for call in _audio_calls(torch.zeros(2, 2, 2, 1024)):
        with pytest.raises(ValueError):
            call()
    for name, call in zip(("hpss", "hpss", "hpss_medians"), _spec_calls(torch.ones(4, 6, requires_grad=True))):
        with pytest.raises(NotImplementedError, match=f"{name} is not differentiable; detach the input"):
            call()
    for call in _audio_calls(torch.zeros(2, 1024, requires_grad=True)):
        with pytest.raises(NotImplementedError, match="hpss_audio is not differentiable; detach the input"):
            call()
    for bad in (dict(max_iter=2, margin=2.0), dict(max_iter=2, margin=(1.0, 1.5)), dict(max_iter=-1), dict(max_iter=1.0),
                dict(max_iter=True)):
        for call in _audio_calls(x, **bad):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError, match="both margins equal to 1"):
        si.hpss_audio(x, max_iter=2, margin=2.0, **KW)
    for name in ("hpss", "hpss_medians", "hpss_audio", "harmonic", "percussive"):
        assert callable(getattr(si, name))


def test_an_empty_batch_needs_no_device():
    for dtype, real in ((torch.float32, torch.float32), (torch.complex64, torch.float32), (torch.float16, torch.float16)):
        e = torch.zeros(0, 5, 7, dtype=dtype)
        h, p = si.hpss(e)
        assert h.shape == p.shape == (0, 5, 7) and h.dtype == p.dtype == dtype
        for out in si.hpss(e, mask=True) + si.hpss_medians(e):
            assert out.shape == (0, 5, 7) and out.dtype == real


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def test_abi_argument_errors_do_not_need_a_gpu(lib):
    assert lib.specinv_abi_version() == 1
    buf = (C.c_double * 96)()
    p, q, r = C.addressof(buf), C.addressof(buf) + 256, C.addressof(buf) + 512
    nan, inf = float("nan"), float("inf")

    def call(spec=p, out_a=q, out_b=r, batch=1, n_freq=2, n_frames=3, win_harm=31, win_perc=31, power=2.0, margin_harm=1.0,
             margin_perc=1.0, out_mode=_lib.HPSS_COMPONENTS, is_complex=0, dtype=_lib.F32):
        return lib.specinv_hpss(spec, out_a, out_b, batch, n_freq, n_frames, win_harm, win_perc, power, margin_harm, margin_perc,
                                out_mode, is_complex, dtype, 0, None)

    for kw, word in ((dict(spec=None), b"NULL spec"), (dict(out_a=None), b"NULL out_a"), (dict(out_b=None), b"NULL out_b"),
                     (dict(out_a=p), b"alias spec"), (dict(out_b=p), b"alias spec"), (dict(out_b=q), b"alias out_a"),
                     (dict(batch=0), b"batch"), (dict(n_freq=0), b"n_freq"), (dict(n_frames=-1), b"n_frames"),
                     (dict(win_harm=0), b"win_harm"), (dict(win_harm=30), b"win_harm"), (dict(win_harm=129), b"win_harm"),
                     (dict(win_perc=0), b"win_perc"), (dict(win_perc=4), b"win_perc"), (dict(win_perc=129), b"win_perc"),
                     (dict(power=0.0), b"power"), (dict(power=-2.0), b"power"), (dict(power=nan), b"power"),
                     (dict(margin_harm=0.5), b"margin_harm"), (dict(margin_harm=inf), b"margin_harm"),
                     (dict(margin_harm=nan), b"margin_harm"), (dict(margin_perc=0.5), b"margin_perc"),
                     (dict(margin_perc=inf), b"margin_perc"), (dict(margin_perc=nan), b"margin_perc"),
                     (dict(out_mode=3), b"out_mode"), (dict(out_mode=-1), b"out_mode"), (dict(dtype=7), b"dtype"),
                     # the documented order: the earlier error is the one reported
                     (dict(spec=None, out_a=p, batch=0), b"NULL spec"), (dict(out_a=p, batch=0), b"alias"),
                     (dict(batch=0, win_harm=4), b"batch"), (dict(win_harm=4, win_perc=4), b"win_harm"),
                     (dict(win_perc=4, power=0.0), b"win_perc"), (dict(power=0.0, margin_harm=0.5), b"power"),
                     (dict(margin_harm=0.5, margin_perc=0.5), b"margin_harm"), (dict(margin_perc=0.5, out_mode=9), b"margin_perc"),
                     (dict(out_mode=9, dtype=7), b"out_mode")):
        assert call(**kw) == _lib.EINVAL, kw
        assert word in lib.specinv_last_error(), (kw, lib.specinv_last_error())
