"""resample / pitch_shift without a GPU: the definition (tests/_resample_oracle.py) against torchaudio's algorithm restated, the
output length, what the width-6 filter does to a tone, the (rate, orig) helper, and the argument errors that are raised before the
device is touched."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import spectrogram_inversion_amd as si
from _resample_oracle import length_out, resample_bank, resample_ref
from spectrogram_inversion_amd import _lib, build

# (orig, new, L)
RATIOS = ((3, 2, 1000), (2, 3, 999), (7, 1, 2000), (1, 5, 33), (160, 147, 1500), (48000, 44100, 700), (27781, 22050, 3000))


@pytest.mark.parametrize("orig,new,length", RATIOS, ids=lambda v: str(v))
def test_the_two_oracles_agree(orig, new, length):
    """measured: 2.6e-13 at 27781:22050, <= 1.4e-14 at 48000:44100 and 160:147, <= 4e-16 at the small ratios"""
    x = np.random.default_rng(orig + new).standard_normal((2, length))
    ref = resample_ref(x, orig, new)
    bank = resample_bank(torch.from_numpy(x), orig, new).numpy()
    assert ref.shape == bank.shape == (2, length_out(length, orig, new))
    err = float(np.abs(ref - bank).max() / np.abs(ref).max())
    print(f"{orig}:{new} L {length}: definition against the filter bank {err:.2e}")
    assert err <= 1e-11


@pytest.mark.parametrize("orig,new,length", RATIOS, ids=lambda v: str(v))
def test_output_length(orig, new, length):
    g = math.gcd(orig, new)
    for n_in in (1, length):
        want = math.ceil((new // g) * n_in / (orig // g))         # (exact: these products are far below 2^53)
        assert length_out(n_in, orig, new) == want
        assert resample_ref(np.ones((1, n_in)), orig, new).shape == (1, want)


def test_a_tone_is_reproduced_to_the_filters_ripple():
    """0.05 cycles/sample through 27781 -> 22050: 4.6e-4 away from the ends, the passband ripple of the width-6 filter"""
    t = np.arange(4000)
    y = resample_ref(np.sin(2 * np.pi * 0.05 * t), 27781, 22050)
    want = np.sin(2 * np.pi * 0.05 * np.arange(y.shape[-1]) * 27781 / 22050)
    err = float(np.abs(y - want)[50:-50].max())
    print(f"tone through 27781:22050: {err:.2e}")
    assert err <= 1e-3


def test_shift_rate_is_torchaudios_two_lines():
    from spectrogram_inversion_amd.timescale import shift_rate
    assert shift_rate(16000, 12, 12) == (0.5, 32000)
    assert shift_rate(16000, -12, 12) == (2.0, 8000)
    assert shift_rate(22050, 4, 12)[1] == 27781
    assert shift_rate(22050, 4)[0] == 2.0 ** (-4 / 12)
    for sr in (1, 8000, 22050, 44100):
        assert shift_rate(sr, 0, 12) == (1.0, sr)
        assert shift_rate(sr, 0.0, 7) == (1.0, sr)


def test_pitch_shift_argument_errors_come_before_the_device():
    x = torch.zeros(2, 1024)
    kw = dict(n_fft=128, hop_length=32, window=torch.hann_window(128))
    for bad in (dict(sample_rate=0), dict(sample_rate=16000.0), dict(sample_rate=True), dict(bins_per_octave=0),
                dict(bins_per_octave=1.5), dict(n_steps="a"), dict(n_steps=None), dict(n_steps=float("nan")),
                dict(n_steps=float("inf")), dict(n_steps=True), dict(method="RTISI_LA"), dict(max_iter=-1)):
        args = dict(sample_rate=16000, n_steps=4, **kw)
        args.update(bad)
        with pytest.raises(ValueError):
            si.pitch_shift(x, **args)
    assert "pitch_shift" in si.timescale.__all__


def test_resample_argument_errors_come_before_the_device():
    x = torch.zeros(2, 100)
    with pytest.raises(TypeError):
        si.resample(x.numpy(), 3, 2)
    with pytest.raises(TypeError):
        si.resample(torch.zeros(2, 100, dtype=torch.complex64), 3, 2)
    with pytest.raises(TypeError):
        si.resample(torch.zeros(2, 100, dtype=torch.int32), 3, 2)
    for orig, new in ((0, 2), (3, 0), (-3, 2), (3.0, 2), (3, 2.0), (True, 2), (3, False), ("3", 2), (None, 2)):
        with pytest.raises(ValueError):
            si.resample(x, orig, new)
    for width in (0, -1, 6.0, True, None):
        with pytest.raises(ValueError):
            si.resample(x, 3, 2, lowpass_filter_width=width)
    for rolloff in (0, 0.0, -0.5, 1.01, float("nan"), "0.9", None, True):
        with pytest.raises(ValueError):
            si.resample(x, 3, 2, rolloff=rolloff)
    with pytest.raises(ValueError):
        si.resample(torch.zeros(()), 3, 2)
    with pytest.raises(ValueError):
        si.resample(torch.zeros(2, 3, 100), 3, 2)
    with pytest.raises(ValueError, match="62 bits"):
        si.resample(x, (1 << 61) + 1, 1 << 61)                      # L_out * o beyond 62 bits
    with pytest.raises(NotImplementedError, match="resample is not differentiable; detach the input"):
        si.resample(x.clone().requires_grad_(True), 3, 2)


def test_resample_without_a_launch_needs_no_device():
    """equal rates copy, and an input without samples has nothing to compute"""
    x = torch.randn(3, 50, generator=torch.Generator().manual_seed(0))
    for orig, new in ((5, 5), (44100, 44100)):
        y = si.resample(x, orig, new)
        assert y.data_ptr() != x.data_ptr() and torch.equal(y, x)
    assert si.resample(torch.zeros(0, 100), 3, 2).shape == (0, 67)
    assert si.resample(torch.zeros(4, 0, dtype=torch.float64), 3, 2).shape == (4, 0)
    assert si.resample(torch.zeros(0), 2, 3).shape == (0,)


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def test_abi_argument_errors_do_not_need_a_gpu(lib):
    assert lib.specinv_abi_version() == 1
    buf = (C.c_double * 64)()
    p, q = C.addressof(buf), C.addressof(buf) + 256

    def call(x=p, y=q, batch=1, n_in=10, n_out=7, orig=3, new=2, width=6, rolloff=0.99, dtype=_lib.F32):
        return lib.specinv_resample(x, y, batch, n_in, n_out, orig, new, width, rolloff, dtype, 0, None)

    for kw, word in ((dict(x=None), b"NULL x"), (dict(y=None), b"NULL y"), (dict(y=p), b"alias"),
                     (dict(n_out=6), b"n_out"), (dict(n_out=8), b"n_out"), (dict(orig=30, new=20, n_out=8), b"n_out"),
                     (dict(orig=0), b"orig_freq"), (dict(new=-2), b"new_freq"), (dict(batch=0), b"batch"), (dict(n_in=0), b"n_in"),
                     (dict(width=0), b"lowpass_filter_width"), (dict(rolloff=0.0), b"rolloff"), (dict(rolloff=1.5), b"rolloff"),
                     (dict(rolloff=float("nan")), b"rolloff"), (dict(dtype=7), b"dtype"),
                     (dict(orig=(1 << 61) + 1, new=1 << 61, n_out=10), b"62 bits")):
        assert call(**kw) == _lib.EINVAL, kw
        assert word in lib.specinv_last_error(), (kw, lib.specinv_last_error())
