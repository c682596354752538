"""pitch_shift on the device: it is time_stretch, resample and a crop or pad, bit for bit, and a tone moves by the interval.

All cases: n_fft 256, hop 64, a Hann window, max_iter 8, L = 4096 (65 centred frames).  time_stretch returns (T_out - 1) * 64
samples, T_out = stretched_frames(65, rate), and resampling multiplies that by 16000 / orig: about L + 64 (1 - rate) + 64 rate f
with f in [0, 1) what the frame count was rounded up by.  Raising the pitch (rate < 1) therefore always crops; +4, -3, +12 and 0.5
steps all do (4115, 4111, 4128, 4104 samples).  -6 steps (rate 1.414, f = 0.04) give 4074 samples and pad.
"""
import math

import pytest
import torch

import spectrogram_inversion_amd as si
from spectrogram_inversion_amd.timescale import shift_rate

pytestmark = pytest.mark.gpu

DEV = "cuda"
L, SR = 4096, 16000


def _kw():
    return dict(n_fft=256, hop_length=64, window=torch.hann_window(256), max_iter=8, verbose=False)


def _x(batched):
    g = torch.Generator().manual_seed(11)
    t = torch.arange(L, dtype=torch.float64)
    x = torch.sin(2 * math.pi * 0.03 * t) + 0.3 * torch.randn(2, L, generator=g, dtype=torch.float64)
    x = x.float().to(DEV)
    return x if batched else x[0]


def _fit(y):
    return y[..., :L] if y.shape[-1] >= L else torch.nn.functional.pad(y, (0, L - y.shape[-1]))


# (n_steps, whether the resampled signal is longer than L)
STEPS = ((4, True), (-3, True), (12, True), (0.5, True), (-6, False))


@pytest.mark.parametrize("batched", (False, True), ids=("L", "2xL"))
@pytest.mark.parametrize("n_steps,crops", STEPS, ids=lambda v: str(v))
def test_it_is_the_composition(n_steps, crops, batched):
    x = _x(batched)
    rate, orig = shift_rate(SR, n_steps)
    assert orig != SR
    y = si.time_stretch(x, rate, **_kw())
    y = si.resample(y, orig, SR, 6, 0.99)
    print(f"n_steps {n_steps}: rate {rate:.4f} orig {orig}, {y.shape[-1]} samples before the {'crop' if crops else 'pad'}")
    assert (y.shape[-1] > L) == crops and y.shape[-1] != L
    z = si.pitch_shift(x, SR, n_steps, **_kw())
    assert z.shape == x.shape and z.dtype == x.dtype and z.device == x.device
    assert torch.equal(z, _fit(y))
    if not crops:
        assert (z[..., y.shape[-1]:] == 0).all()


def test_the_filter_parameters_reach_resample():
    x = _x(True)
    rate, orig = shift_rate(SR, 4)
    y = si.resample(si.time_stretch(x, rate, **_kw()), orig, SR, 10, 0.9)
    z = si.pitch_shift(x, SR, 4, lowpass_filter_width=10, rolloff=0.9, **_kw())
    assert torch.equal(z, _fit(y)) and not torch.equal(z, si.pitch_shift(x, SR, 4, **_kw()))


@pytest.mark.parametrize("batched", (False, True), ids=("L", "2xL"))
def test_no_steps_launch_no_resampling(batched, monkeypatch):
    import sys
    x = _x(batched)
    want = _fit(si.time_stretch(x, 1.0, **_kw()))

    def refuse(*args, **kwargs):
        raise AssertionError("resample was called")

    monkeypatch.setattr(sys.modules["spectrogram_inversion_amd.resample"], "resample", refuse)
    z = si.pitch_shift(x, SR, 0, **_kw())
    assert z.shape == x.shape and torch.equal(z, want)


@pytest.mark.parametrize("n_steps,want", ((12, 0.10), (-12, 0.025)), ids=("up", "down"))
def test_a_tone_moves_by_the_interval(n_steps, want):
    """the vocoder keeps a stationary tone's frequency, the 2:1 / 1:2 resampling scales it exactly; 1 % of 0.10 is two bins of the
    2048-point transform, the main lobe of the untapered segment"""
    x = torch.sin(2 * math.pi * 0.05 * torch.arange(L, dtype=torch.float64)).float().to(DEV)
    z = si.pitch_shift(x, SR, n_steps, **_kw())
    assert z.shape == x.shape
    mid = z[L // 2 - 1024:L // 2 + 1024].double().cpu()
    peak = int(torch.fft.rfft(mid).abs().argmax()) / 2048
    print(f"n_steps {n_steps}: peak at {peak:.5f} cycles/sample, expected {want}")
    assert abs(peak - want) <= 0.01 * want


def test_errors():
    x = _x(True)
    for bad in (dict(method="RTISI_LA"), dict(sample_rate=0), dict(bins_per_octave=0), dict(n_steps="a")):
        args = dict(sample_rate=SR, n_steps=4, **_kw())
        args.update(bad)
        with pytest.raises(ValueError):
            si.pitch_shift(x, **args)
