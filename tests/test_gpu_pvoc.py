"""phase_vocoder and time_stretch on the device against the definition's float64 restatement on the CPU (tests/_pvoc_torch.py).

Shapes and rates are chosen so that k_phase_vocoder meets every corner: T_out below 64, exactly 64, 65 and above 128 (a carry
crosses a step of 64 frames), B * F no multiple of 4 (a partial last workgroup), repeated source frames (rate 0.3), skipped ones
(rate 2.5), T_out = 1 (rate >= T), one- and two-sided spectra.

Bounds.  The error is max |P - P_ref| / max |P_ref|, P_ref the float64 algorithm on the input's bits.
  float32: e_cal is the error of the same restatement with float32 angles and everything else in float64 - what an ideal
    implementation of the kernel's arithmetic has.  The kernel must stay within 4 e_cal + 2^-22: the device's atan2f and magnitude
    may each be an ulp or two from the host's and such errors add as a random walk over T_out; 2^-22 is the final rounding.
  float32 accumulation: at least 10 x below the plain float32 op chain on the same input.
  float64: <= 1e-11, a few hundred ulp-sized angle errors accumulated.
"""
import math

import pytest
import torch

import spectrogram_inversion_amd as si
from _pvoc_torch import max_err, pvoc_chain_f32, pvoc_ref

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DEV = "cuda"


def _wave(n, batch, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=F64)
    chirp = torch.sin(2 * math.pi * (0.02 * t + 0.5 * (0.3 / n) * t * t))
    return chirp + 0.3 * torch.randn(batch, n, generator=g, dtype=F64)


_SPECS = {}


def _spec(n_fft, hop, onesided, batch, frames, dtype):
    """STFT of a seeded chirp + 0.3 noise, made on the CPU once per shape (B, F, frames)"""
    key = (n_fft, hop, onesided, batch, frames, dtype)
    if key not in _SPECS:
        x = _wave((frames - 1) * hop, batch, seed=n_fft + frames)
        w = torch.hann_window(n_fft, dtype=F64)
        s = torch.stft(x, n_fft, hop_length=hop, window=w, onesided=onesided, return_complex=True)
        assert s.shape == (batch, n_fft // 2 + 1 if onesided else n_fft, frames)
        _SPECS[key] = s.to(torch.complex64 if dtype == F32 else torch.complex128)
    return _SPECS[key]


def _kw(n_fft, hop, onesided, dtype):
    return dict(hop_length=hop, onesided=onesided, window=torch.hann_window(n_fft, dtype=dtype))


# (n_fft, hop, onesided, batch (None: unbatched), frames, rate, dtype)
CASES = ([(128, 32, True, 3, 150, r, d) for r in (0.3, 0.8, 1.0, 1.25, 2.5) for d in (F32, F64)]
         + [(400, 160, True, None, 51, r, d) for r in (0.8, 7.3) for d in (F32, F64)]
         + [(512, 128, False, 2, 40, r, d) for r in (0.5, 1.6) for d in (F32, F64)]
         + [(512, 128, True, 2, 5, r, F32) for r in (5.0, 9.0)]
         + [(128, 32, True, 1, 52, 0.8, d) for d in (F32, F64)])          # T_out = 65


def _id(c):
    return f"{c[0]}-{c[1]}-{'one' if c[2] else 'two'}-B{c[3]}-T{c[4]}-r{c[5]}-{'f32' if c[6] == F32 else 'f64'}"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_parity_with_the_float64_definition(case):
    n_fft, hop, onesided, batch, frames, rate, dtype = case
    s = _spec(n_fft, hop, onesided, batch or 1, frames, dtype)
    if batch is None:
        s = s[0]
    ref = pvoc_ref(s, rate, n_fft, hop)
    p = si.phase_vocoder(s.to(DEV), rate, **_kw(n_fft, hop, onesided, dtype))
    assert p.device.type == "cuda" and p.dtype == s.dtype and p.shape == ref.shape
    assert p.shape[-1] == si.stretched_frames(frames, rate)
    err = max_err(p, ref)
    if dtype == F64:
        print(f"{_id(case)}: T_out {p.shape[-1]} float64 error {err:.2e}")
        assert err <= 1e-11
        return
    e_cal = max_err(pvoc_ref(s, rate, n_fft, hop, angle_dtype=F32), ref)
    print(f"{_id(case)}: T_out {p.shape[-1]} float32 error {err:.2e}, e_cal {e_cal:.2e}")
    assert err <= 4 * e_cal + 2.0 ** -22
    if frames >= 150:
        chain = max_err(pvoc_chain_f32(s, rate, n_fft, hop), ref)
        print(f"{_id(case)}: plain float32 chain {chain:.2e}")
        assert 10 * err <= chain


def test_t_out_covers_the_steps_of_the_scan():
    """the cases above do meet the frame counts they are there for"""
    outs = {si.stretched_frames(c[4], c[5]) for c in CASES}
    assert 1 in outs and 64 in outs and 65 in outs and any(n < 64 for n in outs) and any(n > 128 for n in outs)
    assert (3 * 65) % 4 and 201 % 4


def test_silence_and_zero_padding():
    n_fft, hop, rate = 128, 32, 0.8
    s = _spec(n_fft, hop, True, 3, 150, F32)[:1]
    s = torch.cat([s, torch.zeros(1, s.shape[1], 20, dtype=s.dtype)], -1)               # 20 frames of +0 appended
    both = torch.cat([s, torch.zeros_like(s)], 0)                                       # ... beside an item silent throughout
    kw = _kw(n_fft, hop, True, F32)
    p = si.phase_vocoder(both.to(DEV), rate, **kw).cpu()
    assert torch.isfinite(torch.view_as_real(p)).all()
    t = torch.arange(p.shape[-1], dtype=F64) * rate
    i = torch.floor(t).long()
    sp = torch.cat([both, torch.zeros(2, s.shape[1], 2, dtype=s.dtype)], -1)
    silent = (sp[:, :, i] == 0) & (sp[:, :, i + 1] == 0)
    assert silent[0].any() and silent[1].all()
    assert (p[silent] == 0).all()
    alone = si.phase_vocoder(s.to(DEV), rate, **kw).cpu()
    assert torch.equal(torch.view_as_real(alone[0]), torch.view_as_real(p[0]))
    assert max_err(alone, pvoc_ref(s, rate, n_fft, hop)) <= 4 * max_err(pvoc_ref(s, rate, n_fft, hop, angle_dtype=F32),
                                                                        pvoc_ref(s, rate, n_fft, hop)) + 2.0 ** -22


def test_rate_one_returns_the_input():
    n_fft, hop = 128, 32
    s = _spec(n_fft, hop, True, 3, 150, F32)
    ref = pvoc_ref(s, 1.0, n_fft, hop)
    e_cal = max_err(pvoc_ref(s, 1.0, n_fft, hop, angle_dtype=F32), ref)
    p = si.phase_vocoder(s.to(DEV), 1.0, **_kw(n_fft, hop, True, F32))
    err = max_err(p, s)
    print(f"rate 1: error against the input {err:.2e}, e_cal {e_cal:.2e}")
    assert p.shape == s.shape and err <= 4 * e_cal + 2.0 ** -22


@pytest.mark.parametrize("method", ["accelerated_griffin_lim", "griffin_lim"])
def test_time_stretch_is_the_composition(method):
    n_fft, hop, rate = 512, 128, 0.8
    x = _wave(hop * 60, 2, seed=7).to(F32).to(DEV)
    kw = dict(hop_length=hop, window=torch.hann_window(n_fft))
    y = si.time_stretch(x, rate, n_fft, max_iter=5, method=method, verbose=False, **kw)
    run = getattr(si, method)
    p = si.phase_vocoder(si.stft(x, n_fft, **kw), rate, **kw)
    y2 = run(p, max_iter=5, verbose=False, **kw)
    assert y.dtype == F32 and y.device.type == "cuda"
    assert y.shape == (2, (si.stretched_frames(61, rate) - 1) * hop)
    assert torch.equal(y, y2)
    assert torch.equal(si.time_stretch(x, rate, n_fft, max_iter=0, **kw), si.istft(p, **kw))


def test_time_stretch_at_rate_one_reproduces_the_signal():
    n_fft, hop = 512, 128
    x = _wave(hop * 60, 2, seed=8).to(F32).to(DEV)
    kw = dict(hop_length=hop, window=torch.hann_window(n_fft))
    y = si.time_stretch(x, 1.0, n_fft, max_iter=0, **kw)
    assert y.shape == x.shape
    inner = slice(n_fft, x.shape[1] - n_fft)
    base = float((si.istft(si.stft(x, n_fft, **kw), **kw) - x)[:, inner].abs().max())
    err = float((y - x)[:, inner].abs().max())
    print(f"time_stretch at rate 1: max error {err:.2e}, istft(stft(x)) itself {base:.2e}")
    assert err <= 4 * base


def _rel(a, b):
    return float(torch.linalg.norm((a - b).double()) / torch.linalg.norm(b.double()))


@pytest.mark.parametrize("rate", [0.8, 1.25])
def test_refinement_reduces_the_inconsistency(rate):
    n_fft, hop = 512, 128
    x = _wave(hop * 300, 1, seed=9).to(F32).to(DEV)
    kw = dict(hop_length=hop, window=torch.hann_window(n_fft))
    target = si.phase_vocoder(si.stft(x, n_fft, **kw), rate, **kw).abs()
    inc = {}
    for it in (0, 30):
        y = si.time_stretch(x, rate, n_fft, max_iter=it, verbose=False, tol=0, **kw)
        inc[it] = _rel(si.stft(y, n_fft, **kw).abs(), target)
    print(f"rate {rate}: inconsistency {inc[0]:.3f} after the vocoder, {inc[30]:.3f} after 30 iterations")
    assert inc[30] <= 0.5 * inc[0]


def test_shape_dtype_and_device_contract():
    n_fft, hop = 128, 32
    s = _spec(n_fft, hop, True, 3, 150, F32)
    kw = _kw(n_fft, hop, True, F32)
    n_out = si.stretched_frames(150, 1.25)
    one = si.phase_vocoder(s[0].to(DEV), 1.25, **kw)                                     # unbatched in, unbatched out
    assert one.shape == (65, n_out) and one.dtype == torch.complex64 and one.device.type == "cuda"
    batched = si.phase_vocoder(s.to(DEV), 1.25, **kw)
    assert batched.shape == (3, 65, n_out) and torch.equal(torch.view_as_real(batched[0]), torch.view_as_real(one))
    cpu = si.phase_vocoder(s, 1.25, **kw)                                                # a CPU tensor in, a CPU tensor out
    assert cpu.device.type == "cpu" and torch.equal(torch.view_as_real(cpu), torch.view_as_real(batched.cpu()))
    half = si.phase_vocoder(s.to(torch.complex32).to(DEV), 1.25, **kw)
    assert half.dtype == torch.complex32 and half.shape == batched.shape
    d = si.phase_vocoder(s.to(torch.complex128).to(DEV), 1.25, **_kw(n_fft, hop, True, F64))
    assert d.dtype == torch.complex128
    with pytest.raises(NotImplementedError):
        si.phase_vocoder(s.to(DEV).requires_grad_(True), 1.25, **kw)
    with torch.no_grad():
        si.phase_vocoder(s.to(DEV).requires_grad_(True), 1.25, **kw)
    y = si.time_stretch(torch.zeros(hop * 20), 2.0, n_fft, max_iter=0, **kw)             # (L,) on the CPU
    assert y.shape == ((si.stretched_frames(21, 2.0) - 1) * hop,) and y.device.type == "cpu"
