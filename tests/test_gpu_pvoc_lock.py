"""phase_vocoder / time_stretch / pitch_shift with phase_lock="identity" on the device against the definition's float64 restatement
on the CPU (tests/_pvoc_lock_torch.py).

Shapes are those of test_gpu_pvoc.py, for the same corners of the scan (T_out below 64, 64, 65, above 128, 1; B * F no multiple of
4), and for those of k_pvoc_lock_apply: F = 65 and 201 (a last band of 1 and of 9 bins), F = 64 and 512 two-sided (the owner search
runs over the wrap-around), T_out = 7 and 65 (a partial chunk of 64 frames), a chirp in noise (a peak every few bins) and a harmonic
signal (peaks several bands apart).

Bounds.  The error is max |P - P_ref| / max |P_ref|, P_ref the locked restatement in float64 on the input's bits.
  float64: <= 1e-11.
  float32: <= 4 e_cal + 2^-22, e_cal the locked restatement with float32 angles against the same with float64 angles - the
    reference's own calibration.  The peak decisions do not depend on the angles: q is exact in float64.
"""
import math

import pytest
import torch

import spectrogram_inversion_amd as si
from _pvoc_lock_torch import (COMB_HOP, COMB_N_FFT, COMB_OWNER, _parts, comb_spec, harmonic_wave, lock_ref, peaks_and_owners)
from _pvoc_torch import max_err
from spectrogram_inversion_amd import _lib
from spectrogram_inversion_amd.plan import args_helper, get_plan

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DEV = "cuda"
LOCK = "identity"


def _chirp(n, batch, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=F64)
    chirp = torch.sin(2 * math.pi * (0.02 * t + 0.5 * (0.3 / n) * t * t))
    return chirp + 0.3 * torch.randn(batch, n, generator=g, dtype=F64)


_SPECS = {}


def _spec(kind, n_fft, hop, onesided, batch, frames, dtype):
    """STFT of the seeded chirp + 0.3 noise of test_gpu_pvoc.py or of the harmonic signal, made on the CPU once per shape"""
    key = (kind, n_fft, hop, onesided, batch, frames, dtype)
    if key not in _SPECS:
        n = (frames - 1) * hop
        x = _chirp(n, batch, n_fft + frames) if kind == "chirp" else harmonic_wave(n, batch, n_fft + frames)
        w = torch.hann_window(n_fft, dtype=F64)
        s = torch.stft(x, n_fft, hop_length=hop, window=w, onesided=onesided, return_complex=True)
        assert s.shape == (batch, n_fft // 2 + 1 if onesided else n_fft, frames)
        _SPECS[key] = s.to(torch.complex64 if dtype == F32 else torch.complex128)
    return _SPECS[key]


def _kw(n_fft, hop, onesided, dtype):
    return dict(hop_length=hop, onesided=onesided, window=torch.hann_window(n_fft, dtype=dtype))


_REFS = {}


def _ref(s, key, rate, n_fft, hop, angle_dtype=F64):
    key = key + (rate, angle_dtype)
    if key not in _REFS:
        _REFS[key] = lock_ref(s, rate, n_fft, hop, angle_dtype=angle_dtype)
    return _REFS[key]


def _bound(s, key, rate, n_fft, hop):
    """4 e_cal + 2^-22 for a complex64 input"""
    e_cal = max_err(_ref(s, key, rate, n_fft, hop, F32), _ref(s, key, rate, n_fft, hop))
    return 4 * e_cal + 2.0 ** -22, e_cal


# (signal, n_fft, hop, onesided, batch (None: unbatched), frames, rate, dtype)
CASES = ([("chirp", 128, 32, True, 3, 150, r, d) for r in (0.3, 0.8, 1.0, 1.25, 2.5) for d in (F32, F64)]
         + [("harmonic", 128, 32, True, 3, 150, r, d) for r in (0.8, 2.5) for d in (F32, F64)]
         + [("chirp", 400, 160, True, None, 51, r, d) for r in (0.8, 7.3) for d in (F32, F64)]
         + [(k, 64, 16, False, 2, 40, r, d) for k in ("chirp", "harmonic") for r in (0.5, 1.6) for d in (F32, F64)]
         + [("chirp", 512, 128, False, 2, 40, r, d) for r in (0.5, 1.6) for d in (F32, F64)]
         + [("harmonic", 512, 128, True, 2, 40, 0.5, d) for d in (F32, F64)]
         + [("chirp", 128, 32, True, 1, 52, 0.8, d) for d in (F32, F64)]                    # T_out = 65
         + [("chirp", 512, 128, True, 2, 5, r, F32) for r in (5.0, 9.0)])                   # T_out = 1


def _id(c):
    return f"{c[0]}-{c[1]}-{c[2]}-{'one' if c[3] else 'two'}-B{c[4]}-T{c[5]}-r{c[6]}-{'f32' if c[7] == F32 else 'f64'}"


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_parity_with_the_float64_definition(case):
    kind, n_fft, hop, onesided, batch, frames, rate, dtype = case
    s = _spec(kind, n_fft, hop, onesided, batch or 1, frames, dtype)
    if batch is None:
        s = s[0]
    ref = _ref(s, case[:6] + (dtype,), rate, n_fft, hop)
    p = si.phase_vocoder(s.to(DEV), rate, phase_lock=LOCK, **_kw(n_fft, hop, onesided, dtype))
    assert p.device.type == "cuda" and p.dtype == s.dtype and p.shape == ref.shape
    assert p.shape[-1] == si.stretched_frames(frames, rate)
    err = max_err(p, ref)
    if dtype == F64:
        print(f"{_id(case)}: T_out {p.shape[-1]} float64 error {err:.2e}")
        assert err <= 1e-11
        return
    bound, e_cal = _bound(s, case[:6] + (dtype,), rate, n_fft, hop)
    print(f"{_id(case)}: T_out {p.shape[-1]} float32 error {err:.2e}, e_cal {e_cal:.2e}")
    assert err <= bound


def test_the_cases_cover_the_kernels_corners():
    outs = {si.stretched_frames(c[5], c[6]) for c in CASES}
    assert 1 in outs and 7 in outs and 64 in outs and 65 in outs and any(n > 128 for n in outs)
    assert (3 * 65) % 4 and 201 % 4


def test_locking_changes_the_phase_and_keeps_the_magnitude():
    """the locked result is not the unlocked one (a kernel that ignored the mode would pass the parity of a peak-free input only)"""
    n_fft, hop, rate = 128, 32, 0.8
    s = _spec("harmonic", n_fft, hop, True, 3, 150, F32)
    kw = _kw(n_fft, hop, True, F32)
    locked = si.phase_vocoder(s.to(DEV), rate, phase_lock=LOCK, **kw)
    plain = si.phase_vocoder(s.to(DEV), rate, **kw)
    assert max_err(locked, plain) > 0.1
    assert max_err(locked.abs().to(torch.complex64), plain.abs().to(torch.complex64)) <= 2.0 ** -21


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("rate", [1.0, 0.5])
def test_comb_owners_on_the_device(rate, dtype):
    cd = torch.complex64 if dtype == F32 else torch.complex128
    s = comb_spec(cd)
    kw = dict(hop_length=COMB_HOP, window=torch.hann_window(COMB_N_FFT, dtype=dtype))
    p = si.phase_vocoder(s.to(DEV), rate, phase_lock=LOCK, **kw).cpu().to(torch.complex128)
    n_out = p.shape[1]
    want = torch.tensor([COMB_OWNER[int(j * rate)] for j in range(n_out)]).T
    assert torch.equal(peaks_and_owners(s, rate, COMB_N_FFT, COMB_HOP)[1], want)
    _, th0, m, phi = _parts(s, rate, COMB_N_FFT, COMB_HOP, dtype)
    psi = torch.where(want >= 0, torch.gather(phi - th0, 0, want.clamp(min=0)) + th0, phi)     # from the owners written out
    live = m > 0
    turn = torch.angle(p[live] * torch.polar(torch.ones_like(psi[live]), -psi[live]))
    print(f"comb at rate {rate}: largest phase error {float(turn.abs().max()):.2e} rad")
    # the phases are random, a bin under another owner is off by radians; 1e-5: the float32 rounding of P (6e-8 relative)
    assert float(turn.abs().max()) <= 1e-5
    assert (p[~live] == 0).all()


def test_frames_without_a_peak_equal_the_unlocked_vocoder_bit_for_bit():
    for dtype in (F32, F64):
        cd = torch.complex64 if dtype == F32 else torch.complex128
        s = comb_spec(cd)
        kw = dict(hop_length=COMB_HOP, window=torch.hann_window(COMB_N_FFT, dtype=dtype))
        for rate in (1.0, 0.5):
            locked = si.phase_vocoder(s.to(DEV), rate, phase_lock=LOCK, **kw).cpu()
            plain = si.phase_vocoder(s.to(DEV), rate, **kw).cpu()
            none = torch.tensor([COMB_OWNER[int(j * rate)][0] < 0 for j in range(locked.shape[1])])
            assert none.any() and not none.all()
            assert torch.equal(torch.view_as_real(locked[:, none]), torch.view_as_real(plain[:, none]))
            assert not torch.equal(torch.view_as_real(locked[:, ~none]), torch.view_as_real(plain[:, ~none]))
    # a flat spectrum (equal q throughout) of a size with several bands and chunks
    flat = torch.full((2, 65, 150), 3 + 4j, dtype=torch.complex64)
    kw = _kw(128, 32, True, F32)
    assert torch.equal(torch.view_as_real(si.phase_vocoder(flat.to(DEV), 0.8, phase_lock=LOCK, **kw)),
                       torch.view_as_real(si.phase_vocoder(flat.to(DEV), 0.8, **kw)))


def test_silence_and_zero_padding():
    n_fft, hop, rate = 128, 32, 0.8
    s = _spec("chirp", n_fft, hop, True, 3, 150, F32)[:1]
    s = torch.cat([s, torch.zeros(1, s.shape[1], 20, dtype=s.dtype)], -1)               # 20 frames of +0 appended
    both = torch.cat([s, torch.zeros_like(s)], 0)                                       # ... beside an item silent throughout
    kw = _kw(n_fft, hop, True, F32)
    p = si.phase_vocoder(both.to(DEV), rate, phase_lock=LOCK, **kw).cpu()
    assert torch.isfinite(torch.view_as_real(p)).all()
    t = torch.arange(p.shape[-1], dtype=F64) * rate
    i = torch.floor(t).long()
    sp = torch.cat([both, torch.zeros(2, s.shape[1], 2, dtype=s.dtype)], -1)
    silent = (sp[:, :, i] == 0) & (sp[:, :, i + 1] == 0)
    assert silent[0].any() and silent[1].all()
    assert (p[silent] == 0).all()
    alone = si.phase_vocoder(s.to(DEV), rate, phase_lock=LOCK, **kw).cpu()
    assert torch.equal(torch.view_as_real(alone[0]), torch.view_as_real(p[0]))
    ref = lock_ref(s, rate, n_fft, hop)
    assert max_err(alone, ref) <= 4 * max_err(lock_ref(s, rate, n_fft, hop, angle_dtype=F32), ref) + 2.0 ** -22


def _old_entry(s, rate, kw, mode=None):
    """specinv_phase_vocoder (mode None) or specinv_phase_vocoder_locked at `mode`, called on the plan the public function uses"""
    s = s.to(DEV).contiguous()                                  # (torch.stft's result is not)
    n_out = si.stretched_frames(s.shape[2], rate)
    plan = get_plan(args_helper(s, **kw), s.shape[0], n_out, s.real.dtype, s.device)
    plan._sync_stream()
    out = torch.empty((s.shape[0], s.shape[1], n_out), dtype=s.dtype, device=s.device)
    if mode is None:
        _lib.check(plan.lib.specinv_phase_vocoder(plan._h, s.data_ptr(), int(s.shape[2]), float(rate), out.data_ptr()))
    else:
        _lib.check(plan.lib.specinv_phase_vocoder_locked(plan._h, s.data_ptr(), int(s.shape[2]), float(rate), mode, out.data_ptr()))
    torch.cuda.synchronize()
    return out, plan


@pytest.mark.parametrize("dtype", [F32, F64])
def test_no_lock_is_the_old_entry_point_bit_for_bit(dtype):
    n_fft, hop, rate = 128, 32, 0.8
    s = _spec("chirp", n_fft, hop, True, 3, 150, dtype)
    kw = _kw(n_fft, hop, True, dtype)
    old, plan = _old_entry(s, rate, kw)
    for p in (si.phase_vocoder(s.to(DEV), rate, **kw), si.phase_vocoder(s.to(DEV), rate, phase_lock=None, **kw),
              plan.phase_vocoder(s.to(DEV), rate), _old_entry(s, rate, kw, mode=0)[0]):
        assert torch.equal(torch.view_as_real(p), torch.view_as_real(old))
    # ... also after a locked call on the same plan, which reserved the scratch
    before = plan.device_bytes
    locked = _old_entry(s, rate, kw, mode=1)[0]
    assert plan.device_bytes >= before and plan.device_bytes >= 8 * old.numel()
    assert torch.equal(torch.view_as_real(locked), torch.view_as_real(si.phase_vocoder(s.to(DEV), rate, phase_lock=LOCK, **kw)))
    assert torch.equal(torch.view_as_real(_old_entry(s, rate, kw, mode=0)[0]), torch.view_as_real(old))
    with pytest.raises(AssertionError, match="mode"):
        _old_entry(s, rate, kw, mode=2)
    with pytest.raises(ValueError, match="phase_lock"):
        plan.phase_vocoder(s.to(DEV), rate, "scaled")


def test_rate_one_returns_the_input():
    n_fft, hop = 128, 32
    s = _spec("chirp", n_fft, hop, True, 3, 150, F32)
    bound, e_cal = _bound(s, ("chirp", n_fft, hop, True, 3, 150, F32), 1.0, n_fft, hop)
    p = si.phase_vocoder(s.to(DEV), 1.0, phase_lock=LOCK, **_kw(n_fft, hop, True, F32))
    err = max_err(p, s)
    print(f"rate 1: error against the input {err:.2e}, e_cal {e_cal:.2e}")
    assert p.shape == s.shape and err <= bound


@pytest.mark.parametrize("method", ["accelerated_griffin_lim", "griffin_lim", "ADMM"])
def test_time_stretch_is_the_composition(method):
    n_fft, hop, rate = 512, 128, 0.8
    x = _chirp(hop * 60, 2, seed=7).to(F32).to(DEV)
    kw = dict(hop_length=hop, window=torch.hann_window(n_fft))
    y = si.time_stretch(x, rate, n_fft, max_iter=5, method=method, phase_lock=LOCK, verbose=False, **kw)
    p = si.phase_vocoder(si.stft(x, n_fft, **kw), rate, phase_lock=LOCK, **kw)
    y2 = getattr(si, method)(p, max_iter=5, verbose=False, **kw)
    assert y.dtype == F32 and y.device.type == "cuda"
    assert y.shape == (2, (si.stretched_frames(61, rate) - 1) * hop)
    assert torch.equal(y, y2)
    assert not torch.equal(y, si.time_stretch(x, rate, n_fft, max_iter=5, method=method, verbose=False, **kw))
    assert torch.equal(si.time_stretch(x, rate, n_fft, max_iter=0, method=method, phase_lock=LOCK, **kw), si.istft(p, **kw))


def test_pitch_shift_hands_the_argument_through():
    n_fft, hop, sr = 256, 64, 16000
    x = harmonic_wave(4096, 2, seed=4).to(F32).to(DEV)
    kw = dict(n_fft=n_fft, max_iter=4, hop_length=hop, window=torch.hann_window(n_fft), verbose=False)
    z = si.pitch_shift(x, sr, 3, phase_lock=LOCK, **kw)
    rate, orig = si.timescale.shift_rate(sr, 3)
    y = si.resample(si.time_stretch(x, rate, phase_lock=LOCK, **kw), orig, sr)
    n = x.shape[-1]
    want = y[..., :n] if y.shape[-1] >= n else torch.nn.functional.pad(y, (0, n - y.shape[-1]))
    assert z.shape == x.shape and torch.equal(z, want)
    assert not torch.equal(z, si.pitch_shift(x, sr, 3, **kw))


def _rel(a, b):
    return float(torch.linalg.norm((a - b).double()) / torch.linalg.norm(b.double()))


@pytest.mark.parametrize("rate", [0.5, 0.8])
def test_locking_halves_the_inconsistency_on_the_device(rate):
    n_fft, hop = 512, 128
    x = harmonic_wave(hop * 119, 1, seed=5).to(F32).to(DEV)
    kw = dict(hop_length=hop, window=torch.hann_window(n_fft))
    inc = {}
    for lock in (None, LOCK):
        target = si.phase_vocoder(si.stft(x, n_fft, **kw), rate, phase_lock=lock, **kw).abs()
        y = si.time_stretch(x, rate, n_fft, max_iter=0, phase_lock=lock, **kw)
        inc[lock] = _rel(si.stft(y, n_fft, **kw).abs(), target)
    print(f"rate {rate}: inconsistency {inc[None]:.3f} unlocked, {inc[LOCK]:.3f} locked ({inc[LOCK] / inc[None]:.2f} x)")
    assert inc[LOCK] <= 0.5 * inc[None]


def test_shape_dtype_and_device_contract():
    n_fft, hop = 128, 32
    s = _spec("chirp", n_fft, hop, True, 3, 150, F32)
    kw = _kw(n_fft, hop, True, F32)
    n_out = si.stretched_frames(150, 1.25)
    one = si.phase_vocoder(s[0].to(DEV), 1.25, phase_lock=LOCK, **kw)                    # unbatched in, unbatched out
    assert one.shape == (65, n_out) and one.dtype == torch.complex64 and one.device.type == "cuda"
    batched = si.phase_vocoder(s.to(DEV), 1.25, phase_lock=LOCK, **kw)
    assert batched.shape == (3, 65, n_out) and torch.equal(torch.view_as_real(batched[0]), torch.view_as_real(one))
    cpu = si.phase_vocoder(s, 1.25, phase_lock=LOCK, **kw)                               # a CPU tensor in, a CPU tensor out
    assert cpu.device.type == "cpu" and torch.equal(torch.view_as_real(cpu), torch.view_as_real(batched.cpu()))
    half = si.phase_vocoder(s.to(torch.complex32).to(DEV), 1.25, phase_lock=LOCK, **kw)
    assert half.dtype == torch.complex32 and half.shape == batched.shape
    d = si.phase_vocoder(s.to(torch.complex128).to(DEV), 1.25, phase_lock=LOCK, **_kw(n_fft, hop, True, F64))
    assert d.dtype == torch.complex128
    with pytest.raises(NotImplementedError):
        si.phase_vocoder(s.to(DEV).requires_grad_(True), 1.25, phase_lock=LOCK, **kw)
    with torch.no_grad():
        si.phase_vocoder(s.to(DEV).requires_grad_(True), 1.25, phase_lock=LOCK, **kw)
    y = si.time_stretch(torch.zeros(hop * 20), 2.0, n_fft, max_iter=0, phase_lock=LOCK, **kw)      # (L,) on the CPU
    assert y.shape == ((si.stretched_frames(21, 2.0) - 1) * hop,) and y.device.type == "cpu"
