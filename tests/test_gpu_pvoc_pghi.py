"""phase_vocoder / time_stretch / pitch_shift / time_stretch_hpss with phase_lock="pghi" on the device, through the public functions
and through specinv_pvoc_pghi, against the definition's float64 restatement in NumPy on the CPU (tests/_pvoc_pghi_oracle.py).

Shapes.  (F, T_in) from (2, 3) - one lane with a bin, a chain of one step - over F = 65 and 129 (a wave and a bit, two waves and a
bit: the totals cross waves), 513 and 1025 (K = 3 and 5 bins a lane, the last lanes empty) to 1537, 2049, 2561 and 2915 (K = 7, 9,
11 and 13, every chunk size the kernel is instantiated for; 2915 is the limit).  Rates below 1 (a source frame is reused), 1, between
1 and 2 (frames advance by one and by two) and 2.3 (both source frames are read anew); T_out = 1.

Bounds.  The parents are compared everywhere: every decision compares values NumPy and the device compute to the same bits.  The
error is max |P - P_ref| / max |P_ref|, P_ref the restatement in float64 on the input's bits.
  float64: <= 1e-11.
  float32: <= 4 e_cal + 2^-22, e_cal the restatement with float32 angles against the same with float64 angles - the gate and margin
    of test_gpu_pvoc.py and test_gpu_pvoc_lock.py.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import spectrogram_inversion_amd as si
from _pvoc_lock_torch import inconsistency
from _pvoc_pghi_oracle import pghi_ref, random_spec, signal, signal_spec
from _pvoc_torch import max_err
from spectrogram_inversion_amd import _lib

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DEV = "cuda"
LOCK = "pghi"


def _cd(dtype):
    return torch.complex64 if dtype == F32 else torch.complex128


def _kw(n_fft, hop, dtype=F32):
    return dict(hop_length=hop, window=torch.hann_window(n_fft, dtype=dtype))


# (F, T_in, rate): batch 3, n_fft = 2 (F - 1), hop = max(1, n_fft // 4)
SHAPES = [(2, 3, 0.5), (3, 1, 2.3), (5, 4, 0.8), (65, 6, 1.25), (129, 5, 1.0), (513, 9, 2.3), (1025, 4, 0.5),
          (1537, 3, 0.8), (2049, 3, 1.25), (2561, 3, 2.3), (2915, 3, 0.5)]
CASES = [(F, T, r, d) for F, T, r in SHAPES for d in (F32, F64)]
_REFS = {}


def _id(c):
    return f"F{c[0]}-T{c[1]}-r{c[2]}-{'f32' if c[3] == F32 else 'f64'}"


def _case(case):
    """(input on the CPU, n_fft, hop, (P, psi, codes) of the oracle), made once"""
    if case not in _REFS:
        F, T, rate, dtype = case
        n_fft = 2 * (F - 1)
        hop = max(1, n_fft // 4)
        s = torch.from_numpy(random_spec(F, T, seed=F + T, batch=3, dtype=np.complex64 if dtype == F32 else np.complex128))
        _REFS[case] = (s, n_fft, hop, pghi_ref(s, rate, n_fft, hop))
    return _REFS[case]


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_parents_and_values_against_the_definition(case):
    F, T, rate, dtype = case
    s, n_fft, hop, (ref, _, codes) = _case(case)
    p, parents = si.phase_vocoder(s.to(DEV), rate, phase_lock=LOCK, return_parents=True, hop_length=hop)
    assert p.device.type == "cuda" and p.dtype == s.dtype and p.shape == ref.shape == (3, F, si.stretched_frames(T, rate))
    assert parents.dtype == torch.int8 and parents.shape == p.shape and parents.device.type == "cuda"
    if F >= 65:
        assert set(np.unique(codes).tolist()) == {0, 1, 2, 3}
    wrong = int((parents.cpu().numpy() != codes).sum())
    assert wrong == 0, f"{wrong} of {codes.size} parents differ"
    err = max_err(p, torch.from_numpy(ref))
    if dtype == F64:
        print(f"{_id(case)}: T_out {p.shape[-1]} float64 error {err:.2e}")
        assert err <= 1e-11
        return
    e_cal = max_err(torch.from_numpy(pghi_ref(s, rate, n_fft, hop, angle_dtype=np.float32)[0]), torch.from_numpy(ref))
    print(f"{_id(case)}: T_out {p.shape[-1]} float32 error {err:.2e}, e_cal {e_cal:.2e}, "
          f"{err / (4 * e_cal + 2.0 ** -22):.2f} of the gate")
    assert err <= 4 * e_cal + 2.0 ** -22


def test_the_cases_cover_the_kernels_corners():
    assert {(-(-F // 256)) | 1 for F, _, _ in SHAPES} == {1, 3, 5, 7, 9, 11, 13}
    assert 1 in {si.stretched_frames(T, r) for _, T, r in SHAPES} and max(F for F, _, _ in SHAPES) == 2915
    seen = set()
    for case in CASES:
        seen |= set(np.unique(_case(case)[3][2]).tolist())
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("dtype", [F32, F64])
def test_the_entry_point_is_what_the_public_function_calls(dtype):
    case = (513, 9, 2.3, dtype)
    s, n_fft, hop, _ = _case(case)
    d = s.to(DEV).contiguous()
    n_out = si.stretched_frames(9, 2.3)
    out = torch.empty((3, 513, n_out), dtype=d.dtype, device=DEV)
    par = torch.empty((3, 513, n_out), dtype=torch.int8, device=DEV)
    stream = torch.cuda.current_stream()
    lib = _lib.load()
    args = (3, 513, 9, n_out, n_fft, hop, 2.3, 1e-6, _lib.F32 if dtype == F32 else _lib.F64, stream.device.index,
            C.c_void_p(stream.cuda_stream))
    _lib.check(lib.specinv_pvoc_pghi(d.data_ptr(), out.data_ptr(), par.data_ptr(), *args))
    p, parents = si.phase_vocoder(d, 2.3, phase_lock=LOCK, return_parents=True, hop_length=hop)
    assert torch.equal(torch.view_as_real(out), torch.view_as_real(p)) and torch.equal(par, parents)
    out2 = torch.empty_like(out)
    _lib.check(lib.specinv_pvoc_pghi(d.data_ptr(), out2.data_ptr(), None, *args))               # parents_out may be NULL
    assert torch.equal(torch.view_as_real(out2), torch.view_as_real(out))
    assert torch.equal(torch.view_as_real(si.phase_vocoder(d, 2.3, phase_lock=LOCK, hop_length=hop)), torch.view_as_real(out))
    # a larger floor kills more bins and is handed through
    loose = si.phase_vocoder(d, 2.3, phase_lock=LOCK, lock_tol=0.5, return_parents=True, hop_length=hop)[1]
    assert int((loose == 3).sum()) > int((parents == 3).sum())
    assert np.array_equal(loose.cpu().numpy(), pghi_ref(s, 2.3, n_fft, hop, tol=0.5)[2])


_HARM = {}


def _harmonic(dtype=F32, frames=64):
    if (dtype, frames) not in _HARM:
        s, _ = signal_spec("harmonic", 512, 128, frames)
        _HARM[dtype, frames] = s.to(_cd(dtype))
    return _HARM[dtype, frames]


def _gate32(s, rate, n_fft, hop):
    ref = torch.from_numpy(pghi_ref(s, rate, n_fft, hop)[0])
    e_cal = max_err(torch.from_numpy(pghi_ref(s, rate, n_fft, hop, angle_dtype=np.float32)[0]), ref)
    return ref, 4 * e_cal + 2.0 ** -22


def test_the_mode_is_not_ignored_and_leaves_the_other_modes_alone():
    s = _harmonic().unsqueeze(0)
    kw = _kw(512, 128)
    d = s.to(DEV)
    before = [si.phase_vocoder(d, 0.8, phase_lock=lock, **kw) for lock in (None, "identity")]
    pghi = si.phase_vocoder(d, 0.8, phase_lock=LOCK, **kw)
    after = [si.phase_vocoder(d, 0.8, phase_lock=lock, **kw) for lock in (None, "identity")]
    ref, gate = _gate32(s, 0.8, 512, 128)
    assert max_err(pghi, ref) <= gate
    for b, a in zip(before, after):
        assert torch.equal(torch.view_as_real(b), torch.view_as_real(a))
        print(f"pghi against another mode: {max_err(pghi, b):.2e}, gate {gate:.2e}")
        assert b.shape == pghi.shape and max_err(pghi, b) > gate
        # the magnitude is the same but for one rounding of |z| in float64 and the rounding of P
        assert max_err(pghi.abs().to(torch.complex64), b.abs().to(torch.complex64)) <= 2.0 ** -21


def test_silence_and_zero_padding():
    n_fft, hop, rate = 512, 128, 0.8
    s = _harmonic().unsqueeze(0)
    s = torch.cat([s, torch.zeros(1, s.shape[1], 20, dtype=s.dtype)], -1)               # 20 frames of +0 appended
    both = torch.cat([s, torch.zeros_like(s)], 0)                                       # ... beside an item silent throughout
    kw = _kw(n_fft, hop)
    p, parents = si.phase_vocoder(both.to(DEV), rate, phase_lock=LOCK, return_parents=True, **kw)
    p, parents = p.cpu(), parents.cpu()
    assert torch.isfinite(torch.view_as_real(p)).all()
    t = torch.arange(p.shape[-1], dtype=F64) * rate
    i = torch.floor(t).long()
    sp = torch.cat([both, torch.zeros(2, s.shape[1], 2, dtype=s.dtype)], -1)
    silent = (sp[:, :, i] == 0) & (sp[:, :, i + 1] == 0)
    assert silent[0].any() and silent[1].all()
    assert (p[silent] == 0).all() and (parents[silent] == 3).all()
    alone = si.phase_vocoder(s.to(DEV), rate, phase_lock=LOCK, **kw).cpu()
    assert torch.equal(torch.view_as_real(alone[0]), torch.view_as_real(p[0]))
    ref, gate = _gate32(s, rate, n_fft, hop)
    assert max_err(alone, ref) <= gate


def test_rate_one_returns_the_input():
    s = _harmonic().unsqueeze(0)
    ref, gate = _gate32(s, 1.0, 512, 128)
    p = si.phase_vocoder(s.to(DEV), 1.0, phase_lock=LOCK, **_kw(512, 128))
    print(f"rate 1: error against the oracle {max_err(p, ref):.2e}, against the input {max_err(p, s):.2e}, gate {gate:.2e}")
    assert p.shape == s.shape and max_err(p, ref) <= gate


def _wave(name, frames=60, hop=128, batch=2):
    return torch.stack([signal(name, hop * frames, seed=5 + b) for b in range(batch)]).to(F32).to(DEV)


@pytest.mark.parametrize("max_iter", [0, 5])
def test_time_stretch_is_the_composition(max_iter):
    n_fft, hop, rate = 512, 128, 0.8
    x = _wave("chirp")
    kw = _kw(n_fft, hop)
    y = si.time_stretch(x, rate, n_fft, max_iter=max_iter, phase_lock=LOCK, verbose=False, **kw)
    p = si.phase_vocoder(si.stft(x, n_fft, **kw), rate, phase_lock=LOCK, **kw)
    y2 = si.istft(p, **kw) if max_iter == 0 else si.accelerated_griffin_lim(p, max_iter=max_iter, verbose=False, **kw)
    assert y.dtype == F32 and y.device.type == "cuda" and y.shape == (2, (si.stretched_frames(61, rate) - 1) * hop)
    assert torch.equal(y, y2)
    for lock in (None, "identity"):
        assert not torch.equal(y, si.time_stretch(x, rate, n_fft, max_iter=max_iter, phase_lock=lock, verbose=False, **kw))
    # lock_tol is handed on
    y3 = si.time_stretch(x, rate, n_fft, max_iter=max_iter, phase_lock=LOCK, lock_tol=0.3, verbose=False, **kw)
    p3 = si.phase_vocoder(si.stft(x, n_fft, **kw), rate, phase_lock=LOCK, lock_tol=0.3, **kw)
    y4 = si.istft(p3, **kw) if max_iter == 0 else si.accelerated_griffin_lim(p3, max_iter=max_iter, verbose=False, **kw)
    assert torch.equal(y3, y4) and not torch.equal(y3, y)


def test_pitch_shift_and_time_stretch_hpss_are_their_compositions():
    n_fft, hop, sr = 256, 64, 16000
    x = _wave("harmonic", frames=64, hop=64)
    kw = dict(n_fft=n_fft, max_iter=4, hop_length=hop, window=torch.hann_window(n_fft), verbose=False)
    z = si.pitch_shift(x, sr, 3, phase_lock=LOCK, **kw)
    rate, orig = si.timescale.shift_rate(sr, 3)
    y = si.resample(si.time_stretch(x, rate, phase_lock=LOCK, **kw), orig, sr)
    n = x.shape[-1]
    want = y[..., :n] if y.shape[-1] >= n else torch.nn.functional.pad(y, (0, n - y.shape[-1]))
    assert z.shape == x.shape and torch.equal(z, want)
    assert not torch.equal(z, si.pitch_shift(x, sr, 3, phase_lock="identity", **kw))
    # time_stretch_hpss: the harmonic branch takes the mode; without the keyword it is identity locking as before
    hk = dict(hop_length=hop, window=torch.hann_window(n_fft))
    h = si.time_stretch_hpss(x, 0.8, n_fft, max_iter=3, phase_lock=LOCK, **hk)
    x_h, x_p = si.hpss_audio(x, n_fft, 31, 2.0, 1.0, 0, **hk)
    y_h = si.time_stretch(x_h, 0.8, n_fft, 3, "accelerated_griffin_lim", phase_lock=LOCK, **hk)
    assert torch.equal(h, y_h + si.ola(x_p, 0.8, 256, None, length=y_h.shape[-1]))
    plain = si.time_stretch_hpss(x, 0.8, n_fft, max_iter=3, **hk)
    assert torch.equal(plain, si.time_stretch_hpss(x, 0.8, n_fft, max_iter=3, phase_lock="identity", **hk))
    y_i = si.time_stretch(x_h, 0.8, n_fft, 3, "accelerated_griffin_lim", phase_lock="identity", **hk)
    assert torch.equal(plain, y_i + si.ola(x_p, 0.8, 256, None, length=y_i.shape[-1])) and not torch.equal(plain, h)


def _device_inconsistency(name, rate, lock):
    n_fft, hop = 512, 128
    s, w = signal_spec(name, n_fft, hop, 64)
    p = si.phase_vocoder(s.to(torch.complex64).to(DEV), rate, phase_lock=lock, **_kw(n_fft, hop))
    return inconsistency(p, n_fft, hop, w)


@pytest.mark.parametrize("rate", [0.5, 0.8])
def test_pghi_halves_the_inconsistency_on_the_device(rate):
    unlocked, pghi = _device_inconsistency("harmonic", rate, None), _device_inconsistency("harmonic", rate, LOCK)
    print(f"harmonic rate {rate}: inconsistency {unlocked:.3f} unlocked, {pghi:.3f} pghi ({pghi / unlocked:.2f} x)")
    assert pghi <= 0.5 * unlocked


@pytest.mark.parametrize("name", ["chirp", "noise"])
@pytest.mark.parametrize("rate", [0.8, 1.25])
def test_pghi_beats_identity_locking_on_the_device(name, rate):
    identity, pghi = _device_inconsistency(name, rate, "identity"), _device_inconsistency(name, rate, LOCK)
    print(f"{name} rate {rate}: inconsistency {identity:.3f} identity, {pghi:.3f} pghi ({pghi / identity:.2f} x)")
    assert pghi <= 0.8 * identity


def test_layouts_and_limits():
    n_fft, hop, rate = 512, 128, 1.25
    s = torch.stack([_harmonic(), _harmonic().flip(0) * 0.5])
    kw = _kw(n_fft, hop)
    n_out = si.stretched_frames(64, rate)
    batched, bp = si.phase_vocoder(s.to(DEV), rate, phase_lock=LOCK, return_parents=True, **kw)
    one, op = si.phase_vocoder(s[1].to(DEV), rate, phase_lock=LOCK, return_parents=True, **kw)   # unbatched in, unbatched out
    assert one.shape == op.shape == (257, n_out) and one.dtype == torch.complex64 and one.device.type == "cuda"
    assert torch.equal(torch.view_as_real(batched[1]), torch.view_as_real(one)) and torch.equal(bp[1], op)
    cpu, cp = si.phase_vocoder(s, rate, phase_lock=LOCK, return_parents=True, **kw)               # a CPU tensor in, CPU tensors out
    assert cpu.device.type == cp.device.type == "cpu"
    assert torch.equal(torch.view_as_real(cpu), torch.view_as_real(batched.cpu())) and torch.equal(cp, bp.cpu())
    half = si.phase_vocoder(s.to(torch.complex32).to(DEV), rate, phase_lock=LOCK, **kw)
    assert half.dtype == torch.complex32 and half.shape == batched.shape
    # a strided torch.stft output as it comes, and a lazily conjugated tensor
    x = _wave("harmonic", frames=63)
    raw = torch.stft(x, n_fft, hop_length=hop, window=kw["window"].to(DEV), return_complex=True)
    assert not raw.is_contiguous()
    assert torch.equal(torch.view_as_real(si.phase_vocoder(raw, rate, phase_lock=LOCK, **kw)),
                       torch.view_as_real(si.phase_vocoder(raw.contiguous(), rate, phase_lock=LOCK, **kw)))
    lazy = s.to(DEV).conj()
    assert lazy.is_conj()
    assert torch.equal(torch.view_as_real(si.phase_vocoder(lazy, rate, phase_lock=LOCK, **kw)),
                       torch.view_as_real(si.phase_vocoder(lazy.resolve_conj(), rate, phase_lock=LOCK, **kw)))
    assert not torch.equal(torch.view_as_real(si.phase_vocoder(lazy, rate, phase_lock=LOCK, **kw)), torch.view_as_real(batched))
    with pytest.raises(NotImplementedError, match="not differentiable"):
        si.phase_vocoder(s.to(DEV).requires_grad_(True), rate, phase_lock=LOCK, **kw)
    with torch.no_grad():
        si.phase_vocoder(s.to(DEV).requires_grad_(True), rate, phase_lock=LOCK, **kw)
    with pytest.raises(NotImplementedError, match="2915"):
        si.phase_vocoder(torch.zeros(2916, 3, dtype=torch.complex64, device=DEV), rate, phase_lock=LOCK, hop_length=100)


def test_more_items_than_the_grid_holds():
    """65 536 workgroups loop over 70 000 items: seven distinct items tiled, every copy must carry its original's bits"""
    s, n_fft, hop, (_, _, codes) = _case((5, 4, 0.8, F32))
    more = torch.from_numpy(random_spec(5, 4, seed=77, batch=4, dtype=np.complex64))
    seven = torch.cat([s, more])
    want, wp = si.phase_vocoder(seven.to(DEV), 0.8, phase_lock=LOCK, return_parents=True, hop_length=hop)
    assert np.array_equal(wp[:3].cpu().numpy(), codes)
    big = seven.to(DEV).repeat(10000, 1, 1)
    got, gp = si.phase_vocoder(big, 0.8, phase_lock=LOCK, return_parents=True, hop_length=hop)
    assert got.shape == (70000, 5, 5)
    assert torch.equal(torch.view_as_real(got), torch.view_as_real(want.repeat(10000, 1, 1))) and torch.equal(gp, wp.repeat(10000, 1, 1))
    with pytest.raises(ValueError, match="at most 65535"):
        si.phase_vocoder(big, 0.8, phase_lock="identity", hop_length=hop)


def test_a_call_between_two_pushes_of_a_running_stream_changes_nothing():
    kw = dict(look_ahead=1, max_iter=2, hop_length=32, window=torch.hann_window(128), device=torch.device(DEV, 0))
    g = torch.Generator().manual_seed(4)
    mag = (torch.rand((1, 65, 12), generator=g) + 0.05).to(DEV)
    a = si.RTISIStream(65, **kw)
    want = torch.cat([a.push(mag[:, :, :5]), a.push(mag[:, :, 5:]), a.flush()], 1)
    b = si.RTISIStream(65, **kw)
    first = b.push(mag[:, :, :5])
    si.phase_vocoder(torch.polar(mag, mag * 3), 0.8, phase_lock=LOCK, hop_length=32)
    got = torch.cat([first, b.push(mag[:, :, 5:]), b.flush()], 1)
    assert torch.equal(got, want)
