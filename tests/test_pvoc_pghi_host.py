"""phase_lock="pghi" without a GPU: the definition's restatement (tests/_pvoc_pghi_oracle.py) alone - the literal heap against the scan
definition, hand-worked frames with their codes written out, rate 1, what the mode is worth on four signals - and the argument
errors that are raised before the device is touched."""
import ctypes as C

import numpy as np
import pytest
import torch

import spectrogram_inversion_amd as si
from _pvoc_lock_torch import inconsistency, lock_ref
from _pvoc_pghi_oracle import frame_codes, frame_codes_heap, pghi_heap, pghi_ref, random_spec, roots, signal_spec
from _pvoc_torch import pvoc_ref
from spectrogram_inversion_amd import _lib, build

RATES = (0.5, 0.8, 1.0, 1.25, 2.3)


@pytest.mark.parametrize("n_fft,hop,frames", [(8, 2, 40), (128, 32, 24), (512, 128, 10)])
def test_heap_equals_definition(n_fft, hop, frames):
    """identical codes and bit-identical psi on distinct magnitudes; and no code-1 bin hangs off a code-2 bin: with k - 1 of code 2
    (Rg[k-1] > p[k-1], Lf[k-1]) and k of code 1 (Lf[k] > p[k], Lf[k] >= Rg[k]) one gets Lf[k] <= max(p[k-1], Lf[k-1]) < Rg[k-1]
    <= max(p[k], Rg[k]) <= Lf[k], so the order in which the two kinds of chain are resolved never decides anything"""
    F = n_fft // 2 + 1
    s = random_spec(F, frames, seed=n_fft, batch=2)
    for item in s:
        v = np.abs(item)[np.abs(item) > 0]
        assert np.unique(v).size == v.size
    seen = set()
    for rate in RATES:
        _, psi_d, codes_d = pghi_ref(s, rate, n_fft, hop)
        _, psi_h, codes_h = pghi_heap(s, rate, n_fft, hop)
        assert np.array_equal(codes_d, codes_h), f"rate {rate}: {int((codes_d != codes_h).sum())} parents differ"
        assert np.array_equal(psi_d.view(np.int64), psi_h.view(np.int64))
        assert not ((codes_d[:, 1:] == 1) & (codes_d[:, :-1] == 2)).any()
        seen |= set(np.unique(codes_d).tolist())
    assert seen == {0, 1, 2, 3}


# Hand-worked frames: n_fft 32 one-sided (F = 17), rate 1 (a = 0 and m = r exactly), integer magnitudes times five on the twelve
# integer directions of tests/_pvoc_lock_torch.py's comb, a frame per row, and the codes they must give.
HAND_N_FFT, HAND_HOP = 32, 8
HAND_MAG = [
    [5, 9, 1, 6, 1, 6, 0, 0, 0, 3, 3, 3, 0, 2, 7, 2, 0],
    [9, 1, 8, 8, 4, 8, 0, 4, 0, 2, 0, 5, 1, 1, 1, 1, 1],
    [1, 2, 9, 7, 0, 3, 5, 6, 0, 3, 6, 9, 7, 6, 5, 4, 2],
    [0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    [3, 0, 2, 5, 4, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 6],
]
HAND_CODES = [
    # frame 0: live bins are their own roots
    [0, 0, 0, 0, 0, 0, 3, 3, 3, 0, 0, 0, 3, 0, 0, 0, 3],
    # bin 2: p 1, Lf 1, Rg 6 -> 2.  bin 4: p 1, Lf = Rg = 6, a tie that code 1 wins.  bin 7: live, no live neighbour and dead a frame
    # ago, all three -inf -> 0.  bins 6, 8 and 10 are dead between live runs.  bins 12 and 16: dead a frame ago, reached from the left.
    [0, 0, 2, 0, 1, 0, 3, 0, 3, 0, 3, 0, 1, 0, 0, 0, 1],
    # bin 3: p = Lf = 8 (bin 2: p 8, c 9), a tie that time wins.  bins 9, 10: a chain of code 2 to the root 11, which also carries
    # the chain of code 1 through bins 12 .. 16 (Lf 5, 5, 5, 5, 4 against p 1).  bin 1: Rg 8 from bin 2.  bin 6: Lf 3 < Rg 4.
    [0, 2, 0, 0, 3, 0, 2, 0, 3, 2, 2, 0, 1, 1, 1, 1, 1],
    # silence
    [3] * 17,
    # after silence every p is -inf, so is every Lf and Rg: every live bin starts again from its own phase
    [0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
]
HAND_ROOTS = [
    list(range(17)),
    [0, 1, 3, 3, 3, 5, 6, 7, 8, 9, 10, 11, 11, 13, 14, 15, 15],
    [0, 2, 2, 3, 4, 5, 7, 7, 8, 11, 11, 11, 11, 11, 11, 11, 11],
    list(range(17)),
    list(range(17)),
]


def hand_spec(dtype=torch.complex128, seed=11):
    g = torch.Generator().manual_seed(seed)
    mag = torch.tensor(HAND_MAG, dtype=torch.float64).T
    dirs = torch.tensor([(5, 0), (-5, 0), (0, 5), (0, -5), (3, 4), (3, -4), (-3, 4), (-3, -4), (4, 3), (4, -3), (-4, 3), (-4, -3)],
                        dtype=torch.float64)
    pick = dirs[torch.randint(0, 12, mag.shape, generator=g)]
    return torch.complex(mag * pick[..., 0], mag * pick[..., 1]).to(dtype)


def test_hand_worked_frames():
    """(the issue also names "a code-1 chain hanging off a code-2 bin": no input gives one - see test_heap_equals_definition - so
    the nearest thing stands here, a root that carries a chain of code 2 on its left and a chain of code 1 on its right)"""
    s = hand_spec()
    assert torch.equal(s.abs(), 5 * torch.tensor(HAND_MAG, dtype=torch.float64).T)
    want = np.array(HAND_CODES, np.int8).T
    P, psi, codes = pghi_ref(s, 1.0, HAND_N_FFT, HAND_HOP)
    assert np.array_equal(codes, want)
    mag = 5.0 * np.array(HAND_MAG, np.float64)
    for j in range(1, 5):                                        # frame by frame, and the heap where no tie decides
        c = np.where(mag[j] > 0, mag[j], -np.inf)
        p = np.where(mag[j - 1] > 0, mag[j - 1], -np.inf)
        assert frame_codes(c, p).tolist() == HAND_CODES[j]
        assert roots(np.array(HAND_CODES[j])).tolist() == HAND_ROOTS[j]
    assert frame_codes_heap(np.where(mag[4] > 0, mag[4], -np.inf), np.full(17, -np.inf)).tolist() == HAND_CODES[4]
    # psi from the roots written out above
    th = np.angle(s.numpy())
    adv = (2 * np.pi * np.arange(17) * HAND_HOP / HAND_N_FFT)[:, None]
    d = np.concatenate([th[:, 1:], np.zeros((17, 1))], 1) - th - adv
    d = d - 2 * np.pi * np.round(d / (2 * np.pi)) + adv
    expect = np.empty_like(th)
    expect[:, 0] = th[:, 0]
    k = np.arange(17)
    for j in range(1, 5):
        phi = expect[:, j - 1] + d[:, j - 1]
        r = np.array(HAND_ROOTS[j])
        expect[:, j] = np.where(r == k, phi, (phi[r] - th[r, j]) + th[:, j])
    assert np.allclose(psi, expect, rtol=0, atol=1e-12)
    # ... in words: a dead bin keeps its time-propagated phase, silence is exact zeros, and at rate 1 the magnitude is the input's
    assert np.array_equal(np.abs(P[:, 3]), np.zeros(17)) and np.array_equal(P[:, 3].real, np.zeros(17))
    assert np.allclose(np.abs(P), mag.T, rtol=1e-14, atol=0)


@pytest.mark.parametrize("n_fft,hop,frames", [(128, 32, 90), (512, 128, 64)])
def test_rate_one_returns_the_input(n_fft, hop, frames):
    s, _ = signal_spec("harmonic", n_fft, hop, frames)
    P, _, _ = pghi_ref(s, 1.0, n_fft, hop)
    err = float(np.abs(P - s.numpy()).max() / np.abs(s.numpy()).max())
    print(f"pghi_ref at rate 1, {n_fft}/{hop}: max error {err:.2e}")
    assert P.shape == tuple(s.shape) and err <= 1e-11


def _three(name, rate, n_fft=512, hop=128, frames=64):
    s, w = signal_spec(name, n_fft, hop, frames)
    unlocked = inconsistency(pvoc_ref(s, rate, n_fft, hop), n_fft, hop, w)
    identity = inconsistency(lock_ref(s, rate, n_fft, hop), n_fft, hop, w)
    pghi = inconsistency(torch.from_numpy(pghi_ref(s, rate, n_fft, hop)[0]), n_fft, hop, w)
    print(f"{name} rate {rate}: inconsistency {unlocked:.3f} unlocked, {identity:.3f} identity, {pghi:.3f} pghi "
          f"({pghi / unlocked:.2f} x, {pghi / identity:.2f} x)")
    return unlocked, identity, pghi


@pytest.mark.parametrize("rate", [0.5, 0.8])
def test_pghi_halves_the_inconsistency_of_a_harmonic_signal(rate):
    unlocked, _, pghi = _three("harmonic", rate)
    assert pghi <= 0.5 * unlocked


@pytest.mark.parametrize("name", ["chirp", "noise"])
@pytest.mark.parametrize("rate", [0.8, 1.25])
def test_pghi_beats_identity_locking_on_noisy_signals(name, rate):
    _, identity, pghi = _three(name, rate)
    assert pghi <= 0.8 * identity


def test_python_argument_errors_come_before_the_device():
    s = hand_spec(torch.complex64)
    x = torch.zeros(2, 128 * 10)
    w = torch.hann_window(128)
    for bad in (0, 0.0, 1, 1.0, -1e-6, 1.5, float("nan"), float("inf"), True, "1e-6", None):
        for lock in (None, "identity", "pghi"):                  # checked on every call, whatever the mode
            with pytest.raises(ValueError, match="lock_tol"):
                si.phase_vocoder(s, 0.8, phase_lock=lock, lock_tol=bad, hop_length=HAND_HOP)
            with pytest.raises(ValueError, match="lock_tol"):
                si.time_stretch(x, 0.8, 128, phase_lock=lock, lock_tol=bad, hop_length=32, window=w)
            with pytest.raises(ValueError, match="lock_tol"):
                si.pitch_shift(x, 16000, 2, n_fft=128, phase_lock=lock, lock_tol=bad, hop_length=32, window=w)
        with pytest.raises(ValueError, match="lock_tol"):
            si.time_stretch_hpss(x, 0.8, 128, lock_tol=bad, hop_length=32, window=w)
    for lock in (None, "identity"):
        with pytest.raises(ValueError, match="return_parents"):
            si.phase_vocoder(s, 0.8, phase_lock=lock, return_parents=True, hop_length=HAND_HOP)
    for bad in ("PGHI", "heap", 2):
        with pytest.raises(ValueError, match="'identity' or 'pghi'"):
            si.phase_vocoder(s, 0.8, phase_lock=bad, hop_length=HAND_HOP)
        with pytest.raises(ValueError, match="'identity' or 'pghi'"):
            si.time_stretch_hpss(x, 0.8, 128, phase_lock=bad, hop_length=32, window=w)
    two = torch.zeros(32, 5, dtype=torch.complex64)
    with pytest.raises(NotImplementedError, match="one-sided"):
        si.phase_vocoder(two, 0.8, phase_lock="pghi", hop_length=8, onesided=False)
    with pytest.raises(NotImplementedError, match="one-sided"):
        si.phase_vocoder(two, 0.8, phase_lock="pghi", hop_length=8, window=torch.ones(32, dtype=torch.complex64))
    with pytest.raises(NotImplementedError, match="2915"):
        si.phase_vocoder(torch.zeros(2916, 3, dtype=torch.complex64), 0.8, phase_lock="pghi", hop_length=8)
    g = torch.zeros(17, 5, dtype=torch.complex64, requires_grad=True)
    with pytest.raises(NotImplementedError, match="not differentiable"):
        si.phase_vocoder(g, 0.8, phase_lock="pghi", hop_length=8)
    empty = si.phase_vocoder(torch.zeros(0, 17, 5, dtype=torch.complex64), 0.8, phase_lock="pghi", return_parents=True, hop_length=8)
    assert empty[0].shape == (0, 17, 7) and empty[1].shape == (0, 17, 7) and empty[1].dtype == torch.int8


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def test_abi_argument_errors_do_not_need_a_gpu(lib):
    buf = (C.c_double * 64)()
    p, q = C.addressof(buf), C.addressof(buf) + 256

    def call(spec_in=p, spec_out=q, parents=None, batch=1, n_freq=3, n_in=4, n_out=5, n_fft=4, hop=1, rate=0.8, tol=1e-6, dtype=0):
        return lib.specinv_pvoc_pghi(spec_in, spec_out, parents, batch, n_freq, n_in, n_out, n_fft, hop, rate, tol, dtype, 0, None)

    # every error alone, then each one in front of all those behind it in the header's order
    errors = [(dict(spec_in=None), b"spec_in"), (dict(spec_out=None), b"spec_out"), (dict(spec_out=p), b"alias"),
              (dict(batch=0), b"batch"), (dict(n_freq=0), b">= 1"), (dict(n_in=0), b"n_frames_in"), (dict(n_out=0), b"n_frames_out"),
              (dict(n_fft=0), b"n_fft must be >= 1"), (dict(n_freq=4), b"n_freq = n_fft / 2 + 1"), (dict(hop=0), b"hop"),
              (dict(rate=0.0), b"rate"), (dict(rate=-1.0), b"rate"), (dict(rate=float("inf")), b"rate"),
              (dict(rate=float("nan")), b"rate"), (dict(n_out=6), b"stretch to 5"), (dict(tol=0.0), b"tol"), (dict(tol=1.0), b"tol"),
              (dict(tol=float("nan")), b"tol"), (dict(dtype=7), b"dtype")]
    for kw, word in errors:
        assert call(**kw) == _lib.EINVAL, kw
        assert word in lib.specinv_last_error(), (kw, lib.specinv_last_error())
    order = [(dict(spec_in=None), b"spec_in"), (dict(spec_out=p), b"alias"), (dict(batch=0), b"batch"),
             (dict(n_freq=4), b"n_freq = n_fft / 2 + 1"), (dict(hop=0), b"hop"), (dict(rate=0.0), b"rate"),
             (dict(n_out=6), b"stretch to"), (dict(tol=2.0), b"tol"), (dict(dtype=7), b"dtype")]
    for at, (kw, word) in enumerate(order):
        later = {}
        for other, _ in order[at + 1:]:
            later.update(other)
        later.update(kw)
        assert call(**later) == _lib.EINVAL
        assert word in lib.specinv_last_error(), (at, lib.specinv_last_error())
    # beyond the kernel's bins: unsupported, after every argument error
    assert call(n_freq=2916, n_fft=5830) == _lib.EUNSUPPORTED
    assert b"2915" in lib.specinv_last_error()
    assert call(n_freq=2916, n_fft=5830, tol=0.0) == _lib.EINVAL
    assert lib.specinv_abi_version() == 1
    assert "specinv_pvoc_pghi" in _lib.SIGNATURES
