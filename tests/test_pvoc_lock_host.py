"""phase_lock="identity" without a GPU: the definition's restatement (tests/_pvoc_lock_torch.py) alone - rate 1, the mirror
symmetry of two-sided spectra, what locking is worth on a harmonic signal, a synthetic comb with its owners written out - and the
argument errors that are raised before the device is touched."""
import ctypes as C

import pytest
import torch

import spectrogram_inversion_amd as si
from _pvoc_lock_torch import (COMB_HOP, COMB_N_FFT, COMB_OWNER, _parts, comb_spec, harmonic_wave, inconsistency, lock_ref,
                              peaks_and_owners)
from _pvoc_torch import max_err, pvoc_ref
from spectrogram_inversion_amd import _lib, build

F64 = torch.float64


def _harmonic_spec(n_fft, hop, frames, batch=1, seed=5):
    x = harmonic_wave((frames - 1) * hop, batch, seed)
    w = torch.hann_window(n_fft, dtype=F64)
    s = torch.stft(x, n_fft, hop_length=hop, window=w, return_complex=True)
    assert s.shape[-1] == frames
    return s, w


def test_rate_one_returns_the_input():
    s, _ = _harmonic_spec(128, 32, 90, batch=2)
    p = lock_ref(s, 1.0, 128, 32)
    err = float(torch.linalg.norm(p - s) / torch.linalg.norm(s))
    print(f"lock_ref at rate 1: relative L2 {err:.2e}")
    assert p.shape == s.shape and err <= 1e-10


@pytest.mark.parametrize("rate", [0.8, 1.6])
def test_two_sided_result_mirrors_itself_and_holds_the_one_sided_one(rate):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(64 * 30, generator=g, dtype=F64)
    w = torch.hann_window(64, dtype=F64)
    two = torch.stft(x, 64, hop_length=16, window=w, onesided=False, return_complex=True)
    p = lock_ref(two, rate, 64, 16)
    err = max_err(p[1:32].flip(0).conj(), p[33:])
    print(f"rate {rate}: mirror symmetry {err:.2e}")
    assert err <= 1e-9
    assert max_err(p[:33], lock_ref(two[:33], rate, 64, 16)) == 0.0
    pk2, own2 = peaks_and_owners(two, rate, 64, 16)
    pk1, own1 = peaks_and_owners(two[:33], rate, 64, 16)
    assert pk2.any() and torch.equal(pk2[:33], pk1) and torch.equal(own2[:33], own1)


@pytest.mark.parametrize("n_fft,hop,frames", [(128, 32, 150), (512, 128, 120)])
@pytest.mark.parametrize("rate", [0.5, 0.8])
def test_locking_halves_the_inconsistency_of_a_harmonic_signal(n_fft, hop, frames, rate):
    s, w = _harmonic_spec(n_fft, hop, frames)
    unlocked = inconsistency(pvoc_ref(s, rate, n_fft, hop), n_fft, hop, w)
    locked = inconsistency(lock_ref(s, rate, n_fft, hop), n_fft, hop, w)
    print(f"{n_fft}/{hop} rate {rate}: inconsistency {unlocked:.3f} unlocked, {locked:.3f} locked ({locked / unlocked:.2f} x)")
    assert locked <= 0.5 * unlocked


@pytest.mark.parametrize("rate", [1.0, 0.5])
def test_comb_owners_and_phase(rate):
    s = comb_spec()
    n_out = si.stretched_frames(s.shape[1], rate)
    src = [int(j * rate) for j in range(n_out)]                  # output frame j reads the peaks of input frame floor(j * rate)
    want = torch.tensor([COMB_OWNER[i] for i in src]).T
    peak, owner = peaks_and_owners(s, rate, COMB_N_FFT, COMB_HOP)
    assert torch.equal(owner, want)
    k = torch.arange(17)[:, None]
    assert torch.equal(peak, want == k)                          # a peak owns itself and nothing else does
    # psi from the owners written out above
    _, th0, _, phi = _parts(s, rate, COMB_N_FFT, COMB_HOP, F64)
    r = phi - th0
    expect = torch.where(want >= 0, torch.gather(r, 0, want.clamp(min=0)) + th0, phi)
    assert torch.equal(lock_ref(s, rate, COMB_N_FFT, COMB_HOP, return_phase=True), expect)
    # ... in words: at a peak the unlocked phase, elsewhere the peak's rotation applied to the bin's own analysis phase
    at_peak = want == k
    assert torch.allclose(expect[at_peak], phi[at_peak], rtol=0, atol=1e-12)
    none = want[0] < 0
    assert none.any() and torch.equal(expect[:, none], phi[:, none])


def test_python_argument_errors_come_before_the_device():
    s = comb_spec(torch.complex64)
    x = torch.zeros(2, 128 * 10)
    w = torch.hann_window(128)
    for bad in ("scaled", True, 1, "Identity", 0, ["identity"]):
        with pytest.raises(ValueError, match="phase_lock"):
            si.phase_vocoder(s, 0.8, phase_lock=bad, hop_length=COMB_HOP)
        with pytest.raises(ValueError, match="phase_lock"):
            si.time_stretch(x, 0.8, 128, phase_lock=bad, hop_length=32, window=w)
        with pytest.raises(ValueError, match="phase_lock"):
            si.pitch_shift(x, 16000, 2, n_fft=128, phase_lock=bad, hop_length=32, window=w)


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def test_abi_argument_errors_do_not_need_a_gpu(lib):
    buf = (C.c_double * 4)()
    p, q = C.addressof(buf), C.addressof(buf) + 16
    fn = lib.specinv_phase_vocoder_locked
    for mode in (0, 1):
        assert fn(None, p, 4, 1.0, mode, q) == _lib.EINVAL             # null plan, after every argument error
        assert b"plan is NULL" in lib.specinv_last_error()
        for bad in (0.0, -2.0, float("inf"), float("nan")):
            assert fn(None, p, 4, bad, mode, q) == _lib.EINVAL
            assert b"rate" in lib.specinv_last_error()
        assert fn(None, None, 4, 1.0, mode, q) == _lib.EINVAL
        assert b"spec_in" in lib.specinv_last_error()
        assert fn(None, p, 4, 1.0, mode, None) == _lib.EINVAL
        assert b"spec_out" in lib.specinv_last_error()
        assert fn(None, p, 0, 1.0, mode, q) == _lib.EINVAL
        assert b"n_frames_in" in lib.specinv_last_error()
        assert fn(None, p, 4, 1.0, mode, p) == _lib.EINVAL             # in place
        assert b"alias" in lib.specinv_last_error()
    for bad in (2, -1, 7):
        assert fn(None, p, 4, 1.0, bad, q) == _lib.EINVAL
        assert b"mode" in lib.specinv_last_error()
        assert fn(None, p, 4, 0.0, bad, q) == _lib.EINVAL               # the rate comes first
        assert b"rate" in lib.specinv_last_error()
    assert lib.specinv_abi_version() == 1
