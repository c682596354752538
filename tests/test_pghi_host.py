"""rtpghi without a GPU: the definition (tests/_pghi_oracle.py) against a literal heap, its tie rule on hand-worked frames, its
gradient formulas against the phase of `torch.stft`, and the argument errors of `rtpghi` and of specinv_pghi, all raised before the
device is touched."""
import ctypes as C

import numpy as np
import pytest
import torch

import spectrogram_inversion_amd as si
from _pghi_oracle import HANN_GAMMA, assert_distinct, definition, gradients, heap, random_magnitudes, wrapped
from spectrogram_inversion_amd import _lib, build, pghi

SHAPES = ((2, 3), (3, 1), (5, 4), (65, 6), (129, 5), (257, 7), (1025, 3))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_the_definition_is_the_heaps_result(shape):
    """identical parents and identical phases (equal, not close): both sum the same terms in the same order"""
    F, T = shape
    n_fft = 2 * (F - 1)
    s = random_magnitudes(F, T, 7 * F + T, batch=3)
    assert len({float(item.max()) for item in s}) == 3
    for item in s:
        assert_distinct(item)
        assert (item == 0).sum() >= (F * T) // 20 or F * T < 100
        ph_d, par_d = definition(item, n_fft, max(1, n_fft // 4), HANN_GAMMA * n_fft ** 2)
        ph_h, par_h = heap(item, n_fft, max(1, n_fft // 4), HANN_GAMMA * n_fft ** 2)
        assert np.array_equal(par_d, par_h)
        assert np.array_equal(ph_d, ph_h)
        assert ((par_d == 3) == ~((item > 0) & (item >= 1e-6 * item.max()))).all()
        assert (ph_d[par_d == 3] == 0).all()


def test_the_tie_rule_on_hand_worked_frames():
    """F = 5 (n_fft 8), magnitudes in eighths.  Worked by hand from the two recurrences:

    frame 0, s = 1 2 2 1 .5: the seed is bin 1, the lower of the two maxima (p = +inf).  Lf = -inf -inf 2 2 1, Rg = 2 -inf -inf -inf
      -inf: bin 0 hangs off bin 1 from the right (2), bins 2, 3, 4 off their left neighbours (1 1 1).
    frame 1, s = 2 1 2 1 1, p = 1 2 2 1 .5: Lf = -inf 1 1 2 1, Rg = 1 2 1 .5 -inf.  Bin 0 has p = Rg = 1 and bin 1 has p = Rg = 2: the
      time direction wins both ties (0 0); bin 2 has p = 2 above both (0); bin 3 has Lf = 2 > p (1); bin 4 has Lf = 1 > p = .5 (1).
    frame 2, s = 4 4 4 0 0, p = 2 1 2 1 1: Lf = -inf 2 2, Rg = 2 2 -inf.  Bin 1 has p = 1 < Lf = Rg = 2: the lower neighbour wins the
      tie (1); bins 0 and 2 have p = 2 equal to what reaches them through bin 1 (0 0); bins 3, 4 are silent (3 3).
    frame 3, s = 0 0 1 1 1, p = 4 4 4 -inf -inf: bins 0, 1 silent (3 3); bin 2 by time (0); bins 3, 4 have only Lf = 1 (1 1)."""
    s = np.array([[1, 2, 2, 1, .5], [2, 1, 2, 1, 1], [4, 4, 4, 0, 0], [0, 0, 1, 1, 1]]).T
    ph, par = definition(s, 8, 2, HANN_GAMMA * 64)
    assert par.T.tolist() == [[2, 0, 1, 1, 1], [0, 0, 0, 1, 1], [0, 1, 0, 3, 3], [3, 3, 0, 1, 1]]
    assert ph[1, 0] == 0 and (ph[3:, 2] == 0).all() and (ph[:2, 3] == 0).all()
    _, wt, wf = gradients(s, 8, 2, HANN_GAMMA * 64)
    assert ph[0, 0] == ph[1, 0] - (wf[1, 0] + wf[0, 0]) / 2 and ph[2, 0] == ph[1, 0] + (wf[1, 0] + wf[2, 0]) / 2
    assert ph[2, 3] == ph[2, 2] + (wt[2, 2] + wt[2, 3]) / 2
    # a bin the previous frame cannot reach starts from that frame's phase 0, and all three being -inf is the time direction
    lone = np.array([[1.0, 0, 0, 0, 0], [0, 0, 0, 0, 1.0]]).T
    ph, par = definition(lone, 8, 2, HANN_GAMMA * 64)
    assert par.T.tolist() == [[0, 3, 3, 3, 3], [3, 3, 3, 3, 0]]
    _, wt, _ = gradients(lone, 8, 2, HANN_GAMMA * 64)
    assert ph[4, 1] == (wt[4, 0] + wt[4, 1]) / 2


def test_silence_and_one_frame():
    ph, par = definition(np.zeros((5, 3)), 8, 2, 16.0)
    assert (par == 3).all() and (ph == 0).all()
    s = random_magnitudes(9, 1, 5)
    _, wt, wf = gradients(s, 16, 4, HANN_GAMMA * 256)
    assert (wf == np.pi).all()                                          # T = 1: D = 0
    ph, par = definition(s, 16, 4, HANN_GAMMA * 256)
    assert ph[int(np.argmax(s[:, 0])), 0] == 0


def test_the_gradient_formulas_are_the_phase_differences_of_torch_stft():
    """Two crossing chirps analysed with a true Gaussian window exp(-pi (j - N/2)^2 / gamma), N 512, hop 64, gamma 0.08 N^2 (4e-4
    at the frame's ends), 48 frames.  On neighbouring bins above 1 % of the maximum, away from the four padded frames at either
    end, the trapezoid steps (wt + wt) / 2 and (wf + wf) / 2 are the wrapped phase differences of `torch.stft` along time and along
    frequency.  Observed 95th percentiles of the error: 0.0075 rad along time (968 pairs), 0.0244 rad along frequency (1100 pairs);
    the bounds are twice those.  A wrong sign gives 2.7 and 3.0 rad, a missing pi 3.14."""
    N, a, T = 512, 64, 48
    gamma = 0.08 * N * N
    w = torch.from_numpy(np.exp(-np.pi * (np.arange(N) - N / 2) ** 2 / gamma))
    n = (T - 1) * a
    t = np.arange(n)
    x = np.sin(2 * np.pi * (0.05 * t + 0.5 * (0.25 / n) * t * t)) + 0.5 * np.sin(2 * np.pi * (0.4 * t - 0.5 * (0.2 / n) * t * t) + 1.0)
    S = torch.stft(torch.from_numpy(x), N, hop_length=a, window=w, return_complex=True).numpy()
    mag, ph = np.abs(S), np.angle(S)
    _, wt, wf = gradients(mag, N, a, gamma)
    big = mag > 0.01 * mag.max()
    big[:, :4] = big[:, -4:] = False
    along_t = np.abs(wrapped(ph[:, 1:] - ph[:, :-1] - (wt[:, 1:] + wt[:, :-1]) / 2))[big[:, 1:] & big[:, :-1]]
    along_f = np.abs(wrapped(ph[1:] - ph[:-1] - (wf[1:] + wf[:-1]) / 2))[big[1:] & big[:-1]]
    assert along_t.size > 500 and along_f.size > 500
    print(f"95th percentiles: time {np.percentile(along_t, 95):.4f}, frequency {np.percentile(along_f, 95):.4f}")
    assert np.percentile(along_t, 95) <= 2 * 0.0075
    assert np.percentile(along_f, 95) <= 2 * 0.0244


def test_argument_errors_come_before_the_device():
    s = torch.ones(5, 4)
    for bad in (torch.ones(5, 4, dtype=torch.complex64), torch.ones(5, 4, dtype=torch.int32), np.ones((5, 4)), None):
        with pytest.raises(TypeError):
            si.rtpghi(bad)
    with pytest.raises(NotImplementedError, match="one-sided"):
        si.rtpghi(torch.ones(8, 4), onesided=False)
    with pytest.raises(NotImplementedError, match="one-sided"):
        si.rtpghi(torch.ones(8, 4), window=torch.ones(8, dtype=torch.complex64))
    with pytest.raises(NotImplementedError, match="even n_fft"):
        si.rtpghi(s, n_fft=9)
    with pytest.raises(NotImplementedError, match="limit"):
        si.rtpghi(torch.ones(2916, 2))
    with pytest.raises(NotImplementedError, match="rtpghi is not differentiable; detach the input"):
        si.rtpghi(torch.ones(5, 4, requires_grad=True))
    for gamma in (0, 0.0, -1.0, float("inf"), float("nan"), "1", True):
        with pytest.raises(ValueError, match="gamma"):
            si.rtpghi(s, gamma=gamma)
    for tol in (0, 0.0, 1, 1.0, float("nan"), -1e-6, 2.0, None, "1e-6", True):
        with pytest.raises(ValueError, match="tol"):
            si.rtpghi(s, tol=tol)
    for shape in ((5,), (2, 2, 5, 4), (), (3, 0, 4), (3, 5, 0), (1, 4)):
        with pytest.raises(ValueError):
            si.rtpghi(torch.ones(shape))
    for n_fft in (10, 6, 0, 8.0):
        with pytest.raises(ValueError, match="n_fft"):
            si.rtpghi(s, n_fft=n_fft)
    with torch.no_grad():                                               # (not under grad mode; an empty batch needs no device)
        e = si.rtpghi(torch.zeros(0, 5, 4, requires_grad=True), return_phase=True, return_parents=True)
    assert e[0].shape == e[1].shape == e[2].shape == (0, 5, 4)
    assert e[0].dtype == torch.complex64 and e[1].dtype == torch.float64 and e[2].dtype == torch.int8


def test_exports():
    assert callable(si.rtpghi) and si.rtpghi is pghi.rtpghi and "rtpghi" in pghi.__all__
    assert pghi.HANN_GAMMA == HANN_GAMMA


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def test_abi_argument_errors_do_not_need_a_gpu(lib):
    assert lib.specinv_abi_version() == 1
    buf = (C.c_double * 96)()
    p, q = C.addressof(buf), C.addressof(buf) + 256
    nan, inf = float("nan"), float("inf")

    def call(mag=p, spec_out=q, phase_out=None, parents_out=None, batch=1, n_freq=5, n_frames=3, n_fft=8, hop=2, gamma=16.0, tol=1e-6,
             dtype=_lib.F32):
        return lib.specinv_pghi(mag, spec_out, phase_out, parents_out, batch, n_freq, n_frames, n_fft, hop, gamma, tol, dtype, 0, None)

    for kw, word in ((dict(mag=None), b"NULL mag"), (dict(spec_out=None), b"NULL spec_out"), (dict(spec_out=p), b"alias"),
                     (dict(batch=0), b"batch"), (dict(n_freq=0), b"batch"), (dict(n_frames=-1), b"batch"),
                     (dict(n_fft=9), b"n_fft"), (dict(n_fft=0, n_freq=1), b"n_fft"), (dict(n_fft=10), b"n_fft"), (dict(n_freq=4), b"n_fft"),
                     (dict(hop=0), b"hop"), (dict(hop=-2), b"hop"),
                     (dict(gamma=0.0), b"gamma"), (dict(gamma=-1.0), b"gamma"), (dict(gamma=inf), b"gamma"), (dict(gamma=nan), b"gamma"),
                     (dict(tol=0.0), b"tol"), (dict(tol=1.0), b"tol"), (dict(tol=nan), b"tol"), (dict(tol=-0.5), b"tol"),
                     (dict(dtype=7), b"dtype"),
                     # the documented order: the earlier error is the one reported
                     (dict(mag=None, spec_out=None), b"NULL mag"), (dict(spec_out=p, batch=0), b"alias"),
                     (dict(batch=0, n_fft=9), b"batch"), (dict(n_fft=9, hop=0), b"n_fft"), (dict(hop=0, gamma=0.0), b"hop"),
                     (dict(gamma=0.0, tol=0.0), b"gamma"), (dict(tol=0.0, dtype=7), b"tol")):
        assert call(**kw) == _lib.EINVAL, kw
        assert word in lib.specinv_last_error(), (kw, lib.specinv_last_error())
    # above the size limit: unsupported, after every argument error and still before the device
    assert call(n_fft=5830, n_freq=2916) == _lib.EUNSUPPORTED
    assert call(n_fft=5830, n_freq=2916, dtype=7) == _lib.EINVAL
