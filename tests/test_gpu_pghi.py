"""rtpghi on the device against its definition in NumPy float64 (tests/_pghi_oracle.py) on the input's own bits.

Shapes (F, T): 2 bins, 3, 5 and 65 bins (fewer than a wave, and one more than a wave), 129 and 257 (one more than two waves' worth
and than a workgroup's lanes), 513 and 1025 at few frames, and 1537, 2049, 2561 and 2915 bins, the last the largest the kernel takes.  With a lane's chunk of bins
made odd, every one of them has a ragged last chunk and lanes without bins.  Batch 3 with the maxima 0.1, 1 and 10; a tenth of the
bins exact zeros, a seventh below the floor.

Bounds (none measured into being):
  parents: equal everywhere.  Every decision compares input values, and the inputs are distinct (asserted).
  phase: the wrapped difference on live bins is at most 16 times the largest wrapped difference between the oracle run in float64
    and run in numpy.longdouble, and at least 1e-12 rad.  That difference is the rounding noise of the definition itself; the factor
    covers the scan's order of summation and the device's logarithm (1 - 2 ulp).
  result: |out - s exp(i phi_oracle)| <= s (that phase tolerance + eps of the output dtype): a phase error d moves the unit vector
    by at most d, and one rounding of each component is at most eps / 2 of it.
"""
import math

import numpy as np
import pytest
import torch

import spectrogram_inversion_amd as si
from _pghi_oracle import HANN_GAMMA, assert_distinct, definition, gradients, random_magnitudes, wrapped
from _pvoc_lock_torch import harmonic_wave, inconsistency

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DEV = "cuda"
SHAPES = ((2, 3), (3, 1), (5, 4), (65, 6), (129, 5), (257, 7), (1025, 3), (513, 9), (1025, 4))


def stft_args(F):
    n_fft = 2 * (F - 1)
    return n_fft, max(1, n_fft // 4)


_REFS = {}


def oracle_item(sb, n_fft, hop, gamma, tol=1e-6):
    """(phase float64, parents, live, phase tolerance) of one item (F, T) float64: the definition in float64, and in longdouble for
    its rounding noise"""
    assert_distinct(sb)
    ph, par = definition(sb, n_fft, hop, gamma, tol)
    ph_l, par_l = definition(sb, n_fft, hop, gamma, tol, real=np.longdouble)
    assert np.array_equal(par, par_l)
    live = par != 3
    noise = float(np.abs(wrapped(ph_l - ph.astype(np.longdouble)))[live].max()) if live.any() else 0.0
    return ph, par, live, max(16 * noise, 1e-12)


def reference(F, T, dtype, batch=3):
    """(magnitudes as a CPU tensor of `dtype`, an `oracle_item` per item), made once"""
    key = (F, T, dtype, batch)
    if key not in _REFS:
        n_fft, hop = stft_args(F)
        s = torch.from_numpy(random_magnitudes(F, T, 1000 * F + T, batch)).to(dtype)
        _REFS[key] = (s, [oracle_item(s[b].double().numpy(), n_fft, hop, HANN_GAMMA * n_fft ** 2) for b in range(batch)])
    return _REFS[key]


def check(s, out, phase, parents, items):
    """one batch (B, F, T) of results against the oracle's items"""
    eps = torch.finfo(s.dtype).eps
    assert out.shape == s.shape and out.dtype == (torch.complex64 if s.dtype == F32 else torch.complex128)
    assert phase.shape == s.shape and phase.dtype == F64 and parents.shape == s.shape and parents.dtype == torch.int8
    for b, (ph, par, live, tol) in enumerate(items):
        assert np.array_equal(parents[b].cpu().numpy(), par), (b, int((parents[b].cpu().numpy() != par).sum()))
        d = np.abs(wrapped(phase[b].cpu().numpy() - ph))
        assert not live.any() or d[live].max() <= tol, (b, d[live].max(), tol)
        assert (phase[b].cpu().numpy()[~live] == 0).all()
        sb = s[b].double().numpy()
        want = sb * np.exp(1j * ph)
        got = out[b].cpu().to(torch.complex128).numpy()
        assert (np.abs(got - want) <= sb * (tol + eps)).all(), (b, float((np.abs(got - want) - sb * (tol + eps)).max()))
        # a bin that is not live returns (s, 0)
        assert np.array_equal(got[~live].real, sb[~live]) and (got[~live].imag == 0).all()


@pytest.mark.parametrize("dtype", (F32, F64), ids=("f32", "f64"))
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_parity_with_the_definition(shape, dtype):
    F, T = shape
    s, items = reference(F, T, dtype)
    n_fft, hop = stft_args(F)
    out, phase, parents = si.rtpghi(s.to(DEV), return_phase=True, return_parents=True, hop_length=hop)
    assert out.device.type == "cuda"
    check(s, out, phase, parents, items)
    # every code occurs where there is room for it
    if F * T >= 300:
        assert set(np.unique(parents.cpu().numpy())) == {0, 1, 2, 3}


@pytest.mark.parametrize("F", (1537, 2049, 2561, 2915))
def test_the_larger_chunks_up_to_the_largest_size_the_kernel_takes(F):
    """7, 9, 11 and 13 bins per lane (the kernel is instantiated per chunk size; the shapes above take 1, 3 and 5): n_fft 3072, 4096,
    5120 and the limit, 5828"""
    s, items = reference(F, 3, F64, batch=1)
    out, phase, parents = si.rtpghi(s.to(DEV), return_phase=True, return_parents=True, hop_length=stft_args(F)[1])
    check(s, out, phase, parents, items)
    if F == 2915:
        with pytest.raises(NotImplementedError):
            si.rtpghi(torch.ones(2916, 2, device=DEV))


def test_a_silent_item_next_to_a_normal_one():
    F, T = 65, 6
    s, items = reference(F, T, F32)
    both = torch.stack([torch.zeros(F, T), s[1]]).to(DEV)
    out, phase, parents = si.rtpghi(both, return_phase=True, return_parents=True, hop_length=stft_args(F)[1])
    assert (parents[0] == 3).all() and (phase[0] == 0).all() and (torch.view_as_real(out[0]) == 0).all()
    check(s[1:2], out[1:], phase[1:], parents[1:], items[1:2])


def test_after_a_silence_gap_the_time_direction_restarts_from_phase_zero():
    F, T = 65, 9
    n_fft, hop = stft_args(F)
    s = random_magnitudes(F, T, 77)
    s[:, 3:6] = 0.0
    assert_distinct(s)
    ph, par, _, tol = oracle_item(s, n_fft, hop, HANN_GAMMA * n_fft ** 2)
    live, wt, _ = gradients(s, n_fft, hop, HANN_GAMMA * n_fft ** 2)
    assert (par[:, 3:6] == 3).all() and set(np.unique(par[:, 6])) == {0, 3} and live[:, 6].sum() > 40
    restart = (wt[:, 5] + wt[:, 6]) / 2
    assert np.array_equal(ph[live[:, 6], 6], restart[live[:, 6]])         # the oracle alone: 0 + (wt + wt) / 2
    s1 = torch.from_numpy(s)[None]
    out, phase, parents = si.rtpghi(s1.to(DEV), return_phase=True, return_parents=True, hop_length=hop)
    check(s1, out, phase, parents, [(ph, par, par != 3, tol)])
    got = phase[0].cpu().numpy()[:, 6]
    assert np.abs(wrapped(got - restart))[live[:, 6]].max() <= tol
    assert (torch.view_as_real(out[0, :, 3:6]) == 0).all()


def test_one_frame_and_an_unbatched_input():
    F = 129
    s, items = reference(F, 1, F64)
    hop = stft_args(F)[1]
    out, phase, parents = si.rtpghi(s.to(DEV), return_phase=True, return_parents=True, hop_length=hop)
    check(s, out, phase, parents, items)
    s, items = reference(65, 6, F32)
    want = si.rtpghi(s[:1].to(DEV), return_phase=True, return_parents=True, hop_length=16)
    got = si.rtpghi(s[0].to(DEV), return_phase=True, return_parents=True, hop_length=16)
    assert got[0].shape == (65, 6) and got[1].shape == got[2].shape == (1, 65, 6)
    assert torch.equal(torch.view_as_real(got[0]), torch.view_as_real(want[0][0]))
    assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    assert torch.equal(torch.view_as_real(si.rtpghi(s[0].to(DEV), hop_length=16)), torch.view_as_real(got[0]))


def test_gamma_tol_and_the_windows_own_length():
    F, T = 65, 6
    s, _ = reference(F, T, F64)
    n_fft, hop = stft_args(F)
    sb = s[2].numpy()
    for kw, gamma, tol in ((dict(gamma=0.29794 * n_fft ** 2), 0.29794 * n_fft ** 2, 1e-6), (dict(), HANN_GAMMA * n_fft ** 2, 1e-3),
                           (dict(win_length=96), HANN_GAMMA * 96 ** 2, 1e-6),
                           (dict(win_length=100, window=torch.hann_window(100)), HANN_GAMMA * 100 ** 2, 1e-6)):
        ph, par, live, bound = oracle_item(sb, n_fft, hop, gamma, tol)
        _, phase, parents = si.rtpghi(s[2].to(DEV), tol=tol, return_phase=True, return_parents=True, hop_length=hop, **kw)
        assert np.array_equal(parents[0].cpu().numpy(), par), kw
        assert np.abs(wrapped(phase[0].cpu().numpy() - ph))[live].max() <= bound, kw


def test_a_cpu_tensor_a_side_stream_and_float16():
    s, _ = reference(65, 6, F32)
    want = si.rtpghi(s.to(DEV), hop_length=16)
    got = si.rtpghi(s, hop_length=16)
    assert got.device.type == "cpu" and torch.equal(torch.view_as_real(got), torch.view_as_real(want.cpu()))
    ph = si.rtpghi(s, return_phase=True, return_parents=True, hop_length=16)
    assert ph[1].device.type == "cpu" and ph[2].device.type == "cpu"
    stream = torch.cuda.Stream()
    sd = s.to(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        side = si.rtpghi(sd, hop_length=16)
    stream.synchronize()
    assert torch.equal(torch.view_as_real(side), torch.view_as_real(want))
    half = s.to(torch.float16)
    got = si.rtpghi(half.to(DEV), hop_length=16)
    wide = si.rtpghi(half.float().to(DEV), hop_length=16)
    assert got.dtype == torch.complex32
    assert torch.equal(torch.view_as_real(got), torch.view_as_real(wide).to(torch.float16))
    assert si.rtpghi(torch.zeros(0, 65, 6, device=DEV)).shape == (0, 65, 6)


def test_the_result_starts_griffin_lim_and_accelerated_griffin_lim():
    n_fft, hop, T = 512, 128, 8
    w = torch.hann_window(n_fft)
    x = harmonic_wave((T - 1) * hop, 2, 5).float()
    mag = torch.stft(x, n_fft, hop_length=hop, window=w, return_complex=True).abs().to(DEV)
    start = si.rtpghi(mag, hop_length=hop, window=w)
    for fn in (si.griffin_lim, si.accelerated_griffin_lim):
        y = fn(start, max_iter=1, verbose=False, hop_length=hop, window=w)
        assert y.shape == (2, (T - 1) * hop) and torch.isfinite(y).all() and y.abs().max() > 0


def test_a_call_between_two_steps_of_a_running_stream_changes_nothing():
    kw = dict(look_ahead=1, max_iter=2, hop_length=32, window=torch.hann_window(128), device=torch.device(DEV, 0))
    g = torch.Generator().manual_seed(4)
    mag = (torch.rand((1, 65, 12), generator=g) + 0.05).to(DEV)
    a = si.RTISIStream(65, **kw)
    want = torch.cat([a.push(mag[:, :, :5]), a.push(mag[:, :, 5:]), a.flush()], 1)
    b = si.RTISIStream(65, **kw)
    first = b.push(mag[:, :, :5])
    si.rtpghi(mag, hop_length=32)
    got = torch.cat([first, b.push(mag[:, :, 5:]), b.flush()], 1)
    assert torch.equal(got, want)


def test_it_is_more_consistent_than_phase_init():
    """512 / 128, 64 frames of the harmonic test signal.  The float64 oracle alone gives 0.111 on these magnitudes and the NumPy
    `phase_init` 0.554 (zero phase: 0.723), so the ordering holds for the definition before any kernel runs."""
    n_fft, hop, T = 512, 128, 64
    w = torch.hann_window(n_fft, dtype=F64)
    x = harmonic_wave((T - 1) * hop, 1, 3)[0]
    mag = torch.stft(x, n_fft, hop_length=hop, window=w, return_complex=True).abs()
    ph, _ = definition(mag.numpy(), n_fft, hop, HANN_GAMMA * n_fft ** 2)
    ours_oracle = inconsistency(mag * torch.exp(1j * torch.from_numpy(ph)), n_fft, hop, w)
    ours = inconsistency(si.rtpghi(mag.to(DEV), hop_length=hop, window=w), n_fft, hop, w)
    theirs = inconsistency(si.phase_init(mag.to(DEV), hop_length=hop, window=w), n_fft, hop, w)
    print(f"inconsistency: rtpghi {ours:.4f} (oracle {ours_oracle:.4f}), phase_init {theirs:.4f}")
    assert ours_oracle < theirs and ours < theirs
    assert math.isclose(ours, ours_oracle, rel_tol=1e-6)           # (the phases agree to 1e-9 rad and better)
