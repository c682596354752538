"""`gla_projection`, `stft`, `istft` without a GPU: the torch restatement the device tests compare against (tests/_proj_torch.py)
is pinned to the NumPy oracle; the adjoint recursion the fused kernel implements (csrc/kernels_proj_adjoint.h), written in torch
ops, is pinned to autograd of the restatement; and the argument errors are raised before a device is asked for."""
import numpy as np
import pytest
import torch

import _proj_torch as pt
import oracle
from _util import hann, rel_l2
from oracle import stftlib

import spectrogram_inversion_amd as si


def _case(n_fft, hop, frames, onesided, center, normalized, seed=0, batch=2):
    kw = dict(hop_length=hop, window=(pt.hamming if not center else hann)(n_fft, np.float64), onesided=onesided, center=center,
              normalized=normalized)
    F = n_fft // 2 + 1 if onesided else n_fft
    a = stftlib.args_helper(F, np.float64, **kw)
    L = stftlib.signal_length(frames, a)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((batch, L))
    mag = np.abs(stftlib.stft(rng.standard_normal((batch, L)), a)) * (0.5 + rng.random((batch, F, frames)))
    return x, mag, rng.standard_normal((batch, L)), kw, a


SWEEP = [(onesided, center, normalized) for onesided in (True, False) for center in (True, False) for normalized in (False, True)]


@pytest.mark.parametrize("onesided,center,normalized", SWEEP)
def test_restatement_is_the_oracle(onesided, center, normalized):
    """float64, 1e-12: the transforms against oracle/stftlib.py, the projection against one oracle.griffin_lim iteration at
    alpha = 0 (methods.py:241-248 without momentum) from a complex start."""
    x, mag, _, kw, a = _case(64, 16, 11, onesided, center, normalized)
    S = pt.stft(torch.from_numpy(x), mag.shape[1], **kw)
    assert rel_l2(S.numpy(), stftlib.stft(x, a)) <= 1e-12
    start = mag * np.exp(1j * np.random.default_rng(1).uniform(-np.pi, np.pi, mag.shape))
    x0 = pt.istft(torch.from_numpy(start), **kw)
    assert rel_l2(x0.numpy(), stftlib.istft(start, a)[0]) <= 1e-12
    y = pt.project(x0, torch.from_numpy(mag), **kw)
    ref = oracle.griffin_lim(start, max_iter=1, alpha=0.0, tol=0, **kw)
    assert y.shape == ref.shape and rel_l2(y.numpy(), ref) <= 1e-12


@pytest.mark.parametrize("onesided,center,normalized", SWEEP)
def test_adjoint_recursion_is_autograd_of_the_restatement(onesided, center, normalized):
    """64 / 16, float64, 1e-10 for x and for mag."""
    x, mag, w, kw, _ = _case(64, 16, 11, onesided, center, normalized)
    xt, mt = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(mag).requires_grad_(True)
    (pt.project(xt, mt, **kw) * torch.from_numpy(w)).sum().backward()
    g_x, g_m = pt.project_adjoint(torch.from_numpy(x), torch.from_numpy(mag), torch.from_numpy(w), **kw)
    ex, em = rel_l2(g_x.numpy(), xt.grad.numpy()), rel_l2(g_m.numpy(), mt.grad.numpy())
    print(f"onesided {onesided} center {center} normalized {normalized}: grad x {ex:.3e} grad mag {em:.3e}")
    assert ex <= 1e-10 and em <= 1e-10


@pytest.mark.parametrize("pad_mode", ["reflect", "constant", "replicate", "circular"])
def test_adjoint_recursion_folds_every_pad_mode(pad_mode):
    x, mag, w, kw, _ = _case(64, 16, 11, True, True, False)
    kw = dict(kw, pad_mode=pad_mode)
    xt, mt = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(mag).requires_grad_(True)
    (pt.project(xt, mt, **kw) * torch.from_numpy(w)).sum().backward()
    g_x, g_m = pt.project_adjoint(torch.from_numpy(x), torch.from_numpy(mag), torch.from_numpy(w), **kw)
    assert rel_l2(g_x.numpy(), xt.grad.numpy()) <= 1e-10 and rel_l2(g_m.numpy(), mt.grad.numpy()) <= 1e-10


def test_adjoint_recursion_convention_where_the_spectrum_vanishes():
    """A silent frame (R exactly 0) and bins with m = 0: the second term is 0, gm of the silent frame is exactly 0 - what torch's
    abs gives autograd at 0 too."""
    x, mag, w, kw, _ = _case(64, 16, 11, True, True, False)
    x[:, 64:128] = 0                                                 # frame 6 covers samples [64, 128)
    mag[:, 3:6] = 0
    xt, mt = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(mag).requires_grad_(True)
    (pt.project(xt, mt, **kw) * torch.from_numpy(w)).sum().backward()
    g_x, g_m = pt.project_adjoint(torch.from_numpy(x), torch.from_numpy(mag), torch.from_numpy(w), **kw)
    assert pt.stft(torch.from_numpy(x), 33, **kw)[:, :, 6].abs().max() == 0
    assert torch.isfinite(g_x).all() and torch.isfinite(g_m).all() and not g_m[:, :, 6].any()
    assert rel_l2(g_x.numpy(), xt.grad.numpy()) <= 1e-10 and rel_l2(g_m.numpy(), mt.grad.numpy()) <= 1e-10


@pytest.mark.parametrize("name", [n for n, _ in pt.SEEDS])
def test_float32_cases_are_well_conditioned(name):
    """The rule tests/_proj_torch.py picks the seeds of the fused float32 cases by: the restatement's own float32 gradient error."""
    f32, f64 = pt.reference(name, np.float32), pt.reference(name, np.float32, np.float64)
    own = max(rel_l2(f32[1], f64[1]), rel_l2(f32[2], f64[2]))
    print(f"{name}: the restatement's own float32 gradient error {own:.3e}")
    assert own <= (2e-5 if name == "2048/512 normalized" else 1e-5)


def test_argument_errors_need_no_gpu():
    w = torch.from_numpy(hann(64, np.float32))
    kw = dict(hop_length=16, window=w)
    x, mag = torch.zeros(2, 160), torch.ones(2, 33, 11)
    with pytest.raises(ValueError, match="11 frames need L = 160"):
        si.gla_projection(torch.zeros(2, 161), mag, **kw)
    with pytest.raises(ValueError, match="11 bins mean n_fft = 20"):
        si.gla_projection(x, mag.transpose(1, 2), **kw)                            # (frame-major data without frame_major=True)
    with pytest.raises(ValueError, match="need L = 160"):
        si.gla_projection(torch.zeros(2, 161), mag.transpose(1, 2), frame_major=True, **kw)
    with pytest.raises(TypeError, match="mag must be real"):
        si.gla_projection(x, torch.ones(2, 33, 11, dtype=torch.complex64), **kw)
    with pytest.raises(TypeError, match="float16 / bfloat16 / float32 / float64"):
        si.gla_projection(x.to(torch.int32), mag, **kw)
    with pytest.raises(ValueError, match="x holds 2 items and mag 3"):
        si.gla_projection(x, torch.ones(3, 33, 11), **kw)
    with pytest.raises(ValueError, match="17 bins mean n_fft = 32, which does not hold a window of 64 samples"):
        si.gla_projection(x, torch.ones(2, 17, 11), **kw)
    with pytest.raises(ValueError, match="must have 1 or 2 dimensions"):
        si.gla_projection(torch.zeros(1, 2, 160), mag, **kw)
    with pytest.raises(ValueError, match="holds 65536 items, gla_projection takes at most 65535"):
        si.gla_projection(torch.zeros(65536, 16), torch.ones(65536, 9, 2), hop_length=16)
    with pytest.raises(TypeError, match="spec must be complex"):
        si.istft(mag, **kw)
    with pytest.raises(ValueError, match="holds 65536 items, istft takes at most 65535"):
        si.istft(torch.ones(65536, 9, 2, dtype=torch.complex64), hop_length=16)
    with pytest.raises(ValueError, match="stft needs n_fft, win_length or a window"):
        si.stft(x, hop_length=16)
    with pytest.raises(ValueError, match="fewer than one frame"):
        si.stft(torch.zeros(2, 10), center=False, **kw)
    with pytest.raises(ValueError, match="holds 65536 items, stft takes at most 65535"):
        si.stft(torch.zeros(65536, 16), n_fft=16)


def test_an_empty_batch_needs_no_gpu():
    kw = dict(hop_length=16, window=torch.from_numpy(hann(64, np.float32)))
    x, mag = torch.zeros(0, 160, requires_grad=True), torch.ones(0, 33, 11, requires_grad=True)
    y = si.gla_projection(x, mag, **kw)
    assert y.shape == (0, 160) and y.requires_grad
    y.sum().backward()
    assert x.grad.shape == x.shape and mag.grad.shape == mag.shape
    assert si.stft(x, **kw).shape == (0, 33, 11) and si.stft(x, **kw).is_complex()
    assert si.istft(torch.ones(0, 33, 11, dtype=torch.complex64), **kw).shape == (0, 160)
