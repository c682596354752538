"""The torch restatement of `griffin_lim` / `ADMM` (tests/_gla_torch.py) without a GPU: it reproduces the reference's autograd on every
case of g10_autograd / g11_autograd_admm, and every end-to-end case of tests/test_gpu_autograd.py is admitted by a CPU-only measure of
its conditioning before a device sees it."""
import glob
import os

import numpy as np
import pytest
import torch

import _gla_torch as gt
from _util import GOLDEN, hann, load_golden, rel_l2

# tag, n_fft, hop, Hann window, extra - the cases of make_golden.py::g10_autograd / g11_autograd_admm (alpha 0.5; rho per case)
G10 = [("f32_hann", 128, 32, True, {}), ("f64_hann", 128, 32, True, {}), ("f64_rect_default", 128, None, False, {}),
       ("f64_const_pad", 64, 16, True, dict(pad_mode="constant")), ("f64_normalized", 64, 16, True, dict(normalized=True))]
G11 = [("f32_hann", 128, 32, True, 0.1, {}), ("f64_hann", 128, 32, True, 0.1, {}), ("f64_rect_default", 64, None, False, 0.5, {}),
       ("f64_twosided", 64, 16, True, 0.2, dict(onesided=False, pad_mode="constant"))]


def _kw(n_fft, hop, use_hann, extra, dtype):
    kw = dict(extra)
    if hop:
        kw["hop_length"] = hop
    if use_hann:
        kw["window"] = hann(n_fft, dtype)
    return kw


def _check(what, method, spec, w, n_iter, coef, kw, y_ref, g_ref):
    y, g = gt.grads(method, spec, w, n_iter, coef, kw)
    ey, eg = (rel_l2(y, y_ref) if y_ref is not None else 0.0), rel_l2(g, g_ref)
    if w.dtype == np.float32:
        noise = gt.noise32_of(method, spec, w, n_iter, coef, kw)
        tol = max(2e-4, 6 * noise)
        print(f"{what}: y {ey:.2e} grad {eg:.2e} (noise32 {noise:.2e}, gate {tol:.2e})")
    else:
        tol = 1e-11
        print(f"{what}: y {ey:.2e} grad {eg:.2e}")
    assert ey <= tol and eg <= tol, (what, ey, eg, tol)


@pytest.mark.parametrize("tag,n_fft,hop,use_hann,extra", G10)
def test_gla_restatement_is_the_reference(tag, n_fft, hop, use_hann, extra):
    g = load_golden("g10_autograd")
    mag = g[f"mag_{tag}"]
    _check(f"g10 {tag}", "gla", mag, g[f"w_{tag}"], 3, 0.5, _kw(n_fft, hop, use_hann, extra, mag.dtype.type), g[f"y_{tag}"],
           g[f"grad_{tag}"])


@pytest.mark.parametrize("method,fixture,n_iter,coef", [("gla", "g10_autograd", 2, 0.3), ("admm", "g11_autograd_admm", 2, 0.3)])
def test_restatement_is_the_reference_from_a_complex_start(method, fixture, n_iter, coef):
    g = load_golden(fixture)
    _check(f"{fixture} complex", method, g["c_complex"], g["w_complex"], n_iter, coef, dict(hop_length=32, window=hann(128, np.float64)),
           None, g["grad_complex"])


def test_gla_restatement_is_the_reference_on_its_test_pattern():
    """test/test_griffin.py:53-66: a 1-D signal, every default, mse against the signal (float32)"""
    g = load_golden("g10_autograd")
    x = torch.from_numpy(g["x_ref_test"])

    def grad(dt):
        sp = torch.stft(x, 256, return_complex=True).abs().to(dt).requires_grad_(True)
        y = gt.gla(sp[None], 2, 0.99)[0]
        torch.nn.functional.mse_loss(x[:y.shape[0]].to(dt), y).backward()
        return sp.grad.numpy()

    noise = rel_l2(grad(torch.float32), grad(torch.float64))
    err = rel_l2(grad(torch.float32), g["grad_ref_test"])
    print(f"g10 ref_test: grad {err:.2e} (noise32 {noise:.2e})")
    assert err <= max(2e-4, 6 * noise)


@pytest.mark.parametrize("tag,n_fft,hop,use_hann,rho,extra", G11)
def test_admm_restatement_is_the_reference(tag, n_fft, hop, use_hann, rho, extra):
    g = load_golden("g11_autograd_admm")
    mag = g[f"mag_{tag}"]
    _check(f"g11 {tag}", "admm", mag, g[f"w_{tag}"], 3, rho, _kw(n_fft, hop, use_hann, extra, mag.dtype.type), g[f"y_{tag}"],
           g[f"grad_{tag}"])


@pytest.mark.parametrize("name", gt.CASES_F64_MAG + gt.CASES_F64_COMPLEX)
def test_float64_case_is_admitted(name):
    """The one-ulp response of the restatement's float64 gradient is at most 1e-10: the device gate max(1e-9, 100 x sens64) stays
    at or below 1e-8."""
    s = gt.sens64(name)
    print(f"{name}: sens64 {s:.2e}")
    assert s <= 1e-10, (name, s)


@pytest.mark.parametrize("name", gt.CASES_F32_COMPLEX)
def test_float32_case_is_admitted(name):
    """The restatement's own float32 gradient is within 1e-3 of its float64 one."""
    n = gt.noise32(name)
    print(f"{name}: noise32 {n:.2e}")
    assert n <= 1e-3, (name, n)


def test_rtisi_fixtures_are_admitted():
    files = sorted(glob.glob(os.path.join(GOLDEN, "g17_autograd_rtisi_sizes_*.npz")))
    assert len(files) == 5
    for f in files:
        s = float(np.load(f)["sens64"])
        print(f"{os.path.basename(f)}: sens64 {s:.2e}")
        assert s <= 1e-8, (f, s)
        assert os.path.getsize(f) < 1 << 20


def test_wellcond_third_item_is_a_mix_of_the_first_two():
    x = gt.wellcond(3, 4000, 5)
    assert x.dtype == np.float32 and x.shape == (3, 4000) and np.array_equal(x[:2], gt.wellcond(2, 4000, 5))
    assert rel_l2(x[2], 0.6 * x[0].astype(np.float64) - 0.8 * x[1]) < 1e-6
