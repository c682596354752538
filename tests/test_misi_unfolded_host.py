"""misi_unfolded, the parts that need no GPU: the torch restatement the GPU tests differentiate (tests/_misi_torch.py) against the
NumPy oracle it restates (tests/_misi_oracle.py), the argument checks of `spectrogram_inversion_amd.misi_unfolded`, and the C ABI
of specinv_misi_mix_adjoint / specinv_misi_step_adjoint (declared, bound, exported, argument errors).
(The errors that depend on a plan's shape need a plan, and a plan needs the device: tests/test_gpu_misi_unfolded.py.)"""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import _misi_oracle as mo
import _misi_torch as mt
from _util import ROOT, hann, rel_l2
from oracle.stftlib import args_helper, signal_length
from spectrogram_inversion_amd import _lib, build

NAMES = ("specinv_misi_mix_adjoint", "specinv_misi_step_adjoint")

# n_fft, hop, extra stft kwargs
CONFIGS = [(128, 32, {}), (64, 16, dict(onesided=False, pad_mode="constant"))]


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def _err(lib):
    return lib.specinv_last_error().decode()


@pytest.mark.parametrize("magnitude_start", [False, True], ids=["complex", "magnitude"])
@pytest.mark.parametrize("n_fft,hop,extra", CONFIGS)
def test_restatement_equals_the_oracle(n_fft, hop, extra, magnitude_start):
    """float64, 3 iterations: tests/test_gpu_misi.py's float64 gate."""
    rng = np.random.default_rng(n_fft + hop)
    B, K, T = 2, 3, 10
    F = n_fft // 2 + 1 if extra.get("onesided", True) else n_fft
    kw = dict(hop_length=hop, window=hann(n_fft, np.float64), **extra)
    mag = rng.random((B, K, F, T)) + 0.05
    L = signal_length(T, args_helper(F, np.float64, **kw))
    mix = 0.1 * rng.standard_normal((B, L + 3))
    if magnitude_start:
        specs, start = mag, mo.mixture_phase_start(mag, mix, **kw)
    else:
        specs = start = mag * np.exp(1j * rng.uniform(-np.pi, np.pi, mag.shape))
    ref = mo.misi(start, mix, 3, **kw)
    x = mt.misi(torch.from_numpy(specs), torch.from_numpy(mix), 3, **kw).numpy()
    assert x.shape == ref.shape == (B, K, L)
    e = rel_l2(x, ref)
    print(f"rel_l2 restatement vs oracle {e:.3e}")
    assert e <= 1e-10, e


def test_restatement_is_differentiable():
    kw = dict(hop_length=32, window=hann(128, np.float64))
    mag = (torch.rand(1, 2, 65, 6, dtype=torch.float64) + 0.05).requires_grad_(True)
    mix = (0.1 * torch.randn(1, 5 * 32 + 3, dtype=torch.float64)).requires_grad_(True)
    mt.misi(mag, mix, 2, **kw).square().sum().backward()
    assert torch.isfinite(mag.grad).all() and mag.grad.abs().max() > 0
    assert torch.isfinite(mix.grad).all() and mix.grad[:, :160].abs().max() > 0 and not mix.grad[:, 160:].any()


def test_python_argument_errors_need_no_gpu():
    from spectrogram_inversion_amd import misi_unfolded
    mag, mix = torch.rand(3, 65, 9, requires_grad=True), torch.randn(8 * 32)
    with pytest.raises(TypeError):
        misi_unfolded(mag.detach().numpy(), mix)
    with pytest.raises(TypeError, match="real"):
        misi_unfolded(mag, mix.to(torch.complex64), hop_length=32)
    with pytest.raises(TypeError, match="float64"):
        misi_unfolded(mag, mix.double(), hop_length=32)                                     # the dtype mismatch
    with pytest.raises(TypeError):
        misi_unfolded(mag.detach().to(torch.int32), mix, hop_length=32)
    with pytest.raises(ValueError, match=r"\(65, 9\)"):
        misi_unfolded(mag[0], mix, hop_length=32)
    with pytest.raises(ValueError, match=r"\(2, 256\)"):
        misi_unfolded(mag, mix.reshape(2, -1)[:, :256].repeat(1, 2), hop_length=32)         # a (B, L) mixture for (K, F, T) specs
    with pytest.raises(ValueError, match=r"\(3, 256\).*\(2, 3, 65, 9\)"):
        misi_unfolded(torch.rand(2, 3, 65, 9), torch.randn(3, 256), hop_length=32)          # three mixtures for two groups
    with pytest.raises(ValueError, match="shorter"):
        misi_unfolded(mag, mix[:255], hop_length=32)
    for bad in (0, -2, 2.5, None, True):
        with pytest.raises(ValueError, match="n_iter"):
            misi_unfolded(mag, mix, n_iter=bad, hop_length=32)
    # the batch limit, with and without a gradient to compute: 21846 mixtures of 3 sources are 65538 items
    for grad in (False, True):
        with pytest.raises(ValueError, match="65538 items"):
            misi_unfolded(torch.rand(21846, 3, 3, 2, requires_grad=grad), torch.randn(21846, 4), hop_length=1)
    with pytest.raises(ValueError, match="sources"):
        misi_unfolded(torch.rand(65536, 3, 1), torch.randn(8), hop_length=1)
    with pytest.raises(TypeError, match="positional"):
        misi_unfolded(mag, mix, 3, 1e-6, hop_length=32)                                     # no tol, eva_iter, metric, verbose


def test_symbols_are_declared_bound_and_exported(lib):
    header = open(ROOT + "/include/specinv.h").read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", header)
        assert decl, name
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(decl.group(1).split(",")), name     # header and binding agree
        for ctype, param in zip(args, decl.group(1).split(",")):
            assert (ctype is C.c_int) == (re.match(r"\s*int\s+\w+\s*$", param) is not None), (name, param)
    assert lib.specinv_abi_version() == 1


def test_argument_errors_do_not_need_a_gpu(lib):
    buf = C.c_void_p(16)                      # never dereferenced: every call below fails its checks first
    assert lib.specinv_misi_mix_adjoint(None, 2, None, buf) == _lib.EINVAL and "g_inout" in _err(lib)
    assert lib.specinv_misi_mix_adjoint(None, 2, buf, None) == _lib.EINVAL and "gmix_accum" in _err(lib)
    for bad in (0, -3):
        assert lib.specinv_misi_mix_adjoint(None, bad, buf, buf) == _lib.EINVAL and "n_src" in _err(lib)
    assert lib.specinv_misi_mix_adjoint(None, 2, buf, buf) == _lib.EINVAL and "plan" in _err(lib)
    names = ("x_prev", "mag_fm", "g_inout", "gmix_accum", "gmag_fm_accum")
    for i, name in enumerate(names):
        ptrs = [None if j == i else buf for j in range(5)]
        assert lib.specinv_misi_step_adjoint(None, 2, *ptrs) == _lib.EINVAL and name in _err(lib), name
    for bad in (0, -3):
        assert lib.specinv_misi_step_adjoint(None, bad, buf, buf, buf, buf, buf) == _lib.EINVAL and "n_src" in _err(lib)
    assert lib.specinv_misi_step_adjoint(None, 2, buf, buf, buf, buf, buf) == _lib.EINVAL and "plan" in _err(lib)
