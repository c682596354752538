"""mel_to_stft_unfolded, the parts that need no GPU: the torch restatement the GPU tests differentiate (tests/_mel_torch.py) against
the NumPy oracle it restates (tests/_mel_oracle.py); the reverse sweep the device runs, written out in NumPy, against
autograd of the restatement; the float32 noise of the GPU tests' cases; the argument checks of `mel_to_stft_unfolded`; and the C ABI
of specinv_mel_nnls_adjoint / specinv_mel_nnls_adjoint_max_iter (declared, bound, exported, argument errors)."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import _mel_oracle as mo
import _mel_torch as mt
from _util import ROOT, rel_l2
from spectrogram_inversion_amd import _lib, build
from spectrogram_inversion_amd.mel import mel_filterbank

NAMES = ("specinv_mel_nnls_adjoint", "specinv_mel_nnls_adjoint_max_iter")


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def _err(lib):
    return lib.specinv_last_error().decode()


@pytest.mark.parametrize("case", mt.CASES, ids=str)
def test_restatement_equals_the_oracle(case):
    """float64: the two differ in the order of the matrix products' sums alone."""
    name, power, n_iter = case
    M, mel, _ = mt.inputs(name, power, np.float64)
    out = mt.reference(case, np.float64)[0]
    ref = mo.mel_to_stft(M, mel, n_iter, power)
    assert out.shape == ref.shape
    if n_iter == 0:
        assert not out.any() and not ref.any()
        return
    e = rel_l2(out, ref)
    print(f"{case}: restatement vs oracle {e:.3e}")
    assert e <= 1e-12, e


@pytest.mark.parametrize("case", mt.CASES, ids=str)
def test_sweep_equals_autograd(case):
    """float64, every case, power 1 included (relu's convention at 0 on both sides): 1e-12.  The silent frame's column and the row of
    a band that touches no bin are exact zeros on both sides."""
    name, power, n_iter = case
    M, mel, w = mt.inputs(name, power, np.float64)
    ref = mt.reference(case, np.float64)[1]
    got = mt.sweep(M, mel, w, n_iter, power)
    assert got.shape == ref.shape == mel.shape
    T = mel.shape[2]
    for g in (got, ref):
        assert not g[:, :, mt.SILENT(T)].any()
        assert name != "zero_row_col40x257" or not g[:, 5].any()
    if n_iter == 0:
        assert not got.any() and not ref.any()
        return
    assert ref.any()
    e = rel_l2(got, ref)
    print(f"{case}: sweep vs autograd {e:.3e}")
    assert e <= 1e-12, e


@pytest.mark.parametrize("case", [c for c in mt.CASES if c[2] > 0], ids=str)
def test_float32_noise_of_the_gpu_cases(case):
    """The restatement's own float32-against-float64 gradient error (float32-rounded inputs on both sides) on every case
    tests/test_gpu_mel_unfolded.py runs in float32 stays at or below 1e-3, the cap of tests/test_agla_unfolded_host.py: the device's
    float32 gate, the larger of 1e-4 and 6 times this figure, is then never wider than 6e-3."""
    g32 = mt.reference(case, np.float32)[1]
    g64 = mt.reference(case, np.float32, np.float64)[1]
    e = rel_l2(g32, g64)
    print(f"{case}: grad float32 vs float64 {e:.3e}")
    assert e <= 1e-3, e


@pytest.mark.parametrize("case", [c for c in mt.CASES if c[1] == 2.0 and c[2] > 0], ids=str)
def test_float32_noise_under_other_orders_of_the_sums(case):
    """Power 2, where the root's derivative grows near zero: the float32 restatement with its sums in four other orders stays within
    half the device's float32 gate (the larger of 1e-4 and 6 x the restatement's own error), so the gate does not hang on the order
    in which an implementation happens to add (the seeds of _mel_torch.SEEDS were chosen for that)."""
    g64 = mt.reference(case, np.float32, np.float64)[1]
    gate = max(1e-4, 6 * rel_l2(mt.reference(case, np.float32)[1], g64))
    rng = np.random.default_rng(100 + case[2])
    for _ in range(4):
        e = rel_l2(mt.reordered(case, rng), g64)
        print(f"{case}: reordered float32 vs float64 {e:.3e} (gate {gate:.1e})")
        assert e <= gate / 2, (e, gate)


def test_python_argument_errors_need_no_gpu():
    from spectrogram_inversion_amd import mel_to_audio_unfolded, mel_to_stft, mel_to_stft_unfolded
    fb = mel_filterbank(22050, 512, 20)
    for grad in (False, True):
        mel = torch.zeros(20, 5, requires_grad=grad)
        with pytest.raises(TypeError, match="torch.Tensor"):
            mel_to_stft_unfolded(mel.detach().numpy(), fb)
        with pytest.raises(TypeError, match="complex"):
            mel_to_stft_unfolded(torch.zeros(20, 5, dtype=torch.complex64), fb)
        with pytest.raises(ValueError, match="n_iter"):
            mel_to_stft_unfolded(mel, fb, n_iter=-1)
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="power"):
                mel_to_stft_unfolded(mel, fb, power=bad)
        with pytest.raises(ValueError, match="shape"):
            mel_to_stft_unfolded(torch.zeros(5, requires_grad=grad), fb)
        with pytest.raises(ValueError, match="19 bands, mel_fb 20"):
            mel_to_stft_unfolded(torch.zeros(19, 5, requires_grad=grad), fb)
        with pytest.raises(NotImplementedError, match="dtype"):
            mel_to_stft_unfolded(torch.zeros(20, 5, dtype=torch.int32), fb)
        with pytest.raises(ValueError, match="65536 items"):
            mel_to_stft_unfolded(torch.zeros(65536, 20, 1, requires_grad=grad), fb)
        with pytest.raises(ValueError, match="n_iter"):
            mel_to_audio_unfolded(mel, fb, nnls_iter=-1)
    # mel_to_stft itself stays as it is
    with pytest.raises(NotImplementedError, match="detach"):
        mel_to_stft(torch.zeros(20, 5, requires_grad=True), fb)


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
    assert lib.specinv_mel_nnls_adjoint(None, buf, -1, 1.0, buf, buf) == _lib.EINVAL and "n_iter" in _err(lib)
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        assert lib.specinv_mel_nnls_adjoint(None, buf, 10, bad, buf, buf) == _lib.EINVAL and "power" in _err(lib)
    for i in range(3):
        ptrs = [None if j == i else buf for j in range(3)]
        assert lib.specinv_mel_nnls_adjoint(None, ptrs[0], 10, 1.0, ptrs[1], ptrs[2]) == _lib.EINVAL and "NULL" in _err(lib)
    assert lib.specinv_mel_nnls_adjoint(None, buf, 10, 1.0, buf, buf) == _lib.EINVAL and "plan" in _err(lib)
    most = C.c_int(-7)
    assert lib.specinv_mel_nnls_adjoint_max_iter(None, None) == _lib.EINVAL and "NULL" in _err(lib)
    assert lib.specinv_mel_nnls_adjoint_max_iter(None, C.byref(most)) == _lib.EINVAL and "plan" in _err(lib)
    assert most.value == -7
