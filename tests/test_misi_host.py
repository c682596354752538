"""MISI, the parts that need no GPU: properties of its NumPy restatement (tests/_misi_oracle.py), the C ABI of specinv_misi_init /
_iterate / _run (declared, bound, exported, argument errors) and the argument checks of `spectrogram_inversion_amd.misi`.
(SPECINV_ESTATE and the errors that depend on a plan's shape need a plan, and a plan needs the device: tests/test_gpu_misi.py.)"""
import ctypes as C
import re

import numpy as np
import pytest

import _misi_oracle as mo
import oracle
from _util import ROOT, hann
from oracle.stftlib import args_helper, istft, signal_length, stft
from spectrogram_inversion_amd import _lib, build

NAMES = ("specinv_misi_init", "specinv_misi_iterate", "specinv_misi_run")


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def _err(lib):
    return lib.specinv_last_error().decode()


def _case(seed, n_fft, hop, T, B, K, extra=None, dtype=np.float64):
    rng = np.random.default_rng(seed)
    kw = dict(hop_length=hop, window=hann(n_fft, dtype), **(extra or {}))
    mag = (rng.random((B, K, n_fft // 2 + 1, T)) + 0.05).astype(dtype)
    start = (mag * np.exp(1j * rng.uniform(-np.pi, np.pi, mag.shape))).astype(np.complex64 if dtype == np.float32 else np.complex128)
    L = signal_length(T, args_helper(n_fft // 2 + 1, dtype, **kw))
    mix = (0.1 * rng.standard_normal((B, L + 5))).astype(dtype)
    return start, mix, L, kw


@pytest.mark.parametrize("n_fft,hop,T,B,K", [(512, 128, 12, 2, 3), (256, 77, 9, 1, 5), (128, 32, 10, 2, 2)])
def test_oracle_sources_add_up_to_the_mixture(n_fft, hop, T, B, K):
    start, mix, L, kw = _case(1, n_fft, hop, T, B, K)
    x = mo.misi(start, mix, 4, **kw)
    assert x.shape == (B, K, L) and np.isfinite(x).all()
    assert np.abs(x.sum(1) - mix[:, :L]).max() <= 1e-12
    x1 = mo.misi(start[0], mix[0], 4, **kw)                      # (K, F, T) with a (L_m,) mixture: the first mixture's rows
    assert x1.shape == (K, L) and np.array_equal(x1, mo.misi(start[:1], mix[:1], 4, **kw)[0])


def test_oracle_single_source_is_the_mixture():
    start, mix, L, kw = _case(2, 256, 64, 11, 2, 1)
    x = mo.misi(start, mix, 3, **kw)
    assert np.abs(x[:, 0] - mix[:, :L]).max() <= 1e-15


def test_oracle_without_coupling_is_griffin_lim_without_momentum():
    start, mix, L, kw = _case(3, 256, 64, 10, 2, 3)
    B, K = start.shape[:2]
    gl = oracle.griffin_lim(start.reshape((B * K,) + start.shape[2:]), max_iter=4, alpha=0.0, tol=0, **kw)
    x = mo.misi(start, mix, 4, mix_on=False, **kw)
    assert np.abs(x.reshape(B * K, L) - gl).max() <= 1e-13 * np.abs(gl).max()


def test_oracle_zero_correction_leaves_the_griffin_lim_step():
    """A mixture that already is the sum of the sources' current signals corrects nothing: one MISI iteration is then one
    Griffin-Lim iteration (alpha = 0) of every source - with the mixture of each step set to the sum of the independent
    trajectories, MISI is those trajectories."""
    start, _, L, kw = _case(4, 256, 64, 10, 2, 3)
    B, K, F, T = start.shape
    a = args_helper(F, start.dtype, **kw)
    flat = start.reshape(B * K, F, T)
    m = np.abs(flat)
    x0, env = istft(flat, a)
    assert np.abs(mo.mix_step(x0.reshape(B, K, L), x0.reshape(B, K, L).sum(1)) - x0.reshape(B, K, L)).max() <= 1e-15
    S = stft(x0, a)
    y, _ = istft(S * m / (np.abs(S) + 1e-16), a, envelope=env)          # one Griffin-Lim step of every source on its own
    # the oracle, fed the sum of the initial signals (first mix step: zero correction) ...
    first = x0.reshape(B, K, L).sum(1)
    x = mo.misi(start, first, 1, **kw)
    # ... differs from that step exactly by the correction towards `first`: taking it out again gives the step back
    e = (first - y.reshape(B, K, L).sum(1)) / K
    assert np.abs((x - e[:, None]) - y.reshape(B, K, L)).max() <= 1e-13
    # and with the step's own sum as the mixture nothing is left to correct
    assert np.abs(mo.mix_step(y.reshape(B, K, L), y.reshape(B, K, L).sum(1)) - y.reshape(B, K, L)).max() <= 1e-15


def test_mixture_phase_start_takes_zero_angle_at_exact_zeros():
    mag = np.full((1, 2, 65, 6), 0.5)
    c = mo.mixture_phase_start(mag, np.zeros((1, 5 * 32)), hop_length=32, window=hann(128, np.float64))
    assert np.array_equal(c, mag.astype(np.complex128))


def test_misi_symbols_are_declared_bound_and_exported(lib):
    header = open(ROOT + "/include/specinv.h").read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
    assert lib.specinv_abi_version() == 1


def test_misi_argument_errors_do_not_need_a_gpu(lib):
    buf = C.c_void_p(16)                      # never dereferenced: every call below fails its checks first
    assert lib.specinv_misi_init(None, None, buf, buf, 100, 2) == _lib.EINVAL and "init_spec" in _err(lib)
    assert lib.specinv_misi_init(None, buf, buf, None, 100, 2) == _lib.EINVAL and "mixture" in _err(lib)
    for bad in (0, -3):
        assert lib.specinv_misi_init(None, buf, buf, buf, 100, bad) == _lib.EINVAL and "n_src" in _err(lib)
    assert lib.specinv_misi_init(None, buf, buf, buf, 100, 2) == _lib.EINVAL and "plan" in _err(lib)
    assert lib.specinv_misi_iterate(None, 1, 0, None) == _lib.EINVAL and "plan" in _err(lib)
    assert lib.specinv_misi_run(None, 10, 5, 0.0, 0, None, None, None, _lib.EVAL_CB(), None) == _lib.EINVAL and "plan" in _err(lib)


def test_python_argument_errors_need_no_gpu():
    import torch
    from spectrogram_inversion_amd import misi
    mag, mix = torch.rand(3, 65, 9), torch.randn(8 * 32)
    with pytest.raises(TypeError):
        misi(mag.numpy(), mix)
    with pytest.raises(TypeError, match="real"):
        misi(mag, mix.to(torch.complex64), hop_length=32)
    with pytest.raises(TypeError, match="float64"):
        misi(mag, mix.double(), hop_length=32)
    with pytest.raises(TypeError):
        misi(mag.to(torch.int32), mix, hop_length=32)
    with pytest.raises(ValueError, match=r"\(65, 9\)"):
        misi(mag[0], mix, hop_length=32)
    with pytest.raises(ValueError, match=r"\(2, 256\)"):
        misi(mag, mix.reshape(2, -1)[:, :256].repeat(1, 2), hop_length=32)                 # a (B, L) mixture for (K, F, T) specs
    with pytest.raises(ValueError, match=r"\(3, 256\).*\(2, 3, 65, 9\)"):
        misi(torch.rand(2, 3, 65, 9), torch.randn(3, 256), hop_length=32)                  # three mixtures for two groups
    with pytest.raises(ValueError, match="shorter"):
        misi(mag, mix[:255], hop_length=32)
    with pytest.raises(ValueError, match="sources"):
        misi(torch.rand(65536, 3, 1), torch.randn(8), hop_length=1)
    with pytest.raises(NotImplementedError, match="detach"):
        misi(mag.clone().requires_grad_(True), mix, hop_length=32)
    with pytest.raises(NotImplementedError, match="detach"):
        misi(mag, mix.clone().requires_grad_(True), hop_length=32)
