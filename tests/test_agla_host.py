"""Accelerated Griffin-Lim, the parts that need no GPU: properties of its NumPy restatement (tests/_agla_oracle.py), the C ABI of
specinv_agla_init / _iterate / _run (declared, bound, exported, argument errors) and the argument checks of
`spectrogram_inversion_amd.accelerated_griffin_lim`.  (SPECINV_ESTATE needs a plan, and a plan needs the device:
tests/test_gpu_agla.py.)"""
import ctypes as C
import re

import numpy as np
import pytest

import _agla_oracle as ao
import oracle
from _util import ROOT, hann, rel_l2
from spectrogram_inversion_amd import _lib, build

NAMES = ("specinv_agla_init", "specinv_agla_iterate", "specinv_agla_run")


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def _err(lib):
    return lib.specinv_last_error().decode()


def _case(seed, n_fft, hop, T, B, dtype=np.float64, extra=None):
    rng = np.random.default_rng(seed)
    kw = dict(hop_length=hop, window=hann(n_fft, dtype), **(extra or {}))
    mag = (rng.random((B, n_fft // 2 + 1, T)) + 0.05).astype(dtype)
    start = (mag * np.exp(1j * rng.uniform(-np.pi, np.pi, mag.shape))).astype(np.complex64 if dtype == np.float32 else np.complex128)
    return start, kw


@pytest.mark.parametrize("n_fft,hop,T,B,dtype", [(256, 64, 10, 2, np.float64), (256, 77, 9, 1, np.float32), (128, 32, 12, 3, np.float32)])
def test_oracle_without_extrapolation_is_griffin_lim_without_momentum(n_fft, hop, T, B, dtype):
    """alpha = 0, gamma = 1: t = y, c = t + 0 (t - t_prev) - the bits of the reference's recursion with lr = 0"""
    start, kw = _case(1, n_fft, hop, T, B, dtype)
    gl = oracle.griffin_lim(start, max_iter=5, alpha=0.0, tol=0, **kw)
    x = ao.agla(start, 5, alpha=0.0, gamma=1.0, **kw)
    assert x.dtype == dtype and x.shape == gl.shape and np.isfinite(x).all()
    assert np.array_equal(x, gl)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_oracle_with_gamma_one_ignores_beta(dtype):
    start, kw = _case(2, 256, 64, 11, 2, dtype)
    out = [ao.agla(start, 6, alpha=0.7, beta=b, gamma=1.0, **kw) for b in (None, 0.0, 3.0)]
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2])
    assert not np.array_equal(out[0], ao.agla(start, 6, alpha=0.7, beta=3.0, gamma=0.7, **kw))      # ... and reads it otherwise
    assert not np.array_equal(ao.agla(start, 6, alpha=0.7, beta=0.0, gamma=0.7, **kw),
                              ao.agla(start, 6, alpha=0.7, beta=3.0, gamma=0.7, **kw))


def test_oracle_first_iteration_has_no_history_and_momentum_moves_the_rest():
    start, kw = _case(3, 256, 64, 10, 2)
    plain = [ao.agla(start, n, alpha=0.0, **kw) for n in (1, 2, 3)]
    fast = [ao.agla(start, n, alpha=0.99, **kw) for n in (1, 2, 3)]
    assert np.array_equal(plain[0], fast[0])                    # n = 1: t_1 = P(c_0), whatever the parameters
    assert np.array_equal(plain[1], fast[1])                    # n = 2: c_1 = t_1, so t_2 = P(t_1) either way
    assert not np.array_equal(plain[2], fast[2])                # n = 3: c_2 = t_2 + alpha (t_2 - t_1) entered the projection
    assert np.array_equal(ao.agla(start, 1, alpha=0.5, beta=1.2, gamma=0.7, **kw), plain[0])


def test_oracle_shapes_real_input_and_evaluation_hooks():
    start, kw = _case(4, 128, 32, 12, 2)
    mag = np.abs(start)
    x = ao.agla(mag, 4, **kw)                                                    # real: from oracle.phase_init
    # (not the same bits: a complex start's target is its own modulus, mag (cos^2 + sin^2)^(1/2), a rounding away from mag)
    assert rel_l2(x, ao.agla(oracle.phase_init(mag, **kw), 4, **kw)) <= 1e-10
    x1 = ao.agla(mag[0], 4, **kw)
    assert x1.shape == (x.shape[1],) and np.array_equal(x1, ao.agla(mag[:1], 4, **kw)[0])
    trace, sums = [], []
    ao.agla(start, 7, eva_iter=2, trace=trace, sums=sums, **kw)
    assert [t[0] for t in trace] == [1, 3, 5] and len(sums) == 7
    assert all(abs(trace[i][2] - sums[2 * i + 1][0] / sums[2 * i + 1][3]) <= 1e-12 * trace[i][2] for i in range(3))


def test_agla_symbols_are_declared_bound_and_exported(lib):
    header = open(ROOT + "/include/specinv.h").read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
    assert lib.specinv_abi_version() == 1


def test_agla_argument_errors_do_not_need_a_gpu(lib):
    buf = C.c_void_p(16)                      # never dereferenced: every call below fails its checks first
    for a, b, g, word in ((-0.1, 0.5, 1.0, "alpha"), (0.5, -1.0, 1.0, "beta"), (0.5, 0.5, 0.0, "gamma"), (0.5, 0.5, -2.0, "gamma"),
                          (float("nan"), 0.5, 1.0, "alpha"), (0.5, 0.5, float("nan"), "gamma")):
        assert lib.specinv_agla_init(None, buf, buf, a, b, g) == _lib.EINVAL and word in _err(lib), (a, b, g)
    assert lib.specinv_agla_init(None, buf, buf, 0.99, 0.99, 1.0) == _lib.EINVAL and "plan" in _err(lib)
    assert lib.specinv_agla_iterate(None, 1, 0, None) == _lib.EINVAL and "plan" in _err(lib)
    assert lib.specinv_agla_run(None, 10, 5, 0.0, 0, None, None, None, _lib.EVAL_CB(), None) == _lib.EINVAL and "plan" in _err(lib)


def test_python_argument_errors_need_no_gpu():
    import torch
    from spectrogram_inversion_amd import accelerated_griffin_lim as agl
    mag = torch.rand(3, 65, 9)
    with pytest.raises(TypeError):
        agl(mag.numpy(), hop_length=32)
    with pytest.raises(TypeError, match="int32"):
        agl(mag.to(torch.int32), hop_length=32)
    with pytest.raises(ValueError, match=r"\(9,\)"):
        agl(mag[0, 0], hop_length=32)
    with pytest.raises(ValueError, match=r"\(1, 3, 65, 9\)"):
        agl(mag[None], hop_length=32)
    with pytest.raises(ValueError, match="no items"):
        agl(mag[:0], hop_length=32)
    with pytest.raises(ValueError, match="alpha"):
        agl(mag, alpha=-0.5, hop_length=32)
    with pytest.raises(ValueError, match="beta"):
        agl(mag, beta=-1e-3, hop_length=32)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="gamma"):
            agl(mag, gamma=bad, hop_length=32)
    with pytest.raises(AssertionError):
        agl(mag, max_iter=0, hop_length=32)
    with pytest.raises(AssertionError):
        agl(mag, metric="nope", hop_length=32)
    with pytest.raises(RuntimeError, match="complex window"):
        agl(mag, hop_length=16, window=torch.ones(65, dtype=torch.complex64))    # (two-sided then: n_fft = 65)
    with pytest.raises(NotImplementedError, match="accelerated_griffin_lim is not differentiable; detach the input"):
        agl(mag.clone().requires_grad_(True), hop_length=32)
    with torch.no_grad():                     # outside grad mode a leaf that requires grad is data like any other: no refusal
        try:
            agl(mag.clone().requires_grad_(True), max_iter=1, verbose=False, hop_length=32)
        except NotImplementedError:
            pytest.fail("requires_grad must only be refused under grad mode")
        except Exception:
            pass                              # (no device here: whatever require_gpu raises)
