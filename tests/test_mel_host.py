"""Mel inversion, the parts that need no GPU: the C ABI of specinv_mel_nnls_setup / specinv_mel_nnls (exported, argument errors)
and the float64 restatement of its algorithm (tests/_mel_oracle.py) against scipy.optimize.nnls."""
import ctypes as C

import numpy as np
import pytest

import _mel_oracle as mo
from spectrogram_inversion_amd import _lib, build
from spectrogram_inversion_amd.mel import mel_filterbank


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def _err(lib):
    return lib.specinv_last_error().decode()


def test_mel_nnls_symbols_are_exported(lib):
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("specinv_mel_nnls_setup", "specinv_mel_nnls"):
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES


def test_mel_nnls_setup_argument_errors(lib):
    buf = C.c_void_p(16)                      # never dereferenced: every call below fails its checks first
    assert lib.specinv_mel_nnls_setup(None, buf, 0, 1.0) == _lib.EINVAL and "n_mels" in _err(lib)
    assert lib.specinv_mel_nnls_setup(None, buf, -3, 1.0) == _lib.EINVAL and "n_mels" in _err(lib)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.specinv_mel_nnls_setup(None, buf, 80, bad) == _lib.EINVAL and "lipschitz" in _err(lib)
    assert lib.specinv_mel_nnls_setup(None, None, 80, 1.0) == _lib.EINVAL and "NULL" in _err(lib)
    assert lib.specinv_mel_nnls_setup(None, buf, 80, 1.0) == _lib.EINVAL and "plan" in _err(lib)


def test_mel_nnls_argument_errors(lib):
    buf = C.c_void_p(16)
    assert lib.specinv_mel_nnls(None, buf, -1, 1.0, buf) == _lib.EINVAL and "n_iter" in _err(lib)
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        assert lib.specinv_mel_nnls(None, buf, 10, bad, buf) == _lib.EINVAL and "power" in _err(lib)
    assert lib.specinv_mel_nnls(None, None, 10, 1.0, buf) == _lib.EINVAL and "NULL" in _err(lib)
    assert lib.specinv_mel_nnls(None, buf, 10, 1.0, None) == _lib.EINVAL and "NULL" in _err(lib)
    assert lib.specinv_mel_nnls(None, buf, 10, 1.0, buf) == _lib.EINVAL and "plan" in _err(lib)


def test_python_argument_errors_need_no_gpu():
    import torch
    from spectrogram_inversion_amd import mel_to_audio, mel_to_stft
    fb = mel_filterbank(22050, 512, 20)
    with pytest.raises(TypeError):
        mel_to_stft(torch.zeros(20, 5, dtype=torch.complex64), fb)
    with pytest.raises(NotImplementedError, match="detach"):
        mel_to_stft(torch.zeros(20, 5, requires_grad=True), fb)
    with pytest.raises(ValueError):
        mel_to_stft(torch.zeros(20, 5), fb, power=0.0)
    with pytest.raises(ValueError):
        mel_to_stft(torch.zeros(20, 5), fb, n_iter=-1)
    with pytest.raises(ValueError):
        mel_to_stft(torch.zeros(5), fb)
    with pytest.raises(ValueError):
        mel_to_audio(torch.zeros(20, 5), fb, method="L_BFGS")


@pytest.fixture(scope="module")
def problem():
    M = mel_filterbank(22050, 2048, 80).astype(np.float64)
    S = mo.magnitude(mo.chirp_signal())
    return M, S


@pytest.mark.parametrize("power", [1.0, 2.0])
def test_oracle_against_scipy_nnls(problem, power):
    """DESIGN's table (this signal, 87 frames): at 300 iterations the KKT conditions hold, and the excess objective over the exact
    NNLS solution and the mel-domain SC stay within 1.6 x the figures measured at 50 / 100 / 300 iterations"""
    from scipy.optimize import nnls
    M, S = problem
    Y = M @ S ** power
    S_opt = np.stack([nnls(M, Y[:, j], maxiter=50 * M.shape[1])[0] for j in range(Y.shape[1])], 1)
    L = mo.lipschitz(M)
    bound = {1.0: {50: 4.5e-6, 100: 6e-8, 300: 4e-14}, 2.0: {50: 3e-5, 100: 6e-6, 300: 2.3e-6}}[power]
    sc_bound = {1.0: {100: 3e-4}, 2.0: {100: 3e-3}}[power]
    for n_iter in (50, 100, 300):
        Sp = mo.fista_nnls(M, Y, n_iter, L=L)
        assert Sp.min() >= 0
        ex = mo.excess_objective(M, Y, Sp, S_opt)
        assert -1e-12 <= ex <= bound[n_iter], (n_iter, ex)
        if n_iter in sc_bound:
            assert mo.mel_sc(M, Y, Sp) <= sc_bound[n_iter]
    S300 = mo.fista_nnls(M, Y, 300, L=L)
    assert mo.kkt_violation(M, Y, S300) < (1e-6 if power == 1.0 else 1e-4)
    assert mo.kkt_violation(M, Y, S_opt) < 1e-9


def test_oracle_edge_cases():
    M = mel_filterbank(16000, 256, 10).astype(np.float64)
    M[3] = 0.0                       # an all-zero row
    M[:, 40] = 0.0                   # ... and column
    Y = np.abs(np.random.default_rng(1).standard_normal((10, 6)))
    Y[:, 2] = 0.0                    # a silent frame
    Y[5, 4] = -0.3                   # an undershooting mel entry
    S = mo.fista_nnls(M, Y, 50, power=2.0)
    assert np.all(np.isfinite(S)) and S.min() >= 0
    assert np.all(S[:, 2] == 0.0) and np.all(S[40] == 0.0)
    assert np.all(mo.fista_nnls(M, Y, 0) == 0.0)
