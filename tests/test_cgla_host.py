"""constrained_griffin_lim, the parts that need no GPU: its NumPy restatement (tests/_cgla_oracle.py) - the split form the
library computes against the direct `where` on the spectrum, the exact invariants, the tie to tests/_agla_oracle.py - the C ABI
of specinv_agla_constrain (declared, bound, exported) and the argument checks of the public function, which come before the
device is required.  (SPECINV_ESTATE needs a plan, and a plan needs the device: tests/test_gpu_cgla.py.)"""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import _agla_oracle as ao
import _cgla_oracle as co
from _util import ROOT, hann, rel_l2
from oracle.stftlib import args_helper, istft, signal_length, stft
from spectrogram_inversion_amd import _lib, build
from spectrogram_inversion_amd.constrained import constrained_griffin_lim

N_FFT, HOP, FRAMES, BATCH, ITERS = 512, 128, 24, 2, 5
PARAMS = [(0.99, None, 1.0), (0.5, 1.2, 0.7)]


def _case(dtype, seed=0):
    """A real signal, its STFT (the known values), a start with random phases, the low quarter band and the two outer thirds of
    the samples known."""
    rng = np.random.default_rng(seed)
    kw = dict(hop_length=HOP, window=hann(N_FFT, dtype))
    F = N_FFT // 2 + 1
    a = args_helper(F, dtype, **kw)
    L = signal_length(FRAMES, a)
    n = np.arange(L)
    x = np.stack([np.sin(2 * np.pi * (0.01 + 0.004 * b) * n) * (1 + 0.5 * np.sin(2 * np.pi * n / 701)) for b in range(BATCH)])
    x = (x + 0.1 * rng.standard_normal(x.shape)).astype(dtype)
    K = stft(x, a)
    start = (np.abs(K) * np.exp(1j * rng.uniform(-np.pi, np.pi, K.shape))).astype(K.dtype)
    M = np.zeros((F, FRAMES), bool)
    M[: F // 4] = True
    W = np.zeros(L, bool)
    W[: L // 3] = True
    W[2 * L // 3:] = True
    return dict(start=start, K=K, M=M, x=x, W=W, kw=kw, a=a, L=L)


def _run(c, params, direct=False, iters=ITERS, spec=True, wave=True):
    alpha, beta, gamma = params
    con = {}
    if spec:
        con.update(known_spec=c["K"], spec_mask=c["M"])
    if wave:
        con.update(known_wave=c["x"], wave_mask=c["W"])
    return co.cgla(c["start"], iters, alpha=alpha, beta=beta, gamma=gamma, eva_iter=iters, direct=direct,
                   **con, **c["kw"])


@pytest.mark.parametrize("params", PARAMS, ids=["fgla", "general"])
@pytest.mark.parametrize("dtype,gate", [(np.float64, 1e-12), (np.float32, 2e-6)], ids=["f64", "f32"])
def test_split_form_is_the_direct_where_on_the_spectrum(dtype, gate, params):
    """The STFT is linear: the projection onto m' plus the constant signal k is the projection with the known bins put in."""
    c = _case(dtype)
    split, direct = _run(c, params), _run(c, params, direct=True)
    assert split.dtype == dtype and split.shape == (BATCH, c["L"]) and np.isfinite(split).all() and np.isfinite(direct).all()
    e = rel_l2(split, direct)
    print(f"split vs direct {e:.3e} gate {gate:.1e}")
    assert e <= gate
    # ... and the constraints act: neither form is the unconstrained run
    free = ao.agla(c["start"], ITERS, alpha=params[0], beta=params[1], gamma=params[2], **c["kw"])
    assert rel_l2(split, free) > 1e-2


@pytest.mark.parametrize("params", PARAMS, ids=["fgla", "general"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("direct", [False, True], ids=["split", "direct"])
def test_known_samples_come_back_bit_for_bit(dtype, params, direct):
    c = _case(dtype, seed=1)
    for iters in (1, 2, ITERS):
        y = _run(c, params, direct=direct, iters=iters)
        assert np.array_equal(y[:, c["W"]], c["x"][:, c["W"]])
        assert not np.array_equal(y[:, ~c["W"]], c["x"][:, ~c["W"]])


def test_with_all_bins_known_one_iteration_is_the_inverse_transform():
    c = _case(np.float32, seed=2)
    y = co.cgla(c["start"], 1, known_spec=c["K"], spec_mask=np.ones((1, 1), bool), eva_iter=1, **c["kw"])
    ref, _ = istft(c["K"], c["a"])
    e = rel_l2(y, ref)
    print(f"all bins known vs istft(known_spec) {e:.3e}")
    assert e <= 1e-6                                            # float32 rounding: eps = 6e-8, measured 1.2e-7
    assert rel_l2(y, c["x"]) <= 1e-5                            # ... which is the signal the bins came from


@pytest.mark.parametrize("params", PARAMS, ids=["fgla", "general"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_without_a_constraint_it_is_the_agla_oracle(dtype, params):
    c = _case(dtype, seed=3)
    ref = ao.agla(c["start"], ITERS, alpha=params[0], beta=params[1], gamma=params[2], **c["kw"])
    assert np.array_equal(_run(c, params, spec=False, wave=False), ref)
    assert np.array_equal(_run(c, params, direct=True, spec=False, wave=False), ref)
    # masks that are false everywhere: the same
    y = co.cgla(c["start"], ITERS, known_spec=c["K"], spec_mask=np.zeros((1, 1, 1), bool), known_wave=c["x"],
                wave_mask=np.zeros(1, bool), alpha=params[0], beta=params[1], gamma=params[2], **c["kw"])
    assert np.array_equal(y, ref)
    # magnitudes in: the start is phase_init, as there
    mag = np.abs(c["start"])
    assert np.array_equal(co.cgla(mag, 3, **c["kw"]), ao.agla(mag, 3, **c["kw"]))
    assert co.cgla(mag[0], 3, **c["kw"]).shape == (c["L"],)


def test_oracle_evaluates_the_result_against_the_full_target():
    c = _case(np.float64, seed=4)
    trace = []
    y = co.cgla(c["start"], 6, known_spec=c["K"], spec_mask=c["M"], known_wave=c["x"], wave_mask=c["W"], eva_iter=2, trace=trace,
                **c["kw"])
    assert [t[0] for t in trace] == [1, 3, 5]
    m_full = np.where(c["M"], np.abs(c["K"]), np.abs(c["start"]))
    S = np.abs(stft(y, c["a"]))
    assert np.isclose(trace[-1][2], np.mean((S - m_full) ** 2), rtol=1e-12)
    assert trace[-1][2] < trace[0][2]
    stopped = []
    r1 = (trace[0][2] - trace[1][2]) / trace[0][2]
    co.cgla(c["start"], 6, known_spec=c["K"], spec_mask=c["M"], known_wave=c["x"], wave_mask=c["W"], eva_iter=2, trace=stopped,
            tol=1.5 * r1, **c["kw"])
    assert [t[0] for t in stopped] == [1, 3]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def test_entry_point_is_declared_bound_and_exported(lib):
    text = re.sub(r"/\*.*?\*/", "", open(f"{ROOT}/include/specinv.h").read(), flags=re.S)
    assert re.search(r"\bint\s+specinv_agla_constrain\s*\(\s*specinv_plan\s*\*\s*plan\s*,\s*const\s+void\s*\*\s*offset\s*,"
                     r"\s*const\s+void\s*\*\s*fixed_mask\s*\)\s*;", text)
    assert _lib.SIGNATURES["specinv_agla_constrain"] == (C.c_int, [C.c_void_p] * 3)
    assert hasattr(C.CDLL(_lib.LIB_PATH), "specinv_agla_constrain")
    assert lib.specinv_agla_constrain(None, None, None) == _lib.EINVAL and "NULL" in lib.specinv_last_error().decode()
    assert lib.specinv_abi_version() == 1
    import spectrogram_inversion_amd as si
    assert si.constrained_griffin_lim is constrained_griffin_lim            # exported from the package


# ---- argument errors of the public function: all before the device is required ---------------------------------------------
def _targs(c):
    t = torch.from_numpy
    kw = dict(hop_length=HOP, window=t(c["kw"]["window"]), verbose=False, max_iter=2)
    return t(c["start"]), t(c["K"]), t(c["M"]), t(c["x"]), t(c["W"]), kw


def test_argument_errors_need_no_device():
    c = _case(np.float32)
    spec, K, M, x, W, kw = _targs(c)
    f = constrained_griffin_lim
    # a half-given pair
    for con in (dict(known_spec=K), dict(spec_mask=M), dict(known_wave=x), dict(wave_mask=W),
                dict(known_spec=K, spec_mask=M, known_wave=x)):
        with pytest.raises(ValueError, match="come together"):
            f(spec, **con, **kw)
    # masks that are not bool
    with pytest.raises(TypeError, match="spec_mask must be a bool"):
        f(spec, known_spec=K, spec_mask=M.to(torch.uint8), **kw)
    with pytest.raises(TypeError, match="wave_mask must be a bool"):
        f(spec, known_wave=x, wave_mask=W.float(), **kw)
    # a real known_spec, a complex known_wave
    with pytest.raises(TypeError, match="known_spec must be complex"):
        f(spec, known_spec=K.abs(), spec_mask=M, **kw)
    with pytest.raises(TypeError, match="known_wave must be real"):
        f(spec, known_wave=x.to(torch.complex64), wave_mask=W, **kw)
    # shapes
    with pytest.raises(ValueError, match="known_spec must have shape"):
        f(spec, known_spec=K[:, :-1], spec_mask=M, **kw)
    with pytest.raises(ValueError, match="known_spec must have shape"):
        f(spec[0], known_spec=K, spec_mask=M, **kw)
    with pytest.raises(ValueError, match="spec_mask of shape .* does not broadcast"):
        f(spec, known_spec=K, spec_mask=M[:, :-1], **kw)
    with pytest.raises(ValueError, match="wave_mask of shape .* does not broadcast"):
        f(spec, known_wave=x, wave_mask=W[:-1], **kw)
    # a known_wave of the wrong length: L belongs to the frames
    for bad in (x[:, :-1], torch.cat([x, x[:, :1]], 1), x[0]):
        with pytest.raises(ValueError, match=f"known_wave must have shape \\({BATCH}, {c['L']}\\)"):
            f(spec, known_wave=bad, wave_mask=W[: bad.shape[-1]], **kw)
    with pytest.raises(ValueError, match=f"known_wave must have shape \\({c['L']},\\)"):
        f(spec[0], known_wave=x, wave_mask=W, **kw)
    # the method's parameters, as accelerated_griffin_lim
    with pytest.raises(ValueError, match="alpha and beta"):
        f(spec, known_wave=x, wave_mask=W, alpha=-0.1, **kw)
    with pytest.raises(ValueError, match="gamma"):
        f(spec, known_wave=x, wave_mask=W, gamma=0.0, **kw)
    with pytest.raises(TypeError):
        f(c["start"], known_wave=x, wave_mask=W, **kw)
    with pytest.raises(ValueError, match=r"\(F, T\) or \(B, F, T\)"):
        f(spec[0, 0], known_wave=x, wave_mask=W, **kw)


def test_not_differentiable_and_at_most_one_plan_of_items():
    c = _case(np.float32)
    spec, K, M, x, W, kw = _targs(c)
    f = constrained_griffin_lim
    for which in range(3):
        args = [spec.clone(), K.clone(), x.clone()]
        args[which].requires_grad_(True)
        with pytest.raises(NotImplementedError, match="not differentiable"):
            f(args[0], known_spec=args[1], spec_mask=M, known_wave=args[2], wave_mask=W, **kw)
    big = torch.zeros((65536, 5, 1), dtype=torch.complex64)              # 65 536 items of one frame of 8 samples each
    with pytest.raises(ValueError, match="at most 65535"):
        f(big, known_spec=big, spec_mask=torch.ones((1, 1, 1), dtype=torch.bool), center=False, window=torch.ones(8), max_iter=1,
          verbose=False)
