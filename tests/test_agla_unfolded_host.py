"""agla_unfolded, the parts that need no GPU: the torch restatement the GPU tests differentiate (tests/_agla_torch.py) against the
NumPy oracle it restates (tests/_agla_oracle.py); the backward recursion the device runs (only c_0 and the t's
recorded, c_{n-1} and d_{n-1} recomputed from them), written out in torch, against autograd of the restatement; the float32 noise
of the GPU tests' cases; the argument checks of `spectrogram_inversion_amd.agla_unfolded`; and the C ABI of specinv_agla_init_sched
and the three adjoint entries (declared, bound, exported, argument errors)."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import _agla_oracle as ao
import _agla_torch as at
from _misi_torch import _setup, envelope, istft
from _util import ROOT, hann, rel_l2
from spectrogram_inversion_amd import _lib, build

NAMES = ("specinv_agla_init_sched", "specinv_agla_extrap_adjoint", "specinv_agla_step_adjoint", "specinv_agla_first_adjoint")

# n_fft, hop, extra stft kwargs
CONFIGS = [(128, 32, {}), (64, 16, dict(onesided=False, pad_mode="constant"))]
GENERAL = ((0.5, 0.45, 0.6, 0.55), (1.2, 1.1, 1.3, 1.25), (0.7, 0.8, 0.65, 0.75))
FGLA = ((0.99, 0.9, 0.8, 0.95), (0.99, 0.3, 0.8, 1.5), (1.0, 1.0, 1.0, 1.0))


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def _err(lib):
    return lib.specinv_last_error().decode()


def _start(n_fft, hop, extra, magnitude_start, T=10, B=2):
    rng = np.random.default_rng(n_fft + hop)
    F = n_fft // 2 + 1 if extra.get("onesided", True) else n_fft
    kw = dict(hop_length=hop, window=hann(n_fft, np.float64), **extra)
    mag = rng.random((B, F, T)) + 0.05
    return (mag if magnitude_start else mag * np.exp(1j * rng.uniform(-np.pi, np.pi, mag.shape))), kw


@pytest.mark.parametrize("params", [(0.99, None, 1.0), (0.5, 1.2, 0.7)], ids=["fgla", "general"])
@pytest.mark.parametrize("magnitude_start", [False, True], ids=["complex", "magnitude"])
@pytest.mark.parametrize("n_fft,hop,extra", CONFIGS)
def test_restatement_equals_the_oracle(n_fft, hop, extra, magnitude_start, params):
    """float64, 5 iterations, constant parameters.  1e-12: the two differ in the order of the inverse transform's sums alone (MISI's
    restatement sits at 2e-15 of its oracle)."""
    spec, kw = _start(n_fft, hop, extra, magnitude_start)
    alpha, beta, gamma = params
    with np.errstate(all="ignore"):
        ref = ao.agla(spec, 5, alpha=alpha, beta=beta, gamma=gamma, **kw)
    y = at.agla(torch.from_numpy(spec), 5, alpha, beta, gamma, **kw).numpy()
    e = rel_l2(y, ref)
    print(f"rel_l2 restatement vs oracle {e:.3e}")
    assert y.shape == ref.shape and e <= 1e-12, e


def _sweep(spec, sched, g_y, kw):
    """The recursion of DESIGN 3.14 in torch, float64: (grad spec, alpha_bar, beta_bar, gamma_bar).  The forward records c_0 and
    t_1 ... t_N and nothing else; the projection's own adjoint is autograd's on one projection."""
    n_iter = len(sched[0])
    al, be, ga = (torch.tensor(v, dtype=torch.float64) for v in sched)
    general = bool((ga != 1).any())
    rec = []
    with torch.no_grad():
        at.agla(spec, n_iter, al, be, ga, record=rec, **kw)
    t = rec                                                      # t[0] = c_0, t[n] = t_n
    F, T = spec.shape[1:]
    a_, w = _setup(F, torch.float64, kw)
    env = envelope(T, a_, w)
    s_in = spec.detach().clone().requires_grad_(True)
    m = s_in.abs() if s_in.is_complex() else s_in
    c0 = istft(s_in if s_in.is_complex() else at.phase_init(s_in, a_), a_, w, env)

    def proj_adjoint(c_prev, gy):
        """(P'(c_prev)^T gy, dP/dm^T gy) at the recorded point"""
        c = c_prev.detach().clone().requires_grad_(True)
        mm = m.detach().clone().requires_grad_(True)
        return torch.autograd.grad(at.project(c, mm, a_, w, env), (c, mm), gy)

    a, gc, gd = g_y.clone(), torch.zeros_like(g_y), torch.zeros_like(g_y)
    gm = torch.zeros_like(m.detach())
    bars = torch.zeros((3, n_iter), dtype=torch.float64)
    for n in range(n_iter, 1, -1):
        an, bn, gn = al[n - 1], be[n - 1], ga[n - 1]
        delta = t[n] - t[n - 1]
        s = a + (1 + an) * gc + ((1 + bn) * gd if general else 0)
        if n > 2:
            c_prev = t[n - 1] + al[n - 2] * (t[n - 1] - t[n - 2])
            d_prev = t[n - 1] + be[n - 2] * (t[n - 1] - t[n - 2])
        else:
            c_prev = d_prev = t[1]
        bars[0, n - 1] = (gc * delta).sum()
        bars[1, n - 1] = (gd * delta).sum() if general else 0.0
        bars[2, n - 1] = (s * (t[n] - d_prev) / gn).sum()
        a = -an * gc - (bn * gd if general else 0)
        if general:
            gd = (1 - gn) * s
        gc, gmi = proj_adjoint(c_prev, gn * s)
        gm += gmi
    gc, gmi = proj_adjoint(t[0], a + gc + (gd if general else 0))
    gm += gmi
    g_spec, = torch.autograd.grad((c0, m), s_in, (gc, gm))
    return g_spec, bars[0], bars[1], bars[2]


@pytest.mark.parametrize("n_iter", [1, 2, 4])
@pytest.mark.parametrize("form", ["general", "fgla"])
@pytest.mark.parametrize("magnitude_start", [False, True], ids=["complex", "magnitude"])
@pytest.mark.parametrize("n_fft,hop,extra", CONFIGS)
def test_backward_recursion_equals_autograd(n_fft, hop, extra, magnitude_start, form, n_iter):
    """1e-10 in float64: the recursion is exact, the recomputed c_{n-1}, d_{n-1} differ from the forward's at rounding.  Gradients
    that are identically zero (every element 0, alpha_N and beta_N, beta with every gamma = 1) must be exactly so."""
    spec, kw = _start(n_fft, hop, extra, magnitude_start)
    sched = tuple(v[:n_iter] for v in (GENERAL if form == "general" else FGLA))
    spec = torch.from_numpy(spec)
    s = spec.clone().requires_grad_(True)
    par = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in sched]
    y = at.agla(s, n_iter, *par, **kw)
    g_y = torch.from_numpy(np.random.default_rng(3).standard_normal(tuple(y.shape)))
    ref = torch.autograd.grad(y, (s, *par), g_y, allow_unused=True)               # (n_iter = 1 never reads a parameter)
    ref = [torch.zeros_like(x) if r is None else r for r, x in zip(ref, (s, *par))]
    got = _sweep(spec, sched, g_y, kw)
    for name, g, r in zip(("spec", "alpha", "beta", "gamma"), got, ref):
        if r.abs().max() == 0:
            assert g.abs().max() == 0, name
            continue
        e = rel_l2(g.numpy(), r.numpy())
        print(f"{name}: rel_l2 {e:.3e}")
        assert e <= 1e-10, (name, e)
        if name != "spec":
            assert g[0] == 0 and r[0] == 0, name                 # iteration 1 does not extrapolate
    assert n_iter == 1 or ref[3][1:].abs().min() > 0             # gamma's gradient lives in both forms


@pytest.mark.parametrize("sched", list(at.SCHEDULES))
@pytest.mark.parametrize("name,magnitude_start", at.FLOAT32_CASES)
def test_float32_noise_of_the_gpu_cases(name, magnitude_start, sched):
    """The restatement's own float32-against-float64 gradient error on every case tests/test_gpu_agla_unfolded.py runs in float32
    stays at or below 1e-3 (the seeds of _agla_torch.SEEDS were chosen for that): the device's float32 gate, the larger of 2e-4 and
    6 times this figure, is then never wider than 6e-3."""
    r32 = at.reference(name, np.float32, magnitude_start, sched)
    r64 = at.reference(name, np.float32, magnitude_start, sched, np.float64)
    for what, g32, g64 in zip(("spec", "alpha", "beta", "gamma"), r32[1:], r64[1:]):
        if np.abs(g64).max() == 0:
            assert np.abs(g32).max() == 0, what
            continue
        e = rel_l2(g32, g64)
        print(f"{name} {sched} grad {what}: float32 vs float64 {e:.3e}")
        assert e <= 1e-3, (what, e)


def test_python_argument_errors_need_no_gpu():
    from spectrogram_inversion_amd import accelerated_griffin_lim, agla_unfolded
    mag = torch.rand(2, 65, 9, requires_grad=True)
    with pytest.raises(TypeError):
        agla_unfolded(mag.detach().numpy())
    with pytest.raises(ValueError, match=r"\(65,\)"):
        agla_unfolded(mag[0, :, 0], hop_length=32)
    with pytest.raises(TypeError):
        agla_unfolded(mag.detach().to(torch.int32), hop_length=32)
    for bad in (0, -2, 2.5, None, True):
        with pytest.raises(ValueError, match="n_iter"):
            agla_unfolded(mag, n_iter=bad, hop_length=32)
    # parameter shapes and kinds
    for name in ("alpha", "beta", "gamma"):
        with pytest.raises(ValueError, match=name + r".*n_iter = 3"):
            agla_unfolded(mag, 3, hop_length=32, **{name: torch.full((2,), 0.5)})
        with pytest.raises(ValueError, match=name):
            agla_unfolded(mag, 3, hop_length=32, **{name: torch.zeros(0)})
        with pytest.raises(TypeError, match=name):
            agla_unfolded(mag, 3, hop_length=32, **{name: torch.zeros(3, dtype=torch.complex64)})
        with pytest.raises(TypeError, match=name):
            agla_unfolded(mag, 3, hop_length=32, **{name: "0.5"})
    with pytest.raises(TypeError, match="gamma"):
        agla_unfolded(mag, 3, hop_length=32, gamma=None)
    # ranges, as accelerated_griffin_lim: constants and single entries of a schedule
    for kw in (dict(alpha=-0.1), dict(beta=-1.0), dict(gamma=0.0), dict(gamma=-1.0), dict(alpha=float("nan")),
               dict(alpha=torch.tensor([0.5, -0.5, 0.5])), dict(beta=torch.tensor([0.5, 0.5, -1e-9])),
               dict(gamma=torch.tensor([1.0, 0.0, 1.0])), dict(gamma=torch.tensor(0.0, requires_grad=True))):
        with pytest.raises(ValueError, match="must be >"):
            agla_unfolded(mag, 3, hop_length=32, **kw)
    # the batch limit, with and without a gradient to compute: no slice plans
    for grad in (False, True):
        with pytest.raises(ValueError, match="65536 items"):
            agla_unfolded(torch.rand(65536, 3, 2, requires_grad=grad), hop_length=1)
    with pytest.raises(TypeError, match="positional"):
        agla_unfolded(mag, 3, 0.5, 0.5, 1.0, 1e-6, hop_length=32)                           # no tol, eva_iter, metric, verbose
    # accelerated_griffin_lim itself stays as it is
    with pytest.raises(NotImplementedError, match="not differentiable"):
        accelerated_griffin_lim(mag, max_iter=3, hop_length=32)


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
    D3 = C.c_double * 3
    ok = D3(0.5, 0.5, 0.5)
    for n in (0, -1):
        assert lib.specinv_agla_init_sched(None, buf, None, n, ok, ok, ok) == _lib.EINVAL and "n_sched" in _err(lib)
    for i, name in enumerate(("alpha", "beta", "gamma")):
        arrs = [None if j == i else ok for j in range(3)]
        assert lib.specinv_agla_init_sched(None, buf, None, 3, *arrs) == _lib.EINVAL and name in _err(lib), name
    assert lib.specinv_agla_init_sched(None, buf, None, 3, D3(0.5, -0.1, 0.5), ok, ok) == _lib.EINVAL and "alpha" in _err(lib)
    assert lib.specinv_agla_init_sched(None, buf, None, 3, ok, D3(0.5, 0.5, -2.0), ok) == _lib.EINVAL and "beta" in _err(lib)
    assert lib.specinv_agla_init_sched(None, buf, None, 3, ok, ok, D3(1.0, 0.0, 1.0)) == _lib.EINVAL and "gamma" in _err(lib)
    assert lib.specinv_agla_init_sched(None, buf, None, 3, ok, ok, ok) == _lib.EINVAL and "plan" in _err(lib)
    assert lib.specinv_agla_init(None, buf, None, -1.0, 0.5, 1.0) == _lib.EINVAL and "alpha" in _err(lib)      # the n_sched = 1 case
    coef = (C.c_double * 5)(0.5, 1.2, 0.7, 0.4, 1.1)
    for fn, extra in ((lib.specinv_agla_extrap_adjoint, ()), (lib.specinv_agla_step_adjoint, (buf, buf))):
        # plan, t_n, t_nm1, t_nm2, coef, a, gc, gd, c_prev, dots
        for i, name in ((0, "t_n"), (1, "t_nm1"), (4, "a_inout"), (5, "gc_inout"), (7, "c_prev_out"), (8, "dots_dev_out")):
            ptrs = [buf, buf, buf, coef, buf, buf, buf, buf, buf]
            ptrs[i] = None
            assert fn(None, *ptrs, *extra) == _lib.EINVAL and name in _err(lib), name
        assert fn(None, buf, buf, buf, None, buf, buf, buf, buf, buf, *extra) == _lib.EINVAL and "coef" in _err(lib)
        for bad, word in (((-0.5, 1.2, 0.7, 0.4, 1.1), "alpha"), ((0.5, 1.2, 0.7, 0.4, -1.1), "beta"), ((0.5, 1.2, 0.0, 0.4, 1.1), "gamma")):
            assert fn(None, buf, buf, buf, (C.c_double * 5)(*bad), buf, buf, buf, buf, buf, *extra) == _lib.EINVAL and word in _err(lib)
        assert fn(None, buf, buf, buf, coef, buf, buf, None, buf, buf, *extra) == _lib.EINVAL and "gd_inout" in _err(lib)   # gamma != 1
        assert fn(None, buf, buf, None, coef, buf, buf, buf, buf, buf, *extra) == _lib.EINVAL and "plan" in _err(lib)       # t_nm2 may be NULL
    for i, name in enumerate(("mag_fm", "gmag_fm_accum")):
        extra = [None if j == i else buf for j in range(2)]
        assert lib.specinv_agla_step_adjoint(None, buf, buf, buf, coef, buf, buf, buf, buf, buf, *extra) == _lib.EINVAL
        assert name in _err(lib), name
    # plan, c0, a, gc, gd, mag_fm, gmag_fm
    for i, name in ((0, "c0"), (1, "a"), (2, "gc_inout"), (4, "mag_fm"), (5, "gmag_fm_accum")):
        ptrs = [buf] * 6
        ptrs[i] = None
        assert lib.specinv_agla_first_adjoint(None, *ptrs) == _lib.EINVAL and name in _err(lib), name
    assert lib.specinv_agla_first_adjoint(None, buf, buf, buf, None, buf, buf) == _lib.EINVAL and "plan" in _err(lib)     # gd may be NULL
