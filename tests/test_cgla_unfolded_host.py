"""constrained_unfolded, the parts that need no GPU: the torch restatement the GPU tests differentiate (tests/_cgla_torch.py) against
the NumPy oracle it restates (tests/_cgla_oracle.py) and against tests/_agla_torch.py without a constraint; its autograd gradient
against central differences; the backward recursion the device runs (only c_0 and the t's recorded, one accumulator for
the constant signal's cotangent), written out in torch, against autograd of the restatement; the float32 noise of the GPU tests'
cases; the argument checks of `spectrogram_inversion_amd.constrained_unfolded`; and the C ABI of the three adjoint entries."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import _agla_torch as at
import _cgla_oracle as co
import _cgla_torch as ct
from _misi_torch import _setup, envelope, istft
from _util import ROOT, rel_l2
from spectrogram_inversion_amd import _lib, build

NAMES = ("specinv_cgla_extrap_adjoint", "specinv_cgla_step_adjoint", "specinv_cgla_first_adjoint")
N_ITER = ct.N_ITER
GENERAL = ct.SCHEDULES["general"]
FGLA = ((0.99, 0.9, 0.8, 0.95), (0.99, 0.3, 0.8, 1.5), (1.0, 1.0, 1.0, 1.0))


@pytest.fixture(scope="module")
def lib():
    build.build_lib()
    return _lib.load()


def _err(lib):
    return lib.specinv_last_error().decode()


def _torch_case(name, magnitude_start, which):
    """(spec, constraint, kw) of a float64 case as torch tensors"""
    c = ct.inputs(name, np.float64, magnitude_start)
    return torch.from_numpy(c["spec"]), {k: torch.from_numpy(v) for k, v in ct.constraint(c, which).items()}, c["kw"], c


@pytest.mark.parametrize("params", [(0.99, None, 1.0), (0.5, 1.2, 0.7)], ids=["fgla", "general"])
@pytest.mark.parametrize("which", ct.CONSTRAINTS)
@pytest.mark.parametrize("name,magnitude_start", list(ct.SEEDS))
def test_restatement_equals_the_oracle(name, magnitude_start, which, params):
    """float64, N iterations, constant parameters, the oracle's split form.  1e-12: the two differ in the order of the inverse
    transform's sums alone."""
    spec, con, kw, c = _torch_case(name, magnitude_start, which)
    alpha, beta, gamma = params
    with np.errstate(all="ignore"):
        ref = co.cgla(c["spec"], N_ITER, alpha=alpha, beta=beta, gamma=gamma, eva_iter=N_ITER, **ct.constraint(c, which), **kw)
    y = ct.cgla(spec, N_ITER, alpha=alpha, beta=beta, gamma=gamma, **con, **kw).numpy()
    e = rel_l2(y, ref)
    print(f"rel_l2 restatement vs oracle {e:.3e}")
    assert y.shape == ref.shape and e <= 1e-12, e


@pytest.mark.parametrize("sched", list(ct.SCHEDULES))
@pytest.mark.parametrize("name,magnitude_start", list(ct.SEEDS))
def test_without_a_constraint_it_is_the_agla_restatement(name, magnitude_start, sched):
    spec = torch.from_numpy(ct.inputs(name, np.float64, magnitude_start)["spec"])
    kw = ct.inputs(name, np.float64, magnitude_start)["kw"]
    al, be, ga = ct.SCHEDULES[sched]
    assert torch.equal(ct.cgla(spec, N_ITER, alpha=al, beta=be, gamma=ga, **kw), at.agla(spec, N_ITER, al, be, ga, **kw))


def _direction(x, rng):
    d = rng.standard_normal(x.shape) + (1j * rng.standard_normal(x.shape) if np.iscomplexobj(x) else 0)
    return d / np.linalg.norm(d)


@pytest.mark.parametrize("wrt", ct.GRADS)
@pytest.mark.parametrize("magnitude_start", [False, True], ids=["complex", "magnitude"])
def test_autograd_matches_a_central_difference(magnitude_start, wrt):
    """float64, 128/32, both constraints, the general schedule: d/dt of sum(w * cgla(...)) at h = 1e-6 against <grad, direction>
    along a random unit direction in each of the six inputs, relative 1e-6 - the truncation is O(h^2), the rounding about 1e-10; a
    wrong formula is off by O(1).  A direction in `spec` or `known_spec` moves masked and unmasked bins alike."""
    c = ct.inputs("128/32", np.float64, magnitude_start)
    ref = ct.reference("128/32", np.float64, magnitude_start, "general")
    k = ct.GRADS.index(wrt)
    base = dict(spec=c["spec"], known_spec=c["known_spec"], known_wave=c["known_wave"],
                **dict(zip(("alpha", "beta", "gamma"), (np.asarray(v, np.float64) for v in GENERAL))))
    d = _direction(base[wrt], np.random.default_rng(11))
    ip = float((np.conj(ref[1 + k]) * d).real.sum())

    def f(t):
        v = dict(base)
        v[wrt] = base[wrt] + t * d
        y = ct.cgla(torch.from_numpy(v["spec"]), N_ITER, torch.from_numpy(v["known_spec"]), torch.from_numpy(c["spec_mask"]),
                    torch.from_numpy(v["known_wave"]), torch.from_numpy(c["wave_mask"]), torch.from_numpy(v["alpha"]),
                    torch.from_numpy(v["beta"]), torch.from_numpy(v["gamma"]), **c["kw"])
        return float((y.numpy() * c["w"]).sum())

    h = 1e-6
    fd = (f(h) - f(-h)) / (2 * h)
    print(f"d/d{wrt}: central difference {fd:.12e}  <grad, direction> {ip:.12e}  relative {abs(fd - ip) / abs(fd):.3e}")
    assert abs(fd - ip) <= 1e-6 * abs(fd), (fd, ip)


def _sweep(spec, con, sched, g_y, kw):
    """The recursion of DESIGN 3.18 in torch, float64: the gradients in the order of ct.GRADS.  The forward records c_0 and
    t_1 ... t_N and nothing else; the projection's own adjoint and the chain from the start to the inputs are autograd's."""
    n_iter = len(sched[0])
    al, be, ga = (torch.tensor(v, dtype=torch.float64) for v in sched)
    general = bool((ga != 1).any())
    t = []
    with torch.no_grad():
        ct.cgla(spec, n_iter, alpha=al, beta=be, gamma=ga, record=t, **con, **kw)     # t[0] = c_0, t[n] = t_n
    F, T = spec.shape[1:]
    a_, w = _setup(F, torch.float64, kw)
    env = envelope(T, a_, w)
    s_in = spec.detach().clone().requires_grad_(True)
    m = s_in.abs() if s_in.is_complex() else s_in
    leaves = [s_in]
    if "known_spec" in con:
        K = con["known_spec"].detach().clone().requires_grad_(True)
        M = con["spec_mask"]
        leaves.append(K)
        m_full, m_free = torch.where(M, K.abs(), m), torch.where(M, torch.zeros_like(m), m)
        start = torch.where(M, K, s_in if s_in.is_complex() else at.phase_init(m_full, a_))
        k = istft(torch.where(M, K, torch.zeros_like(K)), a_, w, env)
    else:
        m_free, k = m, None
        start = s_in if s_in.is_complex() else at.phase_init(m, a_)
    c0 = istft(start, a_, w, env)
    W = con.get("wave_mask", torch.zeros(g_y.shape, dtype=torch.bool))
    zero = torch.zeros_like(g_y)

    def proj_adjoint(c_prev, gy):
        """(P'(c_prev)^T gy, dP/dm'^T gy) at the recorded point"""
        c = c_prev.detach().clone().requires_grad_(True)
        mm = m_free.detach().clone().requires_grad_(True)
        return torch.autograd.grad(at.project(c, mm, a_, w, env), (c, mm), gy)

    a, gc, gd, goff = g_y.clone(), zero.clone(), zero.clone(), zero.clone()
    gm = torch.zeros_like(m.detach())
    bars = torch.zeros((3, n_iter), dtype=torch.float64)
    for n in range(n_iter, 1, -1):
        an, bn, gn = al[n - 1], be[n - 1], ga[n - 1]
        delta = t[n] - t[n - 1]
        s = a + (1 + an) * gc + ((1 + bn) * gd if general else 0)
        sp = torch.where(W, zero, s)
        if n > 2:
            c_prev = t[n - 1] + al[n - 2] * (t[n - 1] - t[n - 2])
            d_prev = t[n - 1] + be[n - 2] * (t[n - 1] - t[n - 2])
        else:
            c_prev = d_prev = t[1]
        bars[0, n - 1] = (gc * delta).sum()
        bars[1, n - 1] = (gd * delta).sum() if general else 0.0
        bars[2, n - 1] = (sp * (t[n] - d_prev) / gn).sum()
        goff = goff + torch.where(W, s, gn * sp)
        a = -an * gc - (bn * gd if general else 0)
        if general:
            gd = (1 - gn) * sp
        gc, gmi = proj_adjoint(c_prev, gn * sp)
        gm += gmi
    s = a + gc + (gd if general else 0)
    goff = goff + s
    gc, gmi = proj_adjoint(t[0], torch.where(W, zero, s))
    gm += gmi
    outs, cots = [c0, m_free], [gc, gm]
    if k is not None:
        outs.append(k)
        cots.append(torch.where(W, zero, goff))
    g = list(torch.autograd.grad(outs, leaves, cots))
    g_K = g[1] if k is not None else None
    g_xk = torch.where(W, goff, zero) if "known_wave" in con else None
    return g[0], g_K, g_xk, bars[0], bars[1], bars[2]


@pytest.mark.parametrize("n_iter", [1, 2, 4])
@pytest.mark.parametrize("form", ["general", "fgla"])
@pytest.mark.parametrize("which", ct.CONSTRAINTS)
@pytest.mark.parametrize("magnitude_start", [False, True], ids=["complex", "magnitude"])
@pytest.mark.parametrize("name", ["128/32", "64/16 two-sided normalized"])
def test_backward_recursion_equals_autograd(name, magnitude_start, which, form, n_iter):
    """1e-10 in float64: the recursion is exact, the recomputed c_{n-1}, d_{n-1} differ from the forward's at rounding.  Gradients
    that are identically zero (every element 0, alpha_N and beta_N, beta with every gamma = 1, `spec` under the mask, `known_spec`
    off it, `known_wave` off its mask) must be exactly so."""
    spec, con, kw, c = _torch_case(name, magnitude_start, which)
    sched = tuple(v[:n_iter] for v in (GENERAL if form == "general" else FGLA))
    s = spec.clone().requires_grad_(True)
    live = {k: (v.clone().requires_grad_(True) if v.dtype != torch.bool else v) for k, v in con.items()}
    par = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in sched]
    y = ct.cgla(s, n_iter, alpha=par[0], beta=par[1], gamma=par[2], **live, **kw)
    g_y = torch.from_numpy(np.random.default_rng(3).standard_normal(tuple(y.shape)))
    wrt = {"spec": s, "known_spec": live.get("known_spec"), "known_wave": live.get("known_wave"), "alpha": par[0], "beta": par[1],
           "gamma": par[2]}
    has = [k for k in ct.GRADS if wrt[k] is not None]
    ref = torch.autograd.grad(y, [wrt[k] for k in has], g_y, allow_unused=True)       # (n_iter = 1 never reads a parameter)
    ref = {k: torch.zeros_like(wrt[k]) if r is None else r for k, r in zip(has, ref)}
    got = dict(zip(ct.GRADS, _sweep(spec, con, sched, g_y, kw)))
    for k in has:
        g, r = got[k], ref[k]
        if r.abs().max() == 0:
            assert g.abs().max() == 0, k
            continue
        e = rel_l2(g.numpy(), r.numpy())
        print(f"{k}: rel_l2 {e:.3e}")
        assert e <= 1e-10, (k, e)
        if k in ("alpha", "beta", "gamma"):
            assert g[0] == 0 and r[0] == 0, k                    # iteration 1 does not extrapolate
    if "known_spec" in con:
        M = con["spec_mask"]
        assert not got["spec"][M].any() and not got["known_spec"][~M].any() and got["known_spec"][M].abs().min() > 0
    if "known_wave" in con:
        assert not got["known_wave"][~con["wave_mask"]].any()


@pytest.mark.parametrize("sched", list(ct.SCHEDULES))
@pytest.mark.parametrize("which", ct.CONSTRAINTS)
@pytest.mark.parametrize("name,magnitude_start", ct.FLOAT32_CASES)
def test_float32_noise_of_the_gpu_cases(name, magnitude_start, which, sched):
    """The restatement's own float32-against-float64 gradient error on every case tests/test_gpu_cgla_unfolded.py runs in float32
    stays at or below 1e-3, the cap of tests/test_agla_unfolded_host.py (the seeds of _cgla_torch.SEEDS were chosen for that): the
    device's float32 gate, the larger of 2e-4 and 6 times this figure, is then never wider than 6e-3."""
    r32 = ct.reference(name, np.float32, magnitude_start, sched, which)
    r64 = ct.reference(name, np.float32, magnitude_start, sched, which, np.float64)
    for what, g32, g64 in zip(ct.GRADS, r32[1:], r64[1:]):
        if g64 is None:
            assert g32 is None
            continue
        if np.abs(g64).max() == 0:
            assert np.abs(g32).max() == 0, what
            continue
        e = rel_l2(g32, g64)
        print(f"{name} {which} {sched} grad {what}: float32 vs float64 {e:.3e}")
        assert e <= 1e-3, (what, e)


def test_python_argument_errors_need_no_gpu():
    from spectrogram_inversion_amd import constrained_griffin_lim, constrained_unfolded
    mag = torch.rand(2, 65, 9)
    K = torch.randn(2, 65, 9, dtype=torch.complex64)
    M = torch.zeros(2, 65, 9, dtype=torch.bool)
    L = 8 * 32
    xk, W = torch.randn(2, L), torch.zeros(2, L, dtype=torch.bool)
    kw = dict(hop_length=32)
    with pytest.raises(TypeError):
        constrained_unfolded(mag.numpy(), K, M, **kw)
    with pytest.raises(ValueError, match=r"\(65,\)"):
        constrained_unfolded(mag[0, :, 0], K, M, **kw)
    # the pairs, as constrained_griffin_lim
    with pytest.raises(ValueError, match="come together"):
        constrained_unfolded(mag, known_spec=K, **kw)
    with pytest.raises(ValueError, match="come together"):
        constrained_unfolded(mag, wave_mask=W, **kw)
    with pytest.raises(TypeError, match="bool"):
        constrained_unfolded(mag, K, M.to(torch.uint8), **kw)
    with pytest.raises(TypeError, match="complex"):
        constrained_unfolded(mag, K.real, M, **kw)
    with pytest.raises(TypeError, match="real"):
        constrained_unfolded(mag, known_wave=xk.to(torch.complex64), wave_mask=W, **kw)
    with pytest.raises(ValueError, match="known_spec must have shape"):
        constrained_unfolded(mag, K[:, :-1], M[:, :-1], **kw)
    with pytest.raises(ValueError, match="does not broadcast"):
        constrained_unfolded(mag, K, M[:, :-1], **kw)
    with pytest.raises(ValueError, match="known_wave must have shape"):
        constrained_unfolded(mag, known_wave=xk[:, :-1], wave_mask=W[:, :-1], **kw)
    with pytest.raises(ValueError, match="does not broadcast"):
        constrained_unfolded(mag, known_wave=xk, wave_mask=W[:, :-1], **kw)
    # n_iter and the parameters, as agla_unfolded - with a pair and with neither
    for con in (dict(known_spec=K, spec_mask=M), dict(known_wave=xk, wave_mask=W), {}):
        for bad in (0, -2, 2.5, None, True):
            with pytest.raises(ValueError, match="n_iter"):
                constrained_unfolded(mag, n_iter=bad, **con, **kw)
        for name in ("alpha", "beta", "gamma"):
            with pytest.raises(ValueError, match=name + r".*n_iter = 3"):
                constrained_unfolded(mag, n_iter=3, **con, **kw, **{name: torch.full((2,), 0.5)})
            with pytest.raises(TypeError, match=name):
                constrained_unfolded(mag, n_iter=3, **con, **kw, **{name: torch.zeros(3, dtype=torch.complex64)})
            with pytest.raises(TypeError, match=name):
                constrained_unfolded(mag, n_iter=3, **con, **kw, **{name: "0.5"})
        with pytest.raises(TypeError, match="gamma"):
            constrained_unfolded(mag, n_iter=3, gamma=None, **con, **kw)
        for par in (dict(alpha=-0.1), dict(beta=-1.0), dict(gamma=0.0), dict(alpha=float("nan")),
                    dict(alpha=torch.tensor([0.5, -0.5, 0.5])), dict(beta=torch.tensor([0.5, 0.5, -1e-9])),
                    dict(gamma=torch.tensor([1.0, 0.0, 1.0])), dict(gamma=torch.tensor(0.0, requires_grad=True))):
            with pytest.raises(ValueError, match="must be >"):
                constrained_unfolded(mag, n_iter=3, **con, **kw, **par)
    with pytest.raises(TypeError, match="int32"):
        constrained_unfolded(mag.to(torch.int32), K, M, **kw)
    # the batch limit, with and without a gradient to compute: no slice plans
    big = torch.rand(65536, 3, 2)
    for grad in (False, True):
        with pytest.raises(ValueError, match="65536 items"):
            constrained_unfolded(big.clone().requires_grad_(grad), known_wave=torch.zeros(65536, 1), wave_mask=torch.zeros(1, dtype=torch.bool),
                                 hop_length=1)
    with pytest.raises(TypeError, match="positional"):
        constrained_unfolded(mag, K, M, xk, W, 3, 0.5, 0.5, 1.0, 1e-6, **kw)                # no tol, eva_iter, metric, verbose
    # constrained_griffin_lim itself stays as it is
    for con in (dict(known_spec=K.clone().requires_grad_(True), spec_mask=M), dict(known_wave=xk.clone().requires_grad_(True), wave_mask=W)):
        with pytest.raises(NotImplementedError, match="not differentiable"):
            constrained_griffin_lim(mag, max_iter=3, **con, **kw)
    with pytest.raises(NotImplementedError, match="not differentiable"):
        constrained_griffin_lim(mag.clone().requires_grad_(True), K, M, max_iter=3, **kw)


def test_symbols_are_declared_bound_and_exported(lib):
    from spectrogram_inversion_amd.plan import Plan
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
        assert callable(getattr(Plan, name[len("specinv_"):])), name
    assert lib.specinv_abi_version() == 1


def test_argument_errors_do_not_need_a_gpu(lib):
    buf = C.c_void_p(16)                      # never dereferenced: every call below fails its checks first
    coef = (C.c_double * 5)(0.5, 1.2, 0.7, 0.4, 1.1)
    for fn, extra in ((lib.specinv_cgla_extrap_adjoint, ()), (lib.specinv_cgla_step_adjoint, (buf, buf))):
        # plan, t_n, t_nm1, t_nm2, coef, fixed_mask, a, gc, gd, goff, c_prev, dots
        for i, name in ((0, "t_n"), (1, "t_nm1"), (5, "a_inout"), (6, "gc_inout"), (8, "goff_accum"), (9, "c_prev_out"),
                        (10, "dots_dev_out")):
            ptrs = [buf, buf, buf, coef, buf, buf, buf, buf, buf, buf, buf]
            ptrs[i] = None
            assert fn(None, *ptrs, *extra) == _lib.EINVAL and name in _err(lib), name
        assert fn(None, buf, buf, buf, None, buf, buf, buf, buf, buf, buf, buf, *extra) == _lib.EINVAL and "coef" in _err(lib)
        for bad, word in (((-0.5, 1.2, 0.7, 0.4, 1.1), "alpha"), ((0.5, 1.2, 0.7, 0.4, -1.1), "beta"), ((0.5, 1.2, 0.0, 0.4, 1.1), "gamma")):
            assert fn(None, buf, buf, buf, (C.c_double * 5)(*bad), buf, buf, buf, buf, buf, buf, buf, *extra) == _lib.EINVAL
            assert word in _err(lib)
        assert fn(None, buf, buf, buf, coef, buf, buf, buf, None, buf, buf, buf, *extra) == _lib.EINVAL and "gd_inout" in _err(lib)
        # t_nm2 and fixed_mask may be NULL
        assert fn(None, buf, buf, None, coef, None, buf, buf, buf, buf, buf, buf, *extra) == _lib.EINVAL and "plan" in _err(lib)
    for i, name in enumerate(("mag_fm", "gmag_fm_accum")):
        extra = [None if j == i else buf for j in range(2)]
        assert lib.specinv_cgla_step_adjoint(None, buf, buf, buf, coef, buf, buf, buf, buf, buf, buf, buf, *extra) == _lib.EINVAL
        assert name in _err(lib), name
    # plan, c0, fixed_mask, a, gc, gd, goff, mag_fm, gmag_fm
    for i, name in ((0, "c0"), (2, "a"), (3, "gc_inout"), (5, "goff_accum"), (6, "mag_fm"), (7, "gmag_fm_accum")):
        ptrs = [buf] * 8
        ptrs[i] = None
        assert lib.specinv_cgla_first_adjoint(None, *ptrs) == _lib.EINVAL and name in _err(lib), name
    # fixed_mask and gd may be NULL
    assert lib.specinv_cgla_first_adjoint(None, buf, None, buf, buf, None, buf, buf, buf) == _lib.EINVAL and "plan" in _err(lib)
