"""`agla_unfolded` on the device: its forward against `accelerated_griffin_lim` (bits) and the torch restatement of the AGLA oracle
(tests/_agla_torch.py), its gradients against autograd on that restatement and against central differences of the inference path,
`specinv_agla_extrap_adjoint` (csrc/kernels_agla_adjoint.h) alone against NumPy, and the layer's properties.  Needs an MI355X:
`-m gpu`."""
import numpy as np
import pytest
import torch

import _agla_torch as at
from _util import hann, rel_l2

pytestmark = pytest.mark.gpu

import spectrogram_inversion_amd as si                                    # noqa: E402
from spectrogram_inversion_amd.plan import Plan, args_helper, clear_plan_cache, get_plan   # noqa: E402

DEV = torch.device("cuda", 0)
N_ITER = at.N_ITER
TDT = {np.float32: torch.float32, np.float64: torch.float64}
F32_FLOOR = 2e-5                # tests/test_gpu_agla.py's float32 forward gate


def N(t):
    return t.detach().cpu().numpy()


def T_(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture
def route(monkeypatch):
    """`route(name)` before a case's first plan: 1024/256 takes the fused, chunk-walking kernel (conftest's chunked_kernel rule),
    every other case the plan's own routing for small problems; the plan cache never mixes the two."""
    def go(name):
        if name == "1024/256":
            monkeypatch.setenv("SPECINV_SMALL_FRAMES", "0")
        clear_plan_cache()
    yield go
    clear_plan_cache()


def _tkw(kw):
    return dict(kw, window=torch.from_numpy(kw["window"]))


def _params(sched, grad=True, device="cpu"):
    """alpha, beta, gamma as (N_ITER,) float64 tensors (beta spelled out where the schedule says None: its gradient is compared)"""
    al, be, ga = at.SCHEDULES[sched]
    return [at.schedule(v, N_ITER).clone().to(device).requires_grad_(grad) for v in (al, al if be is None else be, ga)]


def _device(name, dtype, magnitude_start, sched):
    """(y, grad spec, grad alpha, grad beta, grad gamma) of sum(w * agla_unfolded(...)) on the device, as NumPy arrays"""
    spec, w, L, kw = at.inputs(name, dtype, magnitude_start)
    s, par = T_(spec).requires_grad_(True), _params(sched)
    y = si.agla_unfolded(s, N_ITER, *par, **_tkw(kw))
    assert y.requires_grad and y.shape == w.shape
    with torch.no_grad():
        # the output under grad is the inference path's, bit for bit
        assert torch.equal(y, si.agla_unfolded(s, N_ITER, *par, **_tkw(kw)))
    (y * T_(w)).sum().backward()
    assert s.grad.shape == s.shape and s.grad.dtype == s.dtype
    for p in par:
        assert p.grad.shape == (N_ITER,) and p.grad.dtype == torch.float64 and p.grad.device.type == "cpu"
        assert p.grad[0] == 0                                        # iteration 1 does not extrapolate
    if sched == "fgla":
        assert not par[1].grad.any()                                 # every gamma = 1: beta has no effect, exactly
    return (N(y), N(s.grad)) + tuple(N(p.grad) for p in par)


FORWARD = [(n, m, d) for n, m in at.FLOAT32_CASES for d in (np.float32, np.float64) if not (d == np.float64 and n == "1024/256")]


@pytest.mark.parametrize("name,magnitude_start,dtype", FORWARD + [("400/160", True, np.float64), ("1024/256", True, np.float32)])
def test_constant_parameters_are_accelerated_griffin_lim(route, name, magnitude_start, dtype):
    """No gradient and constant parameters: the bits of accelerated_griffin_lim(max_iter=n_iter, tol=0), floats or tensors; under
    grad the same bits again."""
    route(name)
    spec, w, L, kw = at.inputs(name, dtype, magnitude_start)
    for al, be, ga in ((0.99, None, 1.0), (0.5, 1.2, 0.7)):
        ref = si.accelerated_griffin_lim(T_(spec), max_iter=N_ITER, tol=0, verbose=False, alpha=al, beta=be, gamma=ga, **_tkw(kw))
        y = si.agla_unfolded(T_(spec), N_ITER, al, be, ga, **_tkw(kw))
        assert not y.requires_grad and torch.equal(y, ref)
        as_tensors = [None if v is None else torch.full((N_ITER,), v, dtype=torch.float64) for v in (al, be, ga)]
        assert torch.equal(si.agla_unfolded(T_(spec), N_ITER, *as_tensors, **_tkw(kw)), ref)
        yg = si.agla_unfolded(T_(spec).requires_grad_(True), N_ITER, al, be, torch.tensor(ga, dtype=torch.float64, requires_grad=True),
                              **_tkw(kw))
        assert yg.requires_grad and torch.equal(yg.detach(), ref)
    geo = get_plan(args_helper(T_(spec), **_tkw(kw)), 2, spec.shape[2], TDT[dtype], DEV).launch_geometry
    if dtype == np.float32 and name != "64/16 two-sided normalized":
        assert geo["kernel"] == ("k_fused4" if name == "1024/256" else "k_wave_iter"), geo
        assert name != "1024/256" or geo["chunks"] == 2, geo


@pytest.mark.parametrize("sched", list(at.SCHEDULES))
@pytest.mark.parametrize("name,magnitude_start,dtype", FORWARD + [("400/160", True, np.float64)])
def test_forward_matches_the_restatement(route, name, magnitude_start, dtype, sched):
    """float64: 1e-10.  float32: the larger of 2e-5 and 6 x the restatement's own float32-against-float64 rel-L2 on the case, the
    rule of tests/test_gpu_agla.py."""
    route(name)
    spec, w, L, kw = at.inputs(name, dtype, magnitude_start)
    y = N(si.agla_unfolded(T_(spec), N_ITER, *_params(sched, grad=False), **_tkw(kw)))
    ref = at.reference(name, dtype, magnitude_start, sched)[0]
    gate = 1e-10
    if dtype == np.float32:
        own = rel_l2(ref, at.reference(name, dtype, magnitude_start, sched, np.float64)[0])
        gate = max(F32_FLOOR, 6 * own)
    e = rel_l2(y, ref)
    print(f"{name} {np.dtype(dtype).name} {sched}: forward rel_l2 {e:.3e} gate {gate:.3e}")
    assert y.shape == ref.shape and e <= gate, (e, gate)


F64 = ["128/32", "400/160", "64/16 two-sided normalized"]


@pytest.mark.parametrize("sched", list(at.SCHEDULES))
@pytest.mark.parametrize("magnitude_start", [False, True], ids=["complex", "magnitude"])
@pytest.mark.parametrize("name", F64)
def test_float64_gradients_match_autograd_on_the_restatement(name, magnitude_start, sched):
    """rel-L2 <= 1e-9 for grad spec and for each of the (n_iter,) vectors, tests/test_gpu_autograd.py's float64 gate."""
    clear_plan_cache()
    got = _device(name, np.float64, magnitude_start, sched)
    ref = at.reference(name, np.float64, magnitude_start, sched)
    for what, g, r in zip(("spec", "alpha", "beta", "gamma"), got[1:], ref[1:]):
        if not r.any():
            assert not g.any(), what
            continue
        e = rel_l2(g, r)
        print(f"{name} float64 {sched}: grad {what} {e:.3e}")
        assert e <= 1e-9, (what, e)


@pytest.mark.parametrize("sched", list(at.SCHEDULES))
@pytest.mark.parametrize("name,magnitude_start", at.FLOAT32_CASES)
def test_float32_gradients(route, name, magnitude_start, sched):
    """Against the float64 gradient of the restatement on the same float32 inputs.  The gate is the larger of 2e-4 (the float32
    gradient gate of tests/test_gpu_autograd.py) and 6 times the restatement's own float32-against-float64 gradient error on the
    case (the rule of DESIGN 3.13), which tests/test_agla_unfolded_host.py keeps at or below 1e-3."""
    route(name)
    got = _device(name, np.float32, magnitude_start, sched)
    r32 = at.reference(name, np.float32, magnitude_start, sched)
    r64 = at.reference(name, np.float32, magnitude_start, sched, np.float64)
    spec = at.inputs(name, np.float32, magnitude_start)[0]
    geo = get_plan(args_helper(T_(spec), **_tkw(at.inputs(name, np.float32, magnitude_start)[3])), 2, spec.shape[2], torch.float32,
                   DEV).launch_geometry
    if name != "64/16 two-sided normalized":
        assert geo["kernel"] == ("k_fused4" if name == "1024/256" else "k_wave_iter"), geo
        assert name != "1024/256" or geo["chunks"] == 2, geo
    for what, g, f, r in zip(("spec", "alpha", "beta", "gamma"), got[1:], r32[1:], r64[1:]):
        if not r.any():
            assert not g.any(), what
            continue
        own, e = rel_l2(f, r), rel_l2(g, r)
        print(f"{name} float32 {sched} ({geo['kernel']}): grad {what} {e:.3e} (restatement {own:.3e})")
        assert own <= 1e-3 and e <= max(2e-4, 6 * own), (what, e, own)


@pytest.mark.parametrize("wrt", ["spec", "alpha", "beta", "gamma"])
@pytest.mark.parametrize("magnitude_start", [False, True], ids=["complex", "magnitude"])
def test_gradient_matches_a_central_difference_of_the_inference_path(magnitude_start, wrt):
    """Independent of the restatement: float64, d/dt of sum(w * agla_unfolded(...)) without grad at h = 1e-6 against <grad,
    direction>, along a random unit direction in `spec` and along a unit direction in each parameter's schedule.  Relative 1e-6 (DESIGN
    3.13): the truncation is O(h^2), the rounding about 1e-10; a wrong formula is off by O(1)."""
    clear_plan_cache()
    spec, w, L, kw = at.inputs("128/32", np.float64, magnitude_start)
    got = _device("128/32", np.float64, magnitude_start, "general")
    rng = np.random.default_rng(11)
    k = ("spec", "alpha", "beta", "gamma").index(wrt)
    if wrt == "spec":
        d = rng.standard_normal(spec.shape) + (1j * rng.standard_normal(spec.shape) if np.iscomplexobj(spec) else 0)
    else:
        d = rng.standard_normal(N_ITER)
    d /= np.linalg.norm(d)
    ip = float((np.conj(got[1 + k]) * d).real.sum())
    h = 1e-6

    def f(t):
        par = [N(p) for p in _params("general", grad=False)]
        s = spec
        if wrt == "spec":
            s = spec + t * d
        else:
            par[k - 1] = par[k - 1] + t * d
        y = si.agla_unfolded(T_(s), N_ITER, *[torch.from_numpy(p) for p in par], **_tkw(kw))
        return float((N(y) * w).sum())

    fd = (f(h) - f(-h)) / (2 * h)
    print(f"d/d{wrt}: central difference {fd:.12e}  <grad, direction> {ip:.12e}  relative {abs(fd - ip) / abs(fd):.3e}")
    assert abs(fd - ip) <= 1e-6 * abs(fd), (fd, ip)


def _small_plan(hop, frames, dtype, batch, n_fft=16):
    kw = dict(hop_length=hop, window=torch.from_numpy(hann(n_fft, dtype)))
    cd = torch.complex64 if dtype == np.float32 else torch.complex128
    return Plan(args_helper(torch.empty((1, n_fft // 2 + 1, 1), dtype=cd), **kw), batch, frames, TDT[dtype], DEV)


# hop, frames, batch: L = (frames - 1) hop
EXTRAP = [(4, 4, 1),            # L = 12 = 0 (mod 4): 16-byte accesses; 12 samples, fewer than one workgroup
          (6, 4, 3),            # L = 18 = 2 (mod 4): 8-byte accesses (float64: 16)
          (5, 4, 3),            # L = 15, odd: 4-byte accesses (float64: 8)
          (8, 301, 5)]          # L = 2400, 12000 samples: 12 workgroups in float32, 24 in float64


def _extrap_case(p, dtype, n, general, rng):
    """One specinv_agla_extrap_adjoint call on random data against NumPy in float64.  Returns the measured errors over their
    bounds.  Element-wise: 8 eps (|a| + (1 + alpha)|gc| + (1 + beta)|gd|), for gc over the envelope and times gamma, for gd times
    |1 - gamma|; c_prev: 8 eps (|t_nm1| + alpha'|t_nm1 - t_nm2|).  Inner products: (8 eps + n 2^-53) sum |terms|, worst case - every
    product is formed in double from the stored values, s alone carries the element-wise rounding, the double sums add n 2^-53."""
    B, L = p.batch, p.length
    eps = np.finfo(dtype).eps
    draw = lambda: rng.standard_normal((B, L)).astype(dtype)             # noqa: E731
    a0, gc0, gd0, tn, tp, tpp = (draw() for _ in range(6))
    coef = (0.5, 1.2, 0.7, 0.45, 1.1) if general else (0.99, 0.3, 1.0, 0.9, 0.8)
    al, be, ga, alp, bep = (float(dtype(v)) for v in coef)
    omg = float(dtype(1.0 - coef[2]))
    a, gc, gd = T_(a0), T_(gc0), (T_(gd0) if general else None)
    c_prev = torch.full((B, L), float("nan"), dtype=TDT[dtype], device=DEV)
    dots = torch.full((3,), float("nan"), dtype=torch.float64, device=DEV)
    p.agla_extrap_adjoint(T_(tn), T_(tp), T_(tpp) if n > 2 else None, coef, a, gc, gd, c_prev, dots)
    env = N(p.envelope()).astype(np.float64)
    A, GC, TN, TP, TPP = (x.astype(np.float64) for x in (a0, gc0, tn, tp, tpp))
    GD = gd0.astype(np.float64) if general else np.zeros_like(A)
    size = np.abs(A) + (1 + al) * np.abs(GC) + (1 + be) * np.abs(GD)
    s = A + (1 + al) * GC + (1 + be) * GD
    cp = TP + alp * (TP - TPP) if n > 2 else TP
    dp = TP + bep * (TP - TPP) if n > 2 else TP
    delta = TN - TP
    ratios = [np.max(np.abs(N(a) - (-al * GC - be * GD)) / (8 * eps * size)),
              np.max(np.abs(N(gc) - ga * s / env) / (8 * eps * size * ga / env)),
              np.max(np.abs(N(c_prev) - cp) / (8 * eps * (np.abs(TP) + alp * np.abs(TP - TPP))))]
    if general:
        ratios.append(np.max(np.abs(N(gd) - omg * s) / (8 * eps * size * abs(omg))))
    for got, terms in zip(N(dots), (GC * delta, GD * delta, s * (TN - dp) / ga)):
        bound = (8 * eps + terms.size * 2.0 ** -53) * np.abs(terms).sum()
        if bound == 0:
            assert got == 0                                          # beta's, without gd: exactly zero
            continue
        ratios.append(abs(got - terms.sum()) / bound)
    return ratios


@pytest.mark.parametrize("general", [True, False], ids=["general", "fgla"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("hop,frames,batch", EXTRAP)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_every_arm_of_the_extrapolation_adjoint(dtype, hop, frames, batch, n, general):
    p = _small_plan(hop, frames, dtype, batch)
    assert p.length == (frames - 1) * hop
    ratios = _extrap_case(p, dtype, n, general, np.random.default_rng(hop + n))
    print(f"{np.dtype(dtype).name} L {p.length} B {batch} n {n} {'general' if general else 'fgla'}: error / bound {max(ratios):.3f}")
    assert max(ratios) <= 1, ratios


def test_extrapolation_adjoint_walks_beyond_one_grid():
    """3 x 1048576 float32 samples: more than the 2048 x 256 x 4 one pass of the grid covers."""
    p = _small_plan(256, 4097, np.float32, 3, n_fft=1024)
    assert p.batch * p.length > 2048 * 256 * 4
    ratios = _extrap_case(p, np.float32, 3, True, np.random.default_rng(1))
    print(f"L {p.length} B 3: error / bound {max(ratios):.3f}")
    assert max(ratios) <= 1, ratios


def _layer_case():
    spec, w, L, kw = at.inputs("128/32", np.float32, True)
    return spec, w, _tkw(kw)


def test_backward_twice_gives_identical_gradients():
    spec, w, kw = _layer_case()
    s, par = T_(spec).requires_grad_(True), _params("general")
    loss = (si.agla_unfolded(s, N_ITER, *par, **kw) * T_(w)).sum()
    first = torch.autograd.grad(loss, (s, *par), retain_graph=True)
    second = torch.autograd.grad(loss, (s, *par))
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    assert all(torch.isfinite(a).all() and a.abs().max() > 0 for a in first)


def test_a_backward_leaves_the_cached_plan_as_it_was():
    clear_plan_cache()
    spec, w, kw = _layer_case()
    tk = dict(max_iter=5, tol=0, verbose=False, **kw)

    def neighbours():
        return si.griffin_lim(T_(spec), alpha=0.3, **tk), si.accelerated_griffin_lim(T_(spec), alpha=0.5, beta=1.2, gamma=0.7, **tk)

    before = neighbours()
    s, par = T_(spec).requires_grad_(True), _params("general")
    y = si.agla_unfolded(s, N_ITER, *par, **kw)
    running = neighbours()                                            # the same plan, between forward and backward
    (y * T_(w)).sum().backward()
    after = neighbours()
    assert all(torch.equal(b, r) and torch.equal(b, a) for b, r, a in zip(before, running, after))
    g = s.grad.clone()
    s.grad = None
    (si.agla_unfolded(s, N_ITER, *par, **kw) * T_(w)).sum().backward()
    assert torch.equal(g, s.grad)


def test_parameters_get_gradients_of_their_own_kind():
    spec, w, kw = _layer_case()
    al64, be64, ga64 = _params("general")
    (si.agla_unfolded(T_(spec), N_ITER, al64, be64, ga64, **kw) * T_(w)).sum().backward()
    # float32 on the CPU, float64 on the device, a 0-d tensor: each gets its own dtype, device and shape back
    al = al64.detach().float().requires_grad_(True)
    be = be64.detach().to(DEV).requires_grad_(True)
    ga = torch.tensor(0.7, requires_grad=True)
    y = si.agla_unfolded(T_(spec), N_ITER, al, be, ga, **kw)
    assert y.requires_grad
    (y * T_(w)).sum().backward()
    assert al.grad.dtype == torch.float32 and al.grad.device.type == "cpu" and al.grad.shape == (N_ITER,)
    assert be.grad.dtype == torch.float64 and be.grad.device == DEV and be.grad.shape == (N_ITER,)
    assert ga.grad.dtype == torch.float32 and ga.grad.shape == () and torch.isfinite(ga.grad) and ga.grad != 0
    # beta = None is alpha: its gradient flows into alpha
    a2, b2, g2 = _params("general")
    with torch.no_grad():
        b2.copy_(a2)
    (si.agla_unfolded(T_(spec), N_ITER, a2, b2, g2, **kw) * T_(w)).sum().backward()
    a1, _, g1 = _params("general")
    (si.agla_unfolded(T_(spec), N_ITER, a1, None, g1, **kw) * T_(w)).sum().backward()
    assert torch.equal(a1.grad, a2.grad + b2.grad) and torch.equal(g1.grad, g2.grad)
    # CPU and narrow spectrograms
    s = torch.from_numpy(spec).requires_grad_(True)
    yc = si.agla_unfolded(s, N_ITER, *_params("general", grad=False), **kw)
    assert yc.device.type == "cpu" and yc.shape == w.shape
    (yc * torch.from_numpy(w)).sum().backward()
    assert s.grad.device.type == "cpu" and torch.isfinite(s.grad).all() and s.grad.abs().max() > 0
    s1 = torch.from_numpy(spec[0]).requires_grad_(True)
    assert si.agla_unfolded(s1, N_ITER, **kw).shape == w.shape[1:]
    hs = T_(spec).to(torch.bfloat16).requires_grad_(True)
    hy = si.agla_unfolded(hs, N_ITER, **kw)
    assert hy.dtype == torch.bfloat16
    hy.float().sum().backward()
    assert hs.grad.dtype == torch.bfloat16 and torch.isfinite(hs.grad.float()).all()
