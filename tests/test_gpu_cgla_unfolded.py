"""`constrained_unfolded` on the device: its forward against `constrained_griffin_lim` and `agla_unfolded` (bits) and the torch
restatement of the constrained oracle (tests/_cgla_torch.py), its gradients against autograd on that restatement, against central
differences of the inference path and against the same iteration composed from `gla_projection`, `stft`, `istft` and torch ops,
`specinv_cgla_extrap_adjoint` (csrc/kernels_agla_adjoint.h) alone against NumPy, and the layer's properties.  Needs an MI355X:
`-m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch

import _cgla_torch as ct
from _agla_torch import schedule
from _util import hann, rel_l2

pytestmark = pytest.mark.gpu

import spectrogram_inversion_amd as si                                    # noqa: E402
from spectrogram_inversion_amd import _lib                                 # noqa: E402
from spectrogram_inversion_amd.plan import Plan, args_helper, clear_plan_cache, get_plan   # noqa: E402

DEV = torch.device("cuda", 0)
N_ITER = ct.N_ITER
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


def nz(t):
    """some element is not zero (complex tensors included)"""
    return bool(t.abs().max() > 0)


def _tkw(kw):
    return dict(kw, window=torch.from_numpy(kw["window"]))


def _params(sched, grad=True, device="cpu"):
    """alpha, beta, gamma as (N_ITER,) float64 tensors (beta spelled out where the schedule says None: its gradient is compared)"""
    al, be, ga = ct.SCHEDULES[sched]
    return [schedule(v, N_ITER).clone().to(device).requires_grad_(grad) for v in (al, al if be is None else be, ga)]


def _con(c, which, grad=False, dev=DEV):
    """The constraint of a case as tensors on `dev`, the values requiring grad if asked"""
    con = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in ct.constraint(c, which).items()}
    if grad:
        for k in ("known_spec", "known_wave"):
            if k in con:
                con[k].requires_grad_(True)
    return con


def _routed(c, name, dtype):
    """The kernel the case's projection takes, asserted where the case names one"""
    spec = c["spec"]
    geo = get_plan(args_helper(T_(spec), **_tkw(c["kw"])), 2, spec.shape[2], TDT[dtype], DEV).launch_geometry
    if dtype == np.float32 and name != "64/16 two-sided normalized":
        assert geo["kernel"] == ("k_fused4" if name == "1024/256" else "k_wave_iter"), geo
        assert name != "1024/256" or geo["chunks"] == 2, geo
    return geo


def _device(name, dtype, magnitude_start, sched, which):
    """(y, then the gradients in the order of ct.GRADS, None for an absent input) of sum(w * constrained_unfolded(...)) on the
    device, as NumPy arrays.  Asserts on the way what holds exactly: the output under grad is the inference path's, the gradients'
    shapes and dtypes, their zeros."""
    c = ct.inputs(name, dtype, magnitude_start)
    s, par, con = T_(c["spec"]).requires_grad_(True), _params(sched), _con(c, which, grad=True)
    kw = _tkw(c["kw"])
    y = si.constrained_unfolded(s, **con, n_iter=N_ITER, alpha=par[0], beta=par[1], gamma=par[2], **kw)
    assert y.requires_grad and y.shape == c["w"].shape
    with torch.no_grad():
        assert torch.equal(y, si.constrained_unfolded(s, **con, n_iter=N_ITER, alpha=par[0], beta=par[1], gamma=par[2], **kw))
    (y * T_(c["w"])).sum().backward()
    assert s.grad.shape == s.shape and s.grad.dtype == s.dtype
    for p in par:
        assert p.grad.shape == (N_ITER,) and p.grad.dtype == torch.float64 and p.grad.device.type == "cpu"
        assert p.grad[0] == 0                                        # iteration 1 does not extrapolate
    if sched == "fgla":
        assert not par[1].grad.any()                                 # every gamma = 1: beta has no effect, exactly
    if "known_spec" in con:
        K, M = con["known_spec"], con["spec_mask"]
        assert K.grad.shape == K.shape and K.grad.dtype == K.dtype
        assert not nz(s.grad[M]) and not nz(K.grad[~M]) and nz(K.grad[M])
    if "known_wave" in con:
        xk, W = con["known_wave"], con["wave_mask"]
        assert xk.grad.shape == xk.shape and xk.grad.dtype == xk.dtype
        assert not nz(xk.grad[~W]) and nz(xk.grad[W])
    g = lambda k: N(con[k].grad) if k in con else None               # noqa: E731
    return (N(y), N(s.grad), g("known_spec"), g("known_wave")) + tuple(N(p.grad) for p in par)


FORWARD = [(n, m, d) for n, m in ct.FLOAT32_CASES for d in (np.float32, np.float64) if not (d == np.float64 and n == "1024/256")]


@pytest.mark.parametrize("which", ct.CONSTRAINTS)
@pytest.mark.parametrize("name,magnitude_start,dtype", FORWARD + [("400/160", True, np.float64), ("1024/256", True, np.float32)])
def test_constant_parameters_are_constrained_griffin_lim(route, name, magnitude_start, dtype, which):
    """No gradient and constant parameters: the bits of constrained_griffin_lim(max_iter=n_iter, tol=0), floats or tensors; under
    grad the same bits again."""
    route(name)
    key = (name, magnitude_start) if (name, magnitude_start) in ct.SEEDS else (name, False)
    c = ct.inputs(name, dtype, key[1])
    spec = np.abs(c["spec"]) if magnitude_start and np.iscomplexobj(c["spec"]) else c["spec"]
    con, kw = _con(c, which), _tkw(c["kw"])
    for al, be, ga in ((0.99, None, 1.0), (0.5, 1.2, 0.7)):
        ref = si.constrained_griffin_lim(T_(spec), **con, max_iter=N_ITER, tol=0, verbose=False, alpha=al, beta=be, gamma=ga, **kw)
        y = si.constrained_unfolded(T_(spec), **con, n_iter=N_ITER, alpha=al, beta=be, gamma=ga, **kw)
        assert not y.requires_grad and torch.equal(y, ref)
        as_tensors = [None if v is None else torch.full((N_ITER,), v, dtype=torch.float64) for v in (al, be, ga)]
        assert torch.equal(si.constrained_unfolded(T_(spec), **con, n_iter=N_ITER, alpha=as_tensors[0], beta=as_tensors[1],
                                                   gamma=as_tensors[2], **kw), ref)
        yg = si.constrained_unfolded(T_(spec).requires_grad_(True), **_con(c, which, grad=True), n_iter=N_ITER, alpha=al, beta=be,
                                     gamma=torch.tensor(ga, dtype=torch.float64, requires_grad=True), **kw)
        assert yg.requires_grad and torch.equal(yg.detach(), ref)
    _routed(c, name, dtype)


@pytest.mark.parametrize("sched", list(ct.SCHEDULES))
@pytest.mark.parametrize("name,magnitude_start", [("128/32", False), ("128/32", True), ("1024/256", False)])
def test_without_a_constraint_it_is_agla_unfolded(route, name, magnitude_start, sched):
    route(name)
    c = ct.inputs(name, np.float32, magnitude_start)
    kw = _tkw(c["kw"])
    par = _params(sched, grad=False)
    ref = si.agla_unfolded(T_(c["spec"]), N_ITER, *par, **kw)
    assert torch.equal(si.constrained_unfolded(T_(c["spec"]), n_iter=N_ITER, alpha=par[0], beta=par[1], gamma=par[2], **kw), ref)
    s, g = T_(c["spec"]).requires_grad_(True), T_(c["spec"]).requires_grad_(True)
    y = si.constrained_unfolded(s, n_iter=N_ITER, alpha=par[0], beta=par[1], gamma=par[2], **kw)
    assert y.requires_grad and torch.equal(y.detach(), ref)
    (y * T_(c["w"])).sum().backward()
    (si.agla_unfolded(g, N_ITER, *par, **kw) * T_(c["w"])).sum().backward()
    assert torch.equal(s.grad, g.grad)


@pytest.mark.parametrize("sched", list(ct.SCHEDULES))
@pytest.mark.parametrize("which", ct.CONSTRAINTS)
@pytest.mark.parametrize("name,magnitude_start,dtype", FORWARD + [("400/160", True, np.float64)])
def test_forward_matches_the_restatement(route, name, magnitude_start, dtype, which, sched):
    """A real schedule without a gradient.  float64: 1e-10.  float32: the larger of 2e-5 and 6 x the restatement's own
    float32-against-float64 rel-L2 on the case, the rule of tests/test_gpu_agla.py."""
    route(name)
    c = ct.inputs(name, dtype, magnitude_start)
    par = _params(sched, grad=False)
    y = N(si.constrained_unfolded(T_(c["spec"]), **_con(c, which), n_iter=N_ITER, alpha=par[0], beta=par[1], gamma=par[2],
                                  **_tkw(c["kw"])))
    ref = ct.reference(name, dtype, magnitude_start, sched, which)[0]
    gate = 1e-10
    if dtype == np.float32:
        own = rel_l2(ref, ct.reference(name, dtype, magnitude_start, sched, which, np.float64)[0])
        gate = max(F32_FLOOR, 6 * own)
    e = rel_l2(y, ref)
    print(f"{name} {np.dtype(dtype).name} {which} {sched}: forward rel_l2 {e:.3e} gate {gate:.3e}")
    assert y.shape == ref.shape and e <= gate, (e, gate)
    if which != "spec":                                              # the known samples, bit for bit
        assert np.array_equal(y[c["wave_mask"]], c["known_wave"][c["wave_mask"]])


F64 = ["128/32", "400/160", "64/16 two-sided normalized"]


@pytest.mark.parametrize("sched", list(ct.SCHEDULES))
@pytest.mark.parametrize("which", ct.CONSTRAINTS)
@pytest.mark.parametrize("magnitude_start", [False, True], ids=["complex", "magnitude"])
@pytest.mark.parametrize("name", F64)
def test_float64_gradients_match_autograd_on_the_restatement(name, magnitude_start, which, sched):
    """rel-L2 <= 1e-9 for each of spec, known_spec, known_wave and the (n_iter,) vectors, tests/test_gpu_autograd.py's float64
    gate."""
    clear_plan_cache()
    got = _device(name, np.float64, magnitude_start, sched, which)
    ref = ct.reference(name, np.float64, magnitude_start, sched, which)
    for what, g, r in zip(ct.GRADS, got[1:], ref[1:]):
        if r is None:
            assert g is None, what
            continue
        if not r.any():
            assert not g.any(), what
            continue
        e = rel_l2(g, r)
        print(f"{name} float64 {which} {sched}: grad {what} {e:.3e}")
        assert e <= 1e-9, (what, e)


@pytest.mark.parametrize("sched", list(ct.SCHEDULES))
@pytest.mark.parametrize("which", ct.CONSTRAINTS)
@pytest.mark.parametrize("name,magnitude_start", ct.FLOAT32_CASES)
def test_float32_gradients(route, name, magnitude_start, which, sched):
    """Against the float64 gradient of the restatement on the same float32 inputs.  The gate is the larger of 2e-4 (the float32
    gradient gate of tests/test_gpu_autograd.py) and 6 times the restatement's own float32-against-float64 gradient error on the
    case, which tests/test_cgla_unfolded_host.py keeps at or below 1e-3."""
    route(name)
    got = _device(name, np.float32, magnitude_start, sched, which)
    r32 = ct.reference(name, np.float32, magnitude_start, sched, which)
    r64 = ct.reference(name, np.float32, magnitude_start, sched, which, np.float64)
    geo = _routed(ct.inputs(name, np.float32, magnitude_start), name, np.float32)
    for what, g, f, r in zip(ct.GRADS, got[1:], r32[1:], r64[1:]):
        if r is None:
            assert g is None, what
            continue
        if not r.any():
            assert not g.any(), what
            continue
        own, e = rel_l2(f, r), rel_l2(g, r)
        print(f"{name} float32 {which} {sched} ({geo['kernel']}): grad {what} {e:.3e} (restatement {own:.3e})")
        assert own <= 1e-3 and e <= max(2e-4, 6 * own), (what, e, own)


@pytest.mark.parametrize("wrt", ct.GRADS)
@pytest.mark.parametrize("magnitude_start", [False, True], ids=["complex", "magnitude"])
def test_gradient_matches_a_central_difference_of_the_inference_path(magnitude_start, wrt):
    """Independent of the restatement: float64, 128/32, both constraints, d/dt of sum(w * constrained_unfolded(...)) without grad at
    h = 1e-6 against <grad, direction>, along a random unit direction in each of the six inputs.  Relative 1e-6: the truncation is
    O(h^2), the rounding about 1e-10; a wrong formula is off by O(1).  Measured: <= 7.8e-8, but 9.3e-7 along `spec` from
    magnitudes, where the directional derivative is 9.4e-3 and the rounding of the difference itself shows - the CPU restatement's
    autograd sits at 9.0e-7 of its own central difference along the same direction (tests/test_cgla_unfolded_host.py)."""
    clear_plan_cache()
    c = ct.inputs("128/32", np.float64, magnitude_start)
    got = _device("128/32", np.float64, magnitude_start, "general", "both")
    k = ct.GRADS.index(wrt)
    base = dict(spec=c["spec"], known_spec=c["known_spec"], known_wave=c["known_wave"],
                **dict(zip(("alpha", "beta", "gamma"), (N(p) for p in _params("general", grad=False)))))
    rng = np.random.default_rng(11)
    d = rng.standard_normal(base[wrt].shape) + (1j * rng.standard_normal(base[wrt].shape) if np.iscomplexobj(base[wrt]) else 0)
    d /= np.linalg.norm(d)
    ip = float((np.conj(got[1 + k]) * d).real.sum())
    h = 1e-6

    def f(t):
        v = dict(base)
        v[wrt] = base[wrt] + t * d
        with torch.no_grad():
            y = si.constrained_unfolded(T_(v["spec"]), T_(v["known_spec"]), T_(c["spec_mask"]), T_(v["known_wave"]), T_(c["wave_mask"]),
                                        n_iter=N_ITER, alpha=torch.from_numpy(v["alpha"]), beta=torch.from_numpy(v["beta"]),
                                        gamma=torch.from_numpy(v["gamma"]), **_tkw(c["kw"]))
        return float((N(y) * c["w"]).sum())

    fd = (f(h) - f(-h)) / (2 * h)
    print(f"d/d{wrt}: central difference {fd:.12e}  <grad, direction> {ip:.12e}  relative {abs(fd - ip) / abs(fd):.3e}")
    assert abs(fd - ip) <= 1e-6 * abs(fd), (fd, ip)


def _composed(s, K, M, xk, W, par, kw):
    """The same iteration from the library's layers and torch ops, a complex start"""
    m_free = torch.where(M, torch.zeros_like(s.real), s.abs())
    c = si.istft(torch.where(M, K, s), **kw)
    k = si.istft(torch.where(M, K, torch.zeros_like(K)), **kw)
    al, be, ga = (p.to(DEV) for p in par)
    t = d = None
    for n in range(1, N_ITER + 1):
        u = si.gla_projection(c, m_free, **kw) + k
        if n == 1:
            t = c = d = torch.where(W, xk, u)
        else:
            tn = torch.where(W, xk, (1.0 - ga[n - 1]) * d + ga[n - 1] * u)
            c = tn + al[n - 1] * (tn - t)
            d = tn + be[n - 1] * (tn - t)
            t = tn
    return t


@pytest.mark.parametrize("sched", list(ct.SCHEDULES))
@pytest.mark.parametrize("name", ["128/32", "400/160"])
def test_layer_matches_the_iteration_composed_from_the_library_layers(name, sched):
    """Independent of the restatement and of the sweep: float64, a complex start, both constraints; the output and the six
    gradients against `gla_projection` / `istft` and torch ops under autograd on the device, rel-L2 <= 1e-9."""
    clear_plan_cache()
    c = ct.inputs(name, np.float64, False)
    kw = _tkw(c["kw"])
    out = []
    for layer in (True, False):
        s, par, con = T_(c["spec"]).requires_grad_(True), _params(sched), _con(c, "both", grad=True)
        if layer:
            y = si.constrained_unfolded(s, **con, n_iter=N_ITER, alpha=par[0], beta=par[1], gamma=par[2], **kw)
        else:
            y = _composed(s, con["known_spec"], con["spec_mask"], con["known_wave"], con["wave_mask"], par, kw)
        (y * T_(c["w"])).sum().backward()
        out.append([N(y), N(s.grad), N(con["known_spec"].grad), N(con["known_wave"].grad)] + [N(p.grad) for p in par])
    for what, g, r in zip(("y",) + ct.GRADS, *out):
        if not r.any():
            assert not g.any(), what
            continue
        e = rel_l2(g, r)
        print(f"{name} {sched}: {what} layer vs composed {e:.3e}")
        assert e <= 1e-9, (what, e)


def _small_plan(hop, frames, dtype, batch, n_fft=16):
    kw = dict(hop_length=hop, window=torch.from_numpy(hann(n_fft, dtype)))
    cd = torch.complex64 if dtype == np.float32 else torch.complex128
    return Plan(args_helper(torch.empty((1, n_fft // 2 + 1, 1), dtype=cd), **kw), batch, frames, TDT[dtype], DEV)


# hop, frames, batch: L = (frames - 1) hop
EXTRAP = [(4, 4, 1),            # L = 12 = 0 (mod 4): 16-byte accesses; 12 samples, fewer than one workgroup
          (6, 4, 3),            # L = 18 = 2 (mod 4): 8-byte accesses (float64: 16)
          (5, 4, 3),            # L = 15, odd: 4-byte accesses (float64: 8)
          (8, 301, 5)]          # L = 2400, 12000 samples: 12 workgroups in float32, 24 in float64


def _odd_mask(B, L):
    """Known samples whose edges fall at odd indices, inside a thread's vector, shifted from item to item"""
    W = np.zeros((B, L), bool)
    for b in range(B):
        W[b, : (L // 3 | 1) + 2 * (b % 2)] = True
        lo = (L // 2 | 1)
        W[b, lo: lo + 3 + 2 * b] = True
    return W


def _extrap_case(p, dtype, n, general, masked, rng, first=False):
    """One specinv_cgla_extrap_adjoint call (`first`: specinv_cgla_first_adjoint's element-wise arm is reached through the step
    with zero magnitudes - see test_the_closing_arm) on random data against NumPy in float64.  Returns the measured errors over their
    bounds, those of tests/test_gpu_agla_unfolded.py.  Element-wise: 8 eps (|a| + (1 + alpha)|gc| + (1 + beta)|gd|), for gc over the
    envelope and times gamma, for gd times |1 - gamma|; c_prev: 8 eps (|t_nm1| + alpha'|t_nm1 - t_nm2|); goff: 8 eps (|goff_0| +
    that size).  Inner products: (8 eps + n 2^-53) sum |terms|."""
    B, L = p.batch, p.length
    eps = np.finfo(dtype).eps
    draw = lambda: rng.standard_normal((B, L)).astype(dtype)             # noqa: E731
    a0, gc0, gd0, tn, tp, tpp, go0 = (draw() for _ in range(7))
    W = _odd_mask(B, L) if masked else np.zeros((B, L), bool)
    coef = (0.5, 1.2, 0.7, 0.45, 1.1) if general else (0.99, 0.3, 1.0, 0.9, 0.8)
    al, be, ga, alp, bep = (float(dtype(v)) for v in coef)
    omg = float(dtype(1.0 - coef[2]))
    a, gc, gd, goff = T_(a0), T_(gc0), (T_(gd0) if general else None), T_(go0)
    c_prev = torch.full((B, L), float("nan"), dtype=TDT[dtype], device=DEV)
    dots = torch.full((3,), float("nan"), dtype=torch.float64, device=DEV)
    p.cgla_extrap_adjoint(T_(tn), T_(tp), T_(tpp) if n > 2 else None, coef, T_(W) if masked else None, a, gc, gd, goff, c_prev, dots)
    env = N(p.envelope()).astype(np.float64)
    A, GC, TN, TP, TPP, GO = (x.astype(np.float64) for x in (a0, gc0, tn, tp, tpp, go0))
    GD = gd0.astype(np.float64) if general else np.zeros_like(A)
    size = np.abs(A) + (1 + al) * np.abs(GC) + (1 + be) * np.abs(GD)
    s = A + (1 + al) * GC + (1 + be) * GD
    sp = np.where(W, 0.0, s)
    cp = TP + alp * (TP - TPP) if n > 2 else TP
    dp = TP + bep * (TP - TPP) if n > 2 else TP
    delta = TN - TP
    assert not (N(gc)[W] != 0).any() and (not general or not (N(gd)[W] != 0).any())      # nothing passes the select: exact zeros
    ratios = [np.max(np.abs(N(a) - (-al * GC - be * GD)) / (8 * eps * size)),
              np.max(np.abs(N(gc) - ga * sp / env) / (8 * eps * size * ga / env)),
              np.max(np.abs(N(c_prev) - cp) / (8 * eps * (np.abs(TP) + alp * np.abs(TP - TPP)))),
              np.max(np.abs(N(goff) - (GO + np.where(W, s, ga * sp))) / (8 * eps * (np.abs(GO) + size)))]
    if general:
        ratios.append(np.max(np.abs(N(gd) - omg * sp) / (8 * eps * size * abs(omg))))
    for got, terms in zip(N(dots), (GC * delta, GD * delta, sp * (TN - dp) / ga)):
        bound = (8 * eps + terms.size * 2.0 ** -53) * np.abs(terms).sum()
        if bound == 0:
            assert got == 0                                          # beta's, without gd: exactly zero
            continue
        ratios.append(abs(got - terms.sum()) / bound)
    return ratios


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "null-mask"])
@pytest.mark.parametrize("general", [True, False], ids=["general", "fgla"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("hop,frames,batch", EXTRAP)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_every_arm_of_the_extrapolation_adjoint(dtype, hop, frames, batch, n, general, masked):
    p = _small_plan(hop, frames, dtype, batch)
    assert p.length == (frames - 1) * hop
    ratios = _extrap_case(p, dtype, n, general, masked, np.random.default_rng(hop + n))
    print(f"{np.dtype(dtype).name} L {p.length} B {batch} n {n} {'general' if general else 'fgla'} "
          f"{'mask' if masked else 'null mask'}: error / bound {max(ratios):.3f}")
    assert max(ratios) <= 1, ratios


@pytest.mark.parametrize("masked", [True, False], ids=["mask", "null-mask"])
@pytest.mark.parametrize("general", [True, False], ids=["general", "fgla"])
@pytest.mark.parametrize("hop,frames,batch", EXTRAP)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_closing_arm(dtype, hop, frames, batch, general, masked):
    """specinv_cgla_first_adjoint: what the element-wise arm wrote shows in goff, goff_0 + a + gc + gd to 8 eps of the sizes, under
    the mask and off it; a and gd are left as they were.  (gc goes on through the projection's adjoint: the next test.)"""
    p = _small_plan(hop, frames, dtype, batch)
    B, L = p.batch, p.length
    eps = np.finfo(dtype).eps
    rng = np.random.default_rng(hop)
    a0, gc0, gd0, go0, c0 = (rng.standard_normal((B, L)).astype(dtype) for _ in range(5))
    W = _odd_mask(B, L) if masked else None
    a, gc, gd, goff = T_(a0), T_(gc0), (T_(gd0) if general else None), T_(go0)
    fm = (B, p.n_frames, p.n_freq)
    gm = torch.zeros(fm, dtype=TDT[dtype], device=DEV)
    p.cgla_first_adjoint(T_(c0), None if W is None else T_(W), a, gc, gd, goff, T_((rng.random(fm) + 0.05).astype(dtype)), gm)
    s = a0.astype(np.float64) + gc0 + (gd0 if general else 0)
    size = np.abs(a0).astype(np.float64) + np.abs(gc0) + (np.abs(gd0) if general else 0)
    r = np.max(np.abs(N(goff) - (go0 + s)) / (8 * eps * (np.abs(go0) + size)))
    print(f"{np.dtype(dtype).name} L {L} B {B}: goff error / bound {r:.3f}")
    assert r <= 1
    assert np.array_equal(N(a), a0) and (not general or np.array_equal(N(gd), gd0))
    assert np.isfinite(N(gc)).all() and np.isfinite(N(gm)).all()


def test_the_closing_arm_feeds_the_projection_adjoint():
    """With magnitudes: gc after specinv_cgla_first_adjoint is the projection's adjoint of (W ? 0 : a + gc + gd), which
    `Plan.project_adjoint` computes from the same cotangent."""
    p = _small_plan(8, 301, np.float64, 2)
    B, L = p.batch, p.length
    rng = np.random.default_rng(5)
    a0, gc0, gd0, c0 = (rng.standard_normal((B, L)) for _ in range(4))
    W = _odd_mask(B, L)
    fm = (B, p.n_frames, p.n_freq)
    mag_fm = T_(rng.random(fm) + 0.05)
    a, gc, gd, goff = T_(a0), T_(gc0), T_(gd0), torch.zeros((B, L), dtype=torch.float64, device=DEV)
    gm = torch.zeros(fm, dtype=torch.float64, device=DEV)
    p.cgla_first_adjoint(T_(c0), T_(W), a, gc, gd, goff, mag_fm, gm)
    g_x, g_m = p.project_adjoint(T_(c0), mag_fm, T_(np.where(W, 0.0, a0 + gc0 + gd0)))
    assert rel_l2(N(gc), N(g_x)) <= 1e-12 and rel_l2(N(gm), N(g_m)) <= 1e-12
    assert rel_l2(N(goff), a0 + gc0 + gd0) <= 1e-15


def test_extrapolation_adjoint_walks_beyond_one_grid():
    """3 x 1048576 float32 samples: more than the 2048 x 256 x 4 one pass of the grid covers."""
    p = _small_plan(256, 4097, np.float32, 3, n_fft=1024)
    assert p.batch * p.length > 2048 * 256 * 4
    ratios = _extrap_case(p, np.float32, 3, True, True, np.random.default_rng(1))
    print(f"L {p.length} B 3: error / bound {max(ratios):.3f}")
    assert max(ratios) <= 1, ratios


def _layer_case():
    c = ct.inputs("128/32", np.float32, True)
    return c, _tkw(c["kw"])


def _loss(c, kw, s, par, con):
    return (si.constrained_unfolded(s, **con, n_iter=N_ITER, alpha=par[0], beta=par[1], gamma=par[2], **kw) * T_(c["w"])).sum()


def test_backward_twice_gives_identical_gradients():
    c, kw = _layer_case()
    s, par, con = T_(c["spec"]).requires_grad_(True), _params("general"), _con(c, "both", grad=True)
    wrt = (s, con["known_spec"], con["known_wave"], *par)
    loss = _loss(c, kw, s, par, con)
    first = torch.autograd.grad(loss, wrt, retain_graph=True)
    second = torch.autograd.grad(loss, wrt)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    assert all(torch.isfinite(torch.view_as_real(a) if a.is_complex() else a).all() and a.abs().max() > 0 for a in first)


def test_a_backward_leaves_the_cached_plan_as_it_was():
    clear_plan_cache()
    c, kw = _layer_case()
    tk = dict(max_iter=5, tol=0, verbose=False, **kw)
    spec = c["spec"]

    def neighbours():
        return (si.griffin_lim(T_(spec), alpha=0.3, **tk), si.accelerated_griffin_lim(T_(spec), alpha=0.5, beta=1.2, gamma=0.7, **tk),
                si.constrained_griffin_lim(T_(spec), **_con(c, "both"), alpha=0.5, beta=1.2, gamma=0.7, **tk))

    before = neighbours()
    s, par, con = T_(spec).requires_grad_(True), _params("general"), _con(c, "both", grad=True)
    loss = _loss(c, kw, s, par, con)
    running = neighbours()                                            # the same plan, between forward and backward
    loss.backward()
    after = neighbours()
    assert all(torch.equal(b, r) and torch.equal(b, a) for b, r, a in zip(before, running, after))
    g = s.grad.clone()
    s.grad = None
    _loss(c, kw, s, par, con).backward()
    assert torch.equal(g, s.grad)


def test_parameters_and_inputs_get_gradients_of_their_own_kind():
    c, kw = _layer_case()
    spec, w = c["spec"], c["w"]
    al64, be64, ga64 = _params("general")
    # float32 on the CPU, float64 on the device, a 0-d tensor: each gets its own dtype, device and shape back
    al = al64.detach().float().requires_grad_(True)
    be = be64.detach().to(DEV).requires_grad_(True)
    ga = torch.tensor(0.7, requires_grad=True)
    y = si.constrained_unfolded(T_(spec), **_con(c, "both"), n_iter=N_ITER, alpha=al, beta=be, gamma=ga, **kw)
    assert y.requires_grad
    (y * T_(w)).sum().backward()
    assert al.grad.dtype == torch.float32 and al.grad.device.type == "cpu" and al.grad.shape == (N_ITER,)
    assert be.grad.dtype == torch.float64 and be.grad.device == DEV and be.grad.shape == (N_ITER,)
    assert ga.grad.dtype == torch.float32 and ga.grad.shape == () and torch.isfinite(ga.grad) and ga.grad != 0
    # beta = None is alpha: its gradient flows into alpha
    a2, b2, g2 = _params("general")
    with torch.no_grad():
        b2.copy_(a2)
    _loss(c, kw, T_(spec), (a2, b2, g2), _con(c, "both")).backward()
    a1, _, g1 = _params("general")
    _loss(c, kw, T_(spec), (a1, None, g1), _con(c, "both")).backward()
    assert torch.equal(a1.grad, a2.grad + b2.grad) and torch.equal(g1.grad, g2.grad)
    # a known_wave alone requiring grad engages the layer; a broadcast mask
    xk = T_(c["known_wave"]).requires_grad_(True)
    y = si.constrained_unfolded(T_(spec), known_wave=xk, wave_mask=T_(c["wave_mask"][0]), n_iter=N_ITER, **kw)
    assert y.requires_grad
    y.sum().backward()
    assert not nz(xk.grad[:, ~T_(c["wave_mask"][0])]) and nz(xk.grad)
    # CPU inputs come back on the CPU
    s = torch.from_numpy(spec).requires_grad_(True)
    con = _con(c, "both", grad=True, dev="cpu")
    yc = si.constrained_unfolded(s, **con, n_iter=N_ITER, **kw)
    assert yc.device.type == "cpu" and yc.shape == w.shape
    (yc * torch.from_numpy(w)).sum().backward()
    for t in (s, con["known_spec"], con["known_wave"]):
        assert t.grad.device.type == "cpu" and t.grad.shape == t.shape and t.grad.abs().max() > 0
        assert torch.isfinite(torch.view_as_real(t.grad) if t.grad.is_complex() else t.grad).all()
    # (F, T) input
    s1 = torch.from_numpy(spec[0]).requires_grad_(True)
    one = {k: v[0] for k, v in _con(c, "both").items()}
    y1 = si.constrained_unfolded(s1, **one, n_iter=N_ITER, **kw)
    assert y1.shape == w.shape[1:] and y1.requires_grad
    y1.sum().backward()
    assert s1.grad.shape == s1.shape
    # bfloat16 round trip
    hs = T_(spec).to(torch.bfloat16).requires_grad_(True)
    hx = T_(c["known_wave"]).to(torch.bfloat16).requires_grad_(True)
    hy = si.constrained_unfolded(hs, known_wave=hx, wave_mask=T_(c["wave_mask"]), n_iter=N_ITER, **kw)
    assert hy.dtype == torch.bfloat16
    hy.float().sum().backward()
    assert hs.grad.dtype == torch.bfloat16 and torch.isfinite(hs.grad.float()).all()
    assert hx.grad.dtype == torch.bfloat16 and torch.isfinite(hx.grad.float()).all()
    # constrained_griffin_lim itself stays as it is
    with pytest.raises(NotImplementedError, match="not differentiable"):
        si.constrained_griffin_lim(T_(spec).requires_grad_(True), **_con(c, "both"), max_iter=2, **kw)


def test_argument_errors_of_the_c_entries_enqueue_nothing():
    """SPECINV_EINVAL on a live plan, its buffers as they were: the outputs keep their NaN."""
    p = _small_plan(8, 301, np.float32, 2)
    lib, h = p.lib, p._h
    B, L = p.batch, p.length
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)     # noqa: E731
    t = [torch.zeros((B, L), dtype=torch.float32, device=DEV) for _ in range(3)]
    a, gc, gd, goff, c_prev = (nan(B, L) for _ in range(5))
    dots = torch.full((3,), float("nan"), dtype=torch.float64, device=DEV)
    fm = (B, p.n_frames, p.n_freq)
    mag_fm, gm = torch.zeros(fm, dtype=torch.float32, device=DEV), nan(*fm)
    W = torch.zeros((B, L), dtype=torch.uint8, device=DEV)
    coef = (C.c_double * 5)(0.5, 1.2, 0.7, 0.4, 1.1)
    ptr = lambda x: C.c_void_p(x.data_ptr())                                                 # noqa: E731
    good = [ptr(t[0]), ptr(t[1]), ptr(t[2]), coef, ptr(W), ptr(a), ptr(gc), ptr(gd), ptr(goff), ptr(c_prev), ptr(dots)]
    for fn, extra in ((lib.specinv_cgla_extrap_adjoint, []), (lib.specinv_cgla_step_adjoint, [ptr(mag_fm), ptr(gm)])):
        for i in (0, 1, 3, 5, 6, 8, 9, 10):
            args = list(good)
            args[i] = None
            assert fn(h, *args, *extra) == _lib.EINVAL, i
        for bad in ((-0.5, 1.2, 0.7, 0.4, 1.1), (0.5, -1.2, 0.7, 0.4, 1.1), (0.5, 1.2, 0.0, 0.4, 1.1), (0.5, 1.2, 0.7, -0.4, 1.1)):
            args = list(good)
            args[3] = (C.c_double * 5)(*bad)
            assert fn(h, *args, *extra) == _lib.EINVAL, bad
        args = list(good)
        args[7] = None                                               # gamma != 1 needs gd
        assert fn(h, *args, *extra) == _lib.EINVAL
    for i in range(2):
        extra = [ptr(mag_fm), ptr(gm)]
        extra[i] = None
        assert lib.specinv_cgla_step_adjoint(h, *good, *extra) == _lib.EINVAL
    first = [ptr(t[0]), ptr(W), ptr(a), ptr(gc), ptr(gd), ptr(goff), ptr(mag_fm), ptr(gm)]
    for i in (0, 2, 3, 5, 6, 7):
        args = list(first)
        args[i] = None
        assert lib.specinv_cgla_first_adjoint(h, *args) == _lib.EINVAL, i
    torch.cuda.synchronize()
    for x in (a, gc, gd, goff, c_prev, dots, gm):
        assert torch.isnan(x).all()
