"""`gla_projection`, `stft` and `istft` on the device: the forward pass against the torch restatement (tests/_proj_torch.py), the
gradients against autograd on that restatement, the fused adjoint kernel (csrc/kernels_proj_adjoint.h) against the staged path on
identical inputs, and the layer's properties.  Needs an MI355X: `-m gpu`."""
import functools

import numpy as np
import pytest
import torch

import _agla_torch as at
import _proj_torch as pt
from _util import hann, rel_l2

pytestmark = pytest.mark.gpu

import spectrogram_inversion_amd as si                                    # noqa: E402
from spectrogram_inversion_amd.plan import args_helper, clear_plan_cache, get_plan   # noqa: E402

DEV = torch.device("cuda", 0)
TDT = {np.float32: torch.float32, np.float64: torch.float64}
IDS = [f"{n} {np.dtype(d).name}" for n, d in pt.FUSED]
IDS0 = [f"{n} {np.dtype(d).name}" for n, d in pt.STAGED]


def N(t):
    return t.detach().cpu().numpy()


def T_(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _tkw(kw):
    return dict(kw, window=torch.from_numpy(kw["window"]))


def _plan(name, dtype, batch=2, frames=None):
    x, mag, w, kw = pt.inputs(name, dtype, batch, frames)
    return get_plan(args_helper(torch.empty(mag.shape[1:], dtype=TDT[dtype]), **_tkw(kw)), batch, mag.shape[2], TDT[dtype], DEV)


def _grads(name, dtype, batch=2, frames=None):
    """(y, grad x, grad mag, the plan's adjoint kind) of sum(w * gla_projection(x, mag)) on the device"""
    x, mag, w, kw = pt.inputs(name, dtype, batch, frames)
    xt, mt = T_(x).requires_grad_(True), T_(mag).requires_grad_(True)
    y = si.gla_projection(xt, mt, **_tkw(kw))
    assert y.requires_grad and y.shape == w.shape and y.dtype == xt.dtype
    (y * T_(w)).sum().backward()
    assert xt.grad.shape == xt.shape and mt.grad.shape == mt.shape
    return N(y), N(xt.grad), N(mt.grad), _plan(name, dtype, batch, frames).project_adjoint_kind


@functools.lru_cache(maxsize=None)
def _default(name, dtype):
    """... on a fresh plan with the default routing, computed once per case"""
    clear_plan_cache()
    return _grads(name, dtype)


@pytest.fixture
def env_plan(monkeypatch):
    """`env_plan(NAME, value)`: a development knob for the plans created from here on; the cache never mixes the two."""
    def go(key, value):
        monkeypatch.setenv(key, value)
        clear_plan_cache()
    yield go
    clear_plan_cache()


@pytest.mark.parametrize("name,dtype", pt.FUSED + pt.STAGED, ids=IDS + IDS0)
def test_forward_matches_the_restatement(name, dtype):
    """float64: 1e-10.  float32: the larger of 2e-5 and 6 x the restatement's own float32-against-float64 rel-L2 on the case
    (DESIGN 3.12's rule).  The same bits without grad, and with the magnitudes handed over frame-major."""
    x, mag, w, kw = pt.inputs(name, dtype)
    y = _default(name, dtype)[0]
    ref = pt.reference(name, dtype)[0]
    gate = 1e-10
    if dtype == np.float32:
        gate = max(2e-5, 6 * rel_l2(ref, pt.reference(name, dtype, np.float64)[0]))
    e = rel_l2(y, ref)
    print(f"{name} {np.dtype(dtype).name}: forward rel_l2 {e:.3e} gate {gate:.3e}")
    assert y.shape == ref.shape and e <= gate, (e, gate)
    with torch.no_grad():
        plain = si.gla_projection(T_(x), T_(mag), **_tkw(kw))
    assert not plain.requires_grad and np.array_equal(N(plain), y)
    fm = T_(mag).transpose(1, 2).contiguous().requires_grad_(True)
    yf = si.gla_projection(T_(x), fm, frame_major=True, **_tkw(kw))
    assert np.array_equal(N(yf), y)
    (yf * T_(w)).sum().backward()
    assert fm.grad.shape == fm.shape and np.array_equal(N(fm.grad.transpose(1, 2)), _default(name, dtype)[2])


@pytest.mark.parametrize("name,dtype", pt.FUSED + pt.STAGED, ids=IDS + IDS0)
def test_gradients_match_autograd_on_the_restatement(name, dtype):
    """float64: rel-L2 <= 1e-9.  float32, against the float64 gradient of the restatement on the same float32 inputs: the larger of
    2e-4 and 6 x the restatement's own float32 gradient error on the case (DESIGN 3.13 / 3.14's rule).  The kind is asserted: the
    fused kernel at every shape it covers, the staged path at 400 / 160 and two-sided."""
    _, gx, gm, kind = _default(name, dtype)
    assert kind == ("fused" if (name, dtype) in pt.FUSED else "staged"), kind
    ref = pt.reference(name, dtype, np.float64)
    own = pt.reference(name, dtype)
    for what, g, f, r in zip(("x", "mag"), (gx, gm), own[1:], ref[1:]):
        gate = 1e-9 if dtype == np.float64 else max(2e-4, 6 * rel_l2(f, r))
        e = rel_l2(g, r)
        print(f"{name} {np.dtype(dtype).name} ({kind}): grad {what} {e:.3e} gate {gate:.3e}")
        assert np.isfinite(g).all() and e <= gate, (what, e, gate)


@pytest.mark.parametrize("name,dtype", pt.FUSED, ids=IDS)
def test_fused_adjoint_matches_the_staged_path(env_plan, name, dtype):
    """Identical inputs, SPECINV_PROJ_ADJ_FUSED=0 on a fresh plan: both gradients to 1e-12 in float64 and 2e-5 in float32, DESIGN
    3.13's gates for a step against the block composition."""
    y, gx, gm, kind = _default(name, dtype)
    assert kind == "fused"
    env_plan("SPECINV_PROJ_ADJ_FUSED", "0")
    y0, gx0, gm0, kind0 = _grads(name, dtype)
    assert kind0 == "staged" and np.array_equal(y0, y)
    gate = 1e-12 if dtype == np.float64 else 2e-5
    ex, em = rel_l2(gx, gx0), rel_l2(gm, gm0)
    ref = pt.reference(name, dtype, np.float64)
    print(f"{name} {np.dtype(dtype).name}: fused against staged grad x {ex:.3e} grad mag {em:.3e}; against the float64 restatement "
          f"fused {rel_l2(gx, ref[1]):.3e} {rel_l2(gm, ref[2]):.3e} staged {rel_l2(gx0, ref[1]):.3e} {rel_l2(gm0, ref[2]):.3e}")
    assert ex <= gate and em <= gate, (ex, em)


@pytest.mark.parametrize("name,batch,frames", [("128/32", 3, 37), ("1024/256", 3, 11)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_two_waves_walk_every_group(env_plan, name, batch, frames, dtype):
    """SPECINV_PROJ_ADJ_WAVES=2: every wave walks several groups of frames, the last one partly filled (128 / 32: 111 frames in groups
    of four).  The bits of the uncapped launch."""
    clear_plan_cache()
    full = _grads(name, dtype, batch, frames)
    env_plan("SPECINV_PROJ_ADJ_WAVES", "2")
    capped = _grads(name, dtype, batch, frames)
    assert full[3] == capped[3] == "fused"
    assert np.array_equal(full[1], capped[1]) and np.array_equal(full[2], capped[2])
    ref = pt.reference(name, dtype, np.float64, batch, frames)
    gate = 1e-9 if dtype == np.float64 else max(2e-4, 6 * rel_l2(pt.reference(name, dtype, None, batch, frames)[1], ref[1]))
    assert rel_l2(capped[1], ref[1]) <= gate


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_silent_frame_and_empty_bins(dtype):
    """A stretch of x set to 0 that makes frame 5's R exactly 0, and bins with m = 0: finite gradients, the silent frame's gm row
    exactly 0, the restatement's values (torch's abs has the same derivative at 0: none)."""
    clear_plan_cache()
    x, mag, w, kw = (v.copy() if isinstance(v, np.ndarray) else v for v in pt.inputs("128/32", dtype, 2, 12))
    x[:, 96:224] = 0                                                 # frame 5 covers samples [96, 224)
    mag[:, 3:6] = 0
    mag[1, 40, 7] = 0
    xt, mt = T_(x).requires_grad_(True), T_(mag).requires_grad_(True)
    (si.gla_projection(xt, mt, **_tkw(kw)) * T_(w)).sum().backward()
    assert _plan("128/32", dtype, 2, 12).project_adjoint_kind == "fused"
    assert si.stft(T_(x), **_tkw(kw))[:, :, 5].abs().max() == 0
    gx, gm = N(xt.grad), N(mt.grad)
    assert np.isfinite(gx).all() and np.isfinite(gm).all() and not gm[:, :, 5].any()
    wide = lambda v: v.astype(np.float64)                                      # noqa: E731
    xr, mr = torch.from_numpy(wide(x)).requires_grad_(True), torch.from_numpy(wide(mag)).requires_grad_(True)
    (pt.project(xr, mr, **dict(kw, window=wide(kw["window"]))) * torch.from_numpy(wide(w))).sum().backward()
    ex, em = rel_l2(gx, xr.grad.numpy()), rel_l2(gm, mr.grad.numpy())
    print(f"silent frame {np.dtype(dtype).name}: grad x {ex:.3e} grad mag {em:.3e}")
    # (float32: the silent frame's gR is gQ m / 1e-16, whose float32 rounding dominates both norms - relative 2e-4 still)
    assert ex <= (1e-9 if dtype == np.float64 else 2e-4) and em <= (1e-9 if dtype == np.float64 else 2e-4)


@pytest.mark.parametrize("wrt", ["x", "mag"])
def test_gradient_matches_a_central_difference_of_the_forward(wrt):
    """Independent of the restatement: float64, d/dt of sum(w * gla_projection(...)) without grad at h = 1e-6 against <grad,
    direction> along a random unit direction.  Relative 1e-6: the truncation is O(h^2), the rounding about 1e-10."""
    x, mag, w, kw = pt.inputs("128/32", np.float64)
    _, gx, gm, kind = _default("128/32", np.float64)
    assert kind == "fused"
    d = np.random.default_rng(11).standard_normal((x if wrt == "x" else mag).shape)
    d /= np.linalg.norm(d)
    ip = float(((gx if wrt == "x" else gm) * d).sum())
    h = 1e-6

    def f(t):
        with torch.no_grad():
            y = si.gla_projection(T_(x + t * d if wrt == "x" else x), T_(mag + t * d if wrt == "mag" else mag), **_tkw(kw))
        return float((N(y) * w).sum())

    fd = (f(h) - f(-h)) / (2 * h)
    print(f"d/d{wrt}: central difference {fd:.12e}  <grad, direction> {ip:.12e}  relative {abs(fd - ip) / abs(fd):.3e}")
    assert abs(fd - ip) <= 1e-6 * abs(fd), (fd, ip)


@pytest.mark.parametrize("name,dtype", [("128/32", np.float32), ("1024/256", np.float32), ("2048/512", np.float64), ("400/160", np.float32)])
def test_backward_twice_gives_identical_gradients(name, dtype):
    x, mag, w, kw = pt.inputs(name, dtype)
    xt, mt = T_(x).requires_grad_(True), T_(mag).requires_grad_(True)
    loss = (si.gla_projection(xt, mt, **_tkw(kw)) * T_(w)).sum()
    first = torch.autograd.grad(loss, (xt, mt), retain_graph=True)
    second = torch.autograd.grad(loss, (xt, mt))
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    assert all(torch.isfinite(a).all() and a.abs().max() > 0 for a in first)


@pytest.mark.parametrize("name,dtype", [("1024/256", np.float32), ("128/32", np.float64), ("400/160", np.float32)])
def test_the_layer_leaves_a_running_griffin_lim_as_it_was(name, dtype):
    """griffin_lim's six iterations, interrupted after three by a forward and a backward pass of the layer on the same plan."""
    clear_plan_cache()
    x, mag, w, kw = pt.inputs(name, dtype)
    plan = _plan(name, dtype)

    def run(interrupt):
        plan.gla_init(None, T_(mag), 0.3)
        plan.iterate(3)
        if interrupt:
            xt, mt = T_(x).requires_grad_(True), T_(mag).requires_grad_(True)
            y = si.gla_projection(xt, mt, **_tkw(kw))
            assert _plan(name, dtype) is plan
            (y * T_(w)).sum().backward()
            assert xt.grad.abs().max() > 0
        plan.iterate(3)
        return plan.wave()

    plain = run(False)
    assert torch.equal(run(True), plain) and torch.equal(run(False), plain)


def test_a_loop_around_the_layer_is_agla_unfolded():
    """x <- t + alpha (t - t_prev), t = gla_projection(c, mag), written in torch ops around the layer from istft(start): three
    iterations in float64 at 128 / 32 are agla_unfolded(start, 3, alpha) - output and the gradients of start and alpha to 1e-9."""
    spec, w, L, kw = at.inputs("128/32", np.float64, False)
    kw = dict(kw, window=torch.from_numpy(kw["window"]))
    al0 = torch.tensor([0.99, 0.6, 0.8], dtype=torch.float64)

    s1, a1 = T_(spec).requires_grad_(True), al0.clone().requires_grad_(True)
    y1 = si.agla_unfolded(s1, 3, a1, **kw)
    (y1 * T_(w)).sum().backward()

    s2, a2 = T_(spec).requires_grad_(True), al0.clone().requires_grad_(True)
    mag, ad = s2.abs(), a2.to(DEV)
    c = si.istft(s2, **kw)
    t = None
    for n in range(3):
        y = si.gla_projection(c, mag, **kw)
        c = y if t is None else y + ad[n] * (y - t)
        t = y
    (t * T_(w)).sum().backward()
    ey, es, ea = rel_l2(N(t), N(y1)), rel_l2(N(s2.grad), N(s1.grad)), rel_l2(N(a2.grad)[1:], N(a1.grad)[1:])
    print(f"loop around the layer against agla_unfolded: y {ey:.3e} grad start {es:.3e} grad alpha {ea:.3e}")
    assert ey <= 1e-9 and es <= 1e-9 and ea <= 1e-9 and a2.grad[0] == 0


@pytest.mark.parametrize("name", ["128/32", "64/16 two-sided normalized"])
def test_stft_and_istft(name):
    """Values: Plan.stft / Plan.istft bit for bit.  Gradients: autograd of the restatement, float64, 1e-9."""
    clear_plan_cache()
    x, mag, w, kw = pt.inputs(name, np.float64)
    plan = _plan(name, np.float64)
    n_fft = pt.CONFIGS[name][0]
    rng = np.random.default_rng(3)
    ws = rng.standard_normal(mag.shape) + 1j * rng.standard_normal(mag.shape)
    xt = T_(x).requires_grad_(True)
    S = si.stft(xt, n_fft=n_fft, **_tkw(kw))
    assert torch.equal(S.detach(), plan.stft(T_(x))) and S.shape == mag.shape
    (S * T_(ws).conj()).real.sum().backward()
    xr = torch.from_numpy(x).requires_grad_(True)
    (pt.stft(xr, mag.shape[1], **kw) * torch.from_numpy(ws).conj()).real.sum().backward()
    e1 = rel_l2(N(xt.grad), xr.grad.numpy())
    start = mag * np.exp(1j * rng.uniform(-np.pi, np.pi, mag.shape))
    st = T_(start).requires_grad_(True)
    y = si.istft(st, **_tkw(kw))
    assert torch.equal(y.detach(), plan.istft(T_(start))) and y.shape == x.shape
    (y * T_(w)).sum().backward()
    sr = torch.from_numpy(start).requires_grad_(True)
    (pt.istft(sr, **kw) * torch.from_numpy(w)).sum().backward()
    e2 = rel_l2(N(st.grad), sr.grad.numpy())
    print(f"{name}: stft grad {e1:.3e} istft grad {e2:.3e}")
    assert e1 <= 1e-9 and e2 <= 1e-9
    # one waveform, a CPU tensor, float32: shape, device and dtype of the input
    S1 = si.stft(torch.from_numpy(x[0]).float(), n_fft=n_fft, **_tkw(kw))
    assert S1.shape == mag.shape[1:] and S1.device.type == "cpu" and S1.dtype == torch.complex64
    y1 = si.istft(torch.from_numpy(start[0]).to(torch.complex64), **_tkw(kw))
    assert y1.shape == x.shape[1:] and y1.device.type == "cpu" and y1.dtype == torch.float32


def test_gradients_come_back_as_the_inputs_are():
    x, mag, w, kw = pt.inputs("128/32", np.float32)
    kw = _tkw(kw)
    ref = _default("128/32", np.float32)
    # one item without a batch axis, on the CPU
    x1, m1 = torch.from_numpy(x[0]).requires_grad_(True), torch.from_numpy(mag[0]).requires_grad_(True)
    y = si.gla_projection(x1, m1, **kw)
    assert y.shape == x1.shape and y.device.type == "cpu" and y.dtype == torch.float32
    (y * torch.from_numpy(w[0])).sum().backward()
    assert x1.grad.shape == x1.shape and m1.grad.shape == m1.shape and x1.grad.device.type == "cpu" and m1.grad.device.type == "cpu"
    assert rel_l2(N(x1.grad), ref[1][0]) <= 2e-5 and rel_l2(N(m1.grad), ref[2][0]) <= 2e-5
    # float64 magnitudes beside a float32 signal: each gets its own dtype back
    xm, mm = T_(x).requires_grad_(True), T_(mag).double().requires_grad_(True)
    (si.gla_projection(xm, mm, **kw) * T_(w)).sum().backward()
    assert xm.grad.dtype == torch.float32 and mm.grad.dtype == torch.float64 and np.array_equal(N(xm.grad), ref[1])
    for half in (torch.float16, torch.bfloat16):
        xh, mh = T_(x).to(half).requires_grad_(True), T_(mag).to(half).requires_grad_(True)
        yh = si.gla_projection(xh, mh, **kw)
        assert yh.dtype == half and yh.shape == xh.shape
        yh.float().sum().backward()
        assert xh.grad.dtype == half and mh.grad.dtype == half and xh.grad.shape == xh.shape and mh.grad.shape == mh.shape
        assert torch.isfinite(xh.grad.float()).all() and torch.isfinite(mh.grad.float()).all()


def test_an_empty_batch():
    kw = dict(hop_length=32, window=torch.from_numpy(hann(128, np.float32)))
    x, mag = torch.zeros(0, 256, device=DEV, requires_grad=True), torch.ones(0, 65, 9, device=DEV, requires_grad=True)
    y = si.gla_projection(x, mag, **kw)
    assert y.shape == (0, 256) and y.requires_grad and y.device == x.device
    y.sum().backward()
    assert x.grad.shape == x.shape and mag.grad.shape == mag.shape
