"""consistent_wiener on the device against its definition in torch on the CPU (tests/_cwf_oracle.py), on the input's own bits.

Shapes: n_fft 64 / hop 16 with 5 frames (F T = 165 bins: an odd item against the kernels' groups of four, so items 1 and 2 of a
batch start off a 16-byte boundary and take the element loads), 128 / 32 with 9, 512 / 128 with 7 (more than one workgroup per
item) and 400 / 160 with 6 (the coverage transforms).  Three items at scales 0.1, 1, 10: chirps in noise, the target's power known
and the noise variance flat.  8 iterations at gamma = 10.

Tolerance, not a number fixed in advance: nu32 is the relative L2 distance between the oracle in float32 (float64 sums) and in
float64 on the same float32 inputs, per item.  The float32 bound is 16 nu32, the float64 bound 16 nu32 eps64 / eps32; the 16 covers
the device's FFT and summation order.  nu32 < 1e-5 is asserted, so the inputs stay well conditioned.  The residual traces
sqrt(rz / rz0) after 1 ... 8 iterations, as vectors, are held to the same bounds (the item's nu32 of S: the traces' own float32
distance is printed beside it, it scatters from 4e-8 to 8e-7 and would make the bound a matter of luck).  Every figure is printed
before it is asserted; DESIGN 3.25 records them.
"""
import pytest
import torch

import spectrogram_inversion_amd as si
import _layouts as L
from _cwf_oracle import chirps_in_noise, cwf

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
CPLX = {F32: torch.complex64, F64: torch.complex128}
EPS = {F32: 2.0 ** -23, F64: 2.0 ** -52}
DEV = "cuda"
SHAPES = [(64, 16, 5), (128, 32, 9), (512, 128, 7), (400, 160, 6)]
SCALES = (0.1, 1.0, 10.0)
N_ITER, GAMMA = 8, 10.0


def _kw(n_fft, hop, dtype):
    return dict(hop_length=hop, window=torch.hann_window(n_fft, dtype=dtype))


def _inputs(n_fft, hop, frames, dtype, scales=SCALES, seed=0):
    """(X, v_s, v_n) on the CPU in `dtype`: per item chirps in noise at its scale, |target|^2 and the noise's mean power"""
    kw = _kw(n_fft, hop, F64)
    X, vs, vn = [], [], []
    for b, c in enumerate(scales):
        s, n = chirps_in_noise((frames - 1) * hop, seed + 7 * b + n_fft, noise=0.85)
        St, Nt = (torch.stft(c * v, n_fft, return_complex=True, **kw) for v in (s, n))
        X.append(St + Nt)
        vs.append(St.abs() ** 2)
        vn.append((Nt.abs() ** 2).mean().expand(St.shape))
    return torch.stack(X).to(CPLX[dtype]), torch.stack(vs).to(dtype), torch.stack(vn).to(dtype)


def _rel(a, b):
    """relative L2 distance per item"""
    d = (a.to(torch.complex128) - b.to(torch.complex128)).flatten(1).norm(dim=1) if a.is_complex() else (a - b).flatten(1).norm(dim=1)
    n = b.to(torch.complex128).flatten(1).norm(dim=1) if b.is_complex() else b.flatten(1).norm(dim=1)
    return d / n


_REF = {}


def reference(shape, dtype):
    """the inputs of (shape, dtype), the float64 oracle on them (S, N, residual traces) and nu32 of S and of the traces, per item"""
    key = (shape, dtype)
    if key not in _REF:
        n_fft, hop, frames = shape
        X, vs, vn = _inputs(n_fft, hop, frames, dtype)
        run = dict(gamma=GAMMA, n_iter=N_ITER, hop_length=hop)
        S, N, res = cwf(X, vs, vn, dtype=F64, window=torch.hann_window(n_fft, dtype=F64), **run)
        X32, vs32, vn32 = _inputs(n_fft, hop, frames, F32)
        S64, _, res64 = cwf(X32, vs32, vn32, dtype=F64, window=torch.hann_window(n_fft, dtype=F64), **run)
        S32, _, res32 = cwf(X32, vs32, vn32, dtype=F32, window=torch.hann_window(n_fft, dtype=F32), **run)
        _REF[key] = (X, vs, vn, S, N, res, _rel(S32, S64), _rel(res32[:, 1:], res64[:, 1:]))
    return _REF[key]


CASES = [(s, d) for s in SHAPES for d in (F32, F64)]
IDS = [f"{s[0]}-{s[1]}-{s[2]}-{'f32' if d == F32 else 'f64'}" for s, d in CASES]


def _bound(nu32, dtype):
    return 16 * nu32 * (1.0 if dtype == F32 else EPS[F64] / EPS[F32])


@pytest.mark.parametrize("shape,dtype", CASES, ids=IDS)
def test_parity_with_the_definition(shape, dtype):
    X, vs, vn, S_ref, N_ref, _, nu32, _ = reference(shape, dtype)
    S, N = si.consistent_wiener(X.to(DEV), vs.to(DEV), vn.to(DEV), gamma=GAMMA, n_iter=N_ITER, **_kw(shape[0], shape[1], dtype))
    assert S.dtype == N.dtype == CPLX[dtype] and S.shape == N.shape == X.shape and S.device.type == "cuda"
    dist, dist_n, bound = _rel(S.cpu(), S_ref), _rel(N.cpu(), N_ref), _bound(nu32, dtype)
    print(f"nu32 {nu32.tolist()} device distance S {dist.tolist()} N {dist_n.tolist()} bound {bound.tolist()}")
    assert (nu32 < 1e-5).all()
    assert (dist <= bound).all()
    # (N = X - S: its distance is S's, measured against |N|)
    assert (dist_n * N_ref.flatten(1).norm(dim=1) <= bound * S_ref.flatten(1).norm(dim=1)).all()


@pytest.mark.parametrize("shape,dtype", CASES, ids=IDS)
def test_residual_trace_at_every_iteration(shape, dtype):
    X, vs, vn, _, _, res_ref, nu32, nu32_trace = reference(shape, dtype)
    Xd, vsd, vnd = X.to(DEV), vs.to(DEV), vn.to(DEV)
    trace = []
    for k in range(1, N_ITER + 1):
        *_, info = si.consistent_wiener(Xd, vsd, vnd, gamma=GAMMA, n_iter=k, return_info=True, **_kw(shape[0], shape[1], dtype))
        assert info["n_iter"] == k and info["residual"].dtype == F64 and info["residual"].shape == (3,)
        trace.append(info["residual"].cpu())
    trace = torch.stack(trace, 1)
    dist, bound = _rel(trace, res_ref[:, 1:]), _bound(nu32, dtype)
    print(f"oracle trace {res_ref.tolist()}\ndevice trace {trace.tolist()}\nnu32 {nu32.tolist()} (the traces' own "
          f"{nu32_trace.tolist()}) distance {dist.tolist()} bound {bound.tolist()}")
    assert (dist <= bound).all()


def _floored(vs, vn, floor=1e-8):
    m = floor * (vs.double() + vn.double()).flatten(1).max(dim=1).values
    m = m.to(vs.dtype)[:, None, None]
    return torch.maximum(vs, m), torch.maximum(vn, m)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_zero_iterations_is_the_wiener_estimate_and_the_parts_add_up(dtype):
    X, vs, vn = (t.to(DEV) for t in _inputs(64, 16, 5, dtype))
    kw = _kw(64, 16, dtype)
    S, N, info = si.consistent_wiener(X, vs, vn, n_iter=0, return_info=True, **kw)
    ps, pn = _floored(vs, vn)
    want = ps / (ps + pn) * X
    gap = float(((S - want).abs() / want.abs()).max())
    print(f"n_iter=0: largest relative gap to the gain times X {gap:.3e}")
    assert gap <= EPS[dtype]
    assert info["n_iter"] == 0 and torch.equal(info["residual"].cpu(), torch.ones(3, dtype=F64))
    for n_iter in (0, 5):
        S, N = si.consistent_wiener(X, vs, vn, n_iter=n_iter, **kw)
        assert torch.equal(N, X - S)
        r = lambda Z: torch.view_as_real(Z)                              # noqa: E731
        # one rounding of N = X - S (half an ulp of N) and the one of this sum (half an ulp of X), component by component
        assert ((r(S + N) - r(X)).abs() <= EPS[dtype] / 2 * (r(N).abs() + r(X).abs())).all()


@pytest.mark.parametrize("shape,dtype", [c for c in CASES if c[0] in SHAPES[:3]], ids=[i for c, i in zip(CASES, IDS) if c[0] in SHAPES[:3]])
def test_an_item_of_a_batch_equals_the_item_alone_and_runs_repeat(shape, dtype):
    X, vs, vn = (t.to(DEV) for t in _inputs(*shape, dtype))
    kw = _kw(shape[0], shape[1], dtype)
    S, N, info = si.consistent_wiener(X, vs, vn, gamma=GAMMA, n_iter=5, return_info=True, **kw)
    S2, N2, info2 = si.consistent_wiener(X, vs, vn, gamma=GAMMA, n_iter=5, return_info=True, **kw)
    assert torch.equal(S, S2) and torch.equal(N, N2) and torch.equal(info["residual"], info2["residual"])
    for b in range(3):
        Sb, Nb, ib = si.consistent_wiener(X[b], vs[b], vn[b], gamma=GAMMA, n_iter=5, return_info=True, **kw)
        assert Sb.shape == X[b].shape
        assert torch.equal(Sb, S[b]) and torch.equal(Nb, N[b]) and torch.equal(ib["residual"], info["residual"][b:b + 1])


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_silent_and_dead_items_come_back_zero(dtype):
    X, vs, vn = (t.to(DEV) for t in _inputs(64, 16, 5, dtype, scales=(1.0, 1.0, 1.0, 1.0)))
    X[1] = 0                              # an all-zero mixture
    vs[2] = 0                             # all-zero variances
    vn[2] = 0
    S, N, info = si.consistent_wiener(X, vs, vn, gamma=GAMMA, n_iter=4, return_info=True, **_kw(64, 16, dtype))
    assert not S[1].any() and not N[1].any() and not S[2].any() and torch.equal(N[2], X[2])
    assert torch.isfinite(torch.view_as_real(S)).all() and torch.isfinite(torch.view_as_real(N)).all()
    assert info["residual"][1] == 0 and info["residual"][2] == 0 and (info["residual"][[0, 3]] > 0).all()
    for b in (0, 3):
        Sb, _ = si.consistent_wiener(X[b], vs[b], vn[b], gamma=GAMMA, n_iter=4, **_kw(64, 16, dtype))
        assert torch.equal(Sb, S[b]) and S[b].any()


def test_tol_stops_at_an_evaluation():
    X, vs, vn = _inputs(128, 32, 9, F32, scales=(1.0,))
    kw = _kw(128, 32, F32)
    _, _, res = cwf(X, vs, vn, dtype=F64, gamma=1.0, n_iter=20, hop_length=32, window=torch.hann_window(128, dtype=F64))
    r10, r20 = float(res[0, 10]), float(res[0, 20])
    print(f"oracle residual after 10: {r10:.3e}, after 20: {r20:.3e}")
    assert r20 < r10
    tol = (r10 * r20) ** 0.5
    *_, info = si.consistent_wiener(X.to(DEV), vs.to(DEV), vn.to(DEV), gamma=1.0, n_iter=50, tol=tol, eva_iter=10, return_info=True, **kw)
    assert info["n_iter"] == 20 and float(info["residual"][0]) <= tol
    *_, info = si.consistent_wiener(X.to(DEV), vs.to(DEV), vn.to(DEV), gamma=1.0, n_iter=50, tol=0.0, eva_iter=10, return_info=True, **kw)
    assert info["n_iter"] == 50


@pytest.mark.parametrize("arg,name", [("mix_spec", "strided"), ("mix_spec", "conj"), ("var_target", "strided"), ("var_noise", "offset")])
def test_a_view_gives_the_bits_of_its_dense_twin(arg, name):
    X, vs, vn = (t.to(DEV) for t in _inputs(64, 16, 5, F32))
    dense = {"mix_spec": X, "var_target": vs, "var_noise": vn}
    kw = _kw(64, 16, F32)
    want = si.consistent_wiener(**dense, gamma=GAMMA, n_iter=3, **kw)
    view, base = L.build(name, dense[arg])
    before = base.clone()
    got = si.consistent_wiener(**{**dense, arg: view}, gamma=GAMMA, n_iter=3, **kw)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(torch.view_as_real(base) if base.is_complex() else base, torch.view_as_real(before) if base.is_complex() else before)


def test_broadcast_variances_cpu_tensors_and_half():
    X, vs, vn = _inputs(64, 16, 5, F32)
    kw = _kw(64, 16, F32)
    want = si.consistent_wiener(X.to(DEV), vs.to(DEV), vn.to(DEV), n_iter=3, **kw)
    got = si.consistent_wiener(X, vs, vn[:, :1, :1], n_iter=3, **kw)              # CPU in, CPU out; a (B, 1, 1) noise variance
    assert got[0].device.type == "cpu" and torch.equal(got[0], want[0].cpu()) and torch.equal(got[1], want[1].cpu())
    half = si.consistent_wiener(X.to(torch.complex32).to(DEV), vs.to(DEV), vn.to(DEV), n_iter=3, **kw)
    assert half[0].dtype == torch.complex32
    exact = si.consistent_wiener(X.to(torch.complex32).to(CPLX[F32]).to(DEV), vs.to(DEV), vn.to(DEV), n_iter=3, **kw)
    assert torch.equal(torch.view_as_real(half[0]), torch.view_as_real(exact[0].to(torch.complex32)))


def test_audio_parts_add_up_to_the_input():
    """x_n is x[:L'] - x_s bit for bit.  The float32 sum x_s + x_n then differs from x by the rounding of that difference and its
    own: half an ulp of x_n and half an ulp of x (an exact identity does not exist in floating point: where |x_s| exceeds
    2 |x|, x - x_s is not representable)."""
    s, n = chirps_in_noise(2048 + 37, 5, noise=0.85)
    x = torch.stack([s + n, 0.5 * s - n]).to(F32).to(DEV)
    kw = _kw(128, 32, F32)
    Xs = si.stft(x, 128, **kw)
    vs, vn = (0.6 * Xs.abs()) ** 2, (0.4 * Xs.abs()) ** 2
    x_s, x_n, info = si.consistent_wiener_audio(x, vs, vn, 128, n_iter=4, return_info=True, **kw)
    S, _ = si.consistent_wiener(Xs, vs, vn, n_iter=4, **kw)
    assert info["n_iter"] == 4
    Lp = x_s.shape[-1]
    assert x_s.shape == x_n.shape == (2, Lp) and Lp == (Xs.shape[-1] - 1) * 32 and x_s.dtype == F32
    assert torch.equal(x_s, si.istft(S, **kw))
    assert torch.equal(x_n, x[:, :Lp] - x_s)
    gap = (x_s + x_n - x[:, :Lp]).abs()
    print(f"largest |x_s + x_n - x| {float(gap.max()):.3e}")
    assert (gap <= EPS[F32] / 2 * (x_n.abs() + x[:, :Lp].abs())).all()
    one = si.consistent_wiener_audio(x[0], vs[0], vn[0], 128, n_iter=4, **kw)
    assert one[0].shape == (Lp,) and torch.equal(one[0], x_s[0])


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_a_call_does_not_disturb_a_running_method(dtype):
    from spectrogram_inversion_amd.plan import args_helper, get_plan
    X, vs, vn = (t.to(DEV) for t in _inputs(128, 32, 9, dtype))
    kw = _kw(128, 32, dtype)
    plan = get_plan(args_helper(X, **kw), 3, X.shape[-1], dtype, X.device)

    def run(between):
        plan.gla_init(X, X.abs(), 0.99)
        plan.iterate(2)
        between()
        plan.iterate(2)
        return plan.wave().clone()

    quiet = run(lambda: None)
    busy = run(lambda: si.consistent_wiener(X, vs, vn, gamma=GAMMA, n_iter=3, **kw))
    assert torch.equal(quiet, busy)
