"""The hand-written adjoints behind the spectrogram gradients, block by block on identical inputs: `stft_adjoint` / `istft_adjoint`
on every transform route (adjoint identities, and the values against float64 autograd on tests/_misi_torch.py), `gla_update_adjoint` /
`admm_update_adjoint` against float64 autograd on the restated step (tests/_gla_torch.py), `phase_init_adjoint` beyond one 64-lane
chunk of frames.  Float32 gates are the larger of 2e-5 and 6 x the restatement's own float32-against-float64 error on the case
(DESIGN 3.12's rule); float64 gates are fixed.  Needs an MI355X."""
import functools

import numpy as np
import pytest
import torch

import _agla_torch as at
import _gla_torch as gt
import _misi_torch as mt
from _proj_torch import hamming
from _util import hann, rel_l2

pytestmark = pytest.mark.gpu

from spectrogram_inversion_amd.plan import Plan, args_helper          # noqa: E402

DEV = torch.device("cuda", 0)
F32, F64 = np.float32, np.float64


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def tdt(dtype):
    return torch.float32 if dtype == F32 else torch.float64


def cdt(dtype):
    return np.complex64 if dtype == F32 else np.complex128


# ---- the linear blocks ---------------------------------------------------------------------------------------------------------------
# id: dtype, n_fft, hop, frames, batch, extra stft kwargs (center=False: a Hamming window, its envelope has no zeros)
WAVE = {                                                         # float32, the wave-level transform (n_fft 512 ... 4096)
    "512/128x70": (F32, 512, 128, 70, 3, {}),
    "1024/256x70 center=False": (F32, 1024, 256, 70, 3, dict(center=False)),
    "2048/512x20 normalized": (F32, 2048, 512, 20, 3, dict(normalized=True)),
    "4096/1024x6": (F32, 4096, 1024, 6, 3, {}),
    "1024/200/800 replicate": (F32, 1024, 200, 9, 3, dict(win_length=800, pad_mode="replicate")),
    "512/170 circular": (F32, 512, 170, 9, 3, dict(pad_mode="circular")),
    "2048/1024x5 reflect": (F32, 2048, 1024, 5, 3, dict(pad_mode="reflect")),
    "512/128x9 constant": (F32, 512, 128, 9, 3, dict(pad_mode="constant")),
}
OTHER = {
    "f32 two-sided 512/128x10": (F32, 512, 128, 10, 3, dict(onesided=False)),
    "f32 8192/2048x4": (F32, 8192, 2048, 4, 3, {}),
    "f32 400/160x12": (F32, 400, 160, 12, 3, {}),
    "f32 1000/250x8": (F32, 1000, 250, 8, 3, {}),
    "f32 1018/509x6": (F32, 1018, 509, 6, 3, {}),                 # 2 x 509, a large prime factor
    "f32 128/32x70": (F32, 128, 32, 70, 3, {}),
    "f32 256/100/200x9": (F32, 256, 100, 9, 3, dict(win_length=200)),
    "f64 512/128x70": (F64, 512, 128, 70, 3, {}),
    "f64 1024/256x12": (F64, 1024, 256, 12, 3, {}),
    "f64 2048/512x10": (F64, 2048, 512, 10, 3, {}),
    "f64 4096/1024x5": (F64, 4096, 1024, 5, 3, {}),
    "f64 8192/2048x3 constant": (F64, 8192, 2048, 3, 3, dict(pad_mode="constant")),      # (3 frames: no longer than n_fft / 2)
    "f64 400/100x12": (F64, 400, 100, 12, 3, {}),
    "f64 two-sided 512/100/300x9": (F64, 512, 100, 9, 3, dict(win_length=300, onesided=False)),
    "f64 64/20x11 circular": (F64, 64, 20, 11, 3, dict(pad_mode="circular")),
    # four steps through device memory (kernels_big.h); three frames are no longer than n_fft / 2, which reflect padding cannot take
    "f32 four-step 32768/8192x3 constant": (F32, 32768, 8192, 3, 1, dict(pad_mode="constant")),
    "f64 four-step 16384/4096x3 replicate": (F64, 16384, 4096, 3, 1, dict(pad_mode="replicate")),
}
LINEAR = {**WAVE, **OTHER}


def _kwargs(case, dtype):
    _, n_fft, hop, _, _, extra = LINEAR[case]
    wl = extra.get("win_length", n_fft)
    win = hamming(wl, dtype) if extra.get("center") is False else hann(wl, dtype)
    return dict(hop_length=hop, window=win, **extra)


def _plan(case):
    dtype, n_fft, hop, frames, batch, extra = LINEAR[case]
    kw = _kwargs(case, dtype)
    F = n_fft // 2 + 1 if extra.get("onesided", True) else n_fft
    a = args_helper(torch.empty(1, F, 1, dtype=tdt(dtype)), **dict(kw, window=torch.from_numpy(kw["window"])))
    return Plan(a, batch, frames, tdt(dtype), DEV)


@functools.lru_cache(maxsize=None)
def _linear_reference(case):
    """Random normal x, Y, g of the case's dtype, and float64 autograd on tests/_misi_torch.py's transforms on them:
    (x, Y, g, stft_adjoint(Y), istft_adjoint(g), and the restatement's own float32 errors of the two (0 in float64))"""
    dtype, n_fft, hop, frames, batch, extra = LINEAR[case]
    F = n_fft // 2 + 1 if extra.get("onesided", True) else n_fft
    a64, w64 = mt._setup(F, torch.float64, _kwargs(case, F64))
    L = int(mt.envelope(frames, a64, w64).shape[0])
    rng = np.random.default_rng(n_fft + hop + frames)
    x, g = rng.standard_normal((batch, L)).astype(dtype), rng.standard_normal((batch, L)).astype(dtype)
    Y = (rng.standard_normal((batch, F, frames)) + 1j * rng.standard_normal((batch, F, frames))).astype(cdt(dtype))

    def adjoints(compute):
        a, w = mt._setup(F, tdt(compute), _kwargs(case, compute))
        env = mt.envelope(frames, a, w)
        Yt, gt_ = torch.from_numpy(Y.astype(cdt(compute))), torch.from_numpy(g.astype(compute))
        xt = torch.zeros((batch, L), dtype=tdt(compute), requires_grad=True)
        S = mt.stft(xt, a, w)
        (S.real * Yt.real + S.imag * Yt.imag).sum().backward()
        Yl = Yt.clone().requires_grad_(True)
        (mt.istft(Yl, a, w, env) * gt_).sum().backward()
        return xt.grad.numpy(), Yl.grad.numpy()

    sa, ia = adjoints(F64)
    e_sa = e_ia = 0.0
    if dtype == F32:
        sa32, ia32 = adjoints(F32)
        e_sa, e_ia = rel_l2(sa32, sa), rel_l2(ia32, ia)
    return x, Y, g, sa, ia, e_sa, e_ia


def _rdot(u, v):
    return float((u.conj() * v).real.sum()) if u.is_complex() else float((u * v).sum())


def _check_linear(case, plan, tag):
    dtype, _, _, _, _, extra = LINEAR[case]
    x, Y, g, sa_ref, ia_ref, e_sa, e_ia = _linear_reference(case)
    x, Y, g = T(x), T(Y), T(g)
    tol = 2e-5 if dtype == F32 else 1e-12
    sa, ia = plan.stft_adjoint(Y, plan.length), plan.istft_adjoint(g)
    lhs, rhs = _rdot(plan.stft(x), Y), _rdot(x, sa)
    d_stft = abs(lhs - rhs) / max(1.0, abs(lhs))
    Y0 = Y.clone()
    if extra.get("onesided", True):                     # irfft ignores the imaginary parts of DC / Nyquist
        Y0[:, 0].imag.zero_()
        Y0[:, -1].imag.zero_()
    lhs, rhs = _rdot(plan.istft(Y), g), _rdot(Y0, ia)
    d_istft = abs(lhs - rhs) / max(1.0, abs(lhs))
    err_sa, err_ia = rel_l2(N(sa), sa_ref), rel_l2(N(ia), ia_ref)
    gate_sa, gate_ia = (max(2e-5, 6 * e_sa), max(2e-5, 6 * e_ia)) if dtype == F32 else (1e-10, 1e-10)
    print(f"{case} [{tag}, plan.path {plan.path}]: identities stft {d_stft:.2e} istft {d_istft:.2e} (gate {tol:.0e}); against float64 "
          f"autograd stft_adjoint {err_sa:.2e} (gate {gate_sa:.2e}) istft_adjoint {err_ia:.2e} (gate {gate_ia:.2e})")
    assert d_stft < tol and d_istft < tol, (case, tag, d_stft, d_istft)
    assert err_sa <= gate_sa and err_ia <= gate_ia, (case, tag, err_sa, gate_sa, err_ia, gate_ia)
    return sa, ia


@pytest.mark.parametrize("case", list(LINEAR))
def test_linear_adjoints_on_every_route(case):
    _check_linear(case, _plan(case), "default route")


@pytest.mark.parametrize("case", list(WAVE))
def test_linear_adjoints_on_the_generic_route(case):
    """The eight wave-level cases again with `force_generic`: the restatement's values, and the default route's to 2e-5."""
    sa, ia = _check_linear(case, _plan(case), "default route")
    plan = _plan(case)
    plan.force_generic(True)
    sa_g, ia_g = _check_linear(case, plan, "force_generic")
    e_sa, e_ia = rel_l2(N(sa), N(sa_g)), rel_l2(N(ia), N(ia_g))
    print(f"{case}: default route against generic stft_adjoint {e_sa:.2e} istft_adjoint {e_ia:.2e}")
    assert e_sa <= 2e-5 and e_ia <= 2e-5, (case, e_sa, e_ia)


# ---- the element-wise steps ----------------------------------------------------------------------------------------------------------
# (B, F, T), n_fft, two-sided
STEP_SHAPES = [((3, 65, 9), 128, False), ((2, 64, 11), 64, True), ((1, 1025, 5), 2048, False), ((3, 201, 7), 400, False)]
T_ZERO, F_M0, F_S0 = 2, 5, 7            # a frame with S = 0 and m = 0; a bin with m = 0; a bin with S = 0 and m > 0


def _step_plan(shape, n_fft, twosided, dtype):
    kw = dict(hop_length=n_fft // 4, window=torch.from_numpy(hann(n_fft, dtype)))
    if twosided:
        kw["onesided"] = False
    return Plan(args_helper(torch.empty(1, shape[1], 1, dtype=tdt(dtype)), **kw), shape[0], shape[2], tdt(dtype), DEV)


def _cplx(rng, shape, dtype, lo=0.1, hi=2.0):
    """modulus in [lo, hi], uniform phase"""
    return (rng.uniform(lo, hi, shape) * np.exp(1j * rng.uniform(-np.pi, np.pi, shape))).astype(cdt(dtype))


def _step_inputs(shape, dtype, seed):
    """S (the recorded, pre-projection spectrum: |S| in [0.1, 2] but for the special entries), m, two more state tensors that vanish
    wherever S does (so that the float64 step reproduces S = 0 exactly there), a starting `gmag`, and four complex cotangents"""
    rng = np.random.default_rng(seed)
    S, m = _cplx(rng, shape, dtype), rng.uniform(0.1, 2.0, shape).astype(dtype)
    S[:, :, T_ZERO], m[:, :, T_ZERO] = 0, 0
    m[:, F_M0] = 0
    S[:, F_S0] = 0
    m[:, F_S0, :T_ZERO], m[:, F_S0, T_ZERO + 1:] = 0.7, 1.3
    A, Bs = _cplx(rng, shape, dtype), _cplx(rng, shape, dtype)
    A[S == 0], Bs[S == 0] = 0, 0
    gmag0 = rng.standard_normal(shape).astype(dtype)
    cot = [(rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(cdt(dtype)) for _ in range(4)]
    own = np.zeros(shape, dtype=bool)
    own[:, F_S0] = True
    own[:, :, T_ZERO] = False                       # (there m = 0 too)
    return S, m, A, Bs, gmag0, cot, own


def _compare_step(what, dtype, names, dev, ref64, ref32, own):
    """Each output against float64 autograd; the entries of the S = 0, m > 0 bin (gradients of order m / 1e-16) on their own"""
    for name, d, r64, r32 in zip(names, dev, ref64, ref32):
        d = N(d)
        assert np.isfinite(d).all(), (what, name)
        for part, sel in (("", ~own), (" [S = 0, m > 0]", own)):
            if not np.abs(r64[sel]).sum():
                assert not np.abs(d[sel]).sum(), (what, name, part)
                continue
            err = rel_l2(d[sel], r64[sel])
            gate = max(2e-5, 6 * rel_l2(r32[sel], r64[sel])) if dtype == F32 else 1e-12
            print(f"{what} {name}{part}: {err:.2e} (gate {gate:.2e})")
            assert err <= gate, (what, name, part, err, gate)


@pytest.mark.parametrize("later", [False, True], ids=["first iteration", "later iteration"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape,n_fft,twosided", STEP_SHAPES, ids=[str(s[0]) for s in STEP_SHAPES])
def test_gla_update_adjoint(shape, n_fft, twosided, dtype, later):
    """(gR, gP, gmag) of S = R - lr P ; Q = S m / (|S| + 1e-16) for cotangents of Q and, in the later form, of S as the next P"""
    lr = 0.5 / 1.5
    S, m, P, _, gmag0, (gQ, gS, _, _), own = _step_inputs(shape, dtype, 11 + shape[1])

    def ref(compute):
        # R in float64 from the float32-representable S and P: the step then reproduces S to an ulp of float64
        Pt = torch.from_numpy(P.astype(cdt(compute))).requires_grad_(True)
        Rt = torch.from_numpy((S.astype(np.complex128) + lr * P.astype(np.complex128)).astype(cdt(compute))).requires_grad_(True)
        mt_ = torch.from_numpy(m.astype(compute)).requires_grad_(True)
        So, Q = gt.gla_update(Rt, Pt, mt_, lr)
        outs, cots = [Q], [torch.from_numpy(gQ.astype(cdt(compute)))]
        if later:
            outs.append(So), cots.append(torch.from_numpy(gS.astype(cdt(compute))))
        return [v.numpy() for v in torch.autograd.grad(outs, [Rt, Pt, mt_], cots)]

    plan = _step_plan(shape, n_fft, twosided, dtype)
    gmag = T(gmag0)
    gR, gP = plan.gla_update_adjoint(T(gQ), T(gS) if later else None, T(S), T(m), lr, gmag)
    _compare_step(f"gla {shape} {np.dtype(dtype).name}", dtype, ("gR", "gP", "gmag"), (gR, gP, gmag - T(gmag0)), ref(F64), ref(dtype), own)


@pytest.mark.parametrize("later", [False, True], ids=["first iteration", "later iteration"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape,n_fft,twosided", STEP_SHAPES, ids=[str(s[0]) for s in STEP_SHAPES])
def test_admm_update_adjoint(shape, n_fft, twosided, dtype, later):
    """(gR, gX, gU, gmag) of the ADMM step for cotangents of Y' and, in the later form, of X' and U'"""
    rho = 0.1
    V, m, X, U, gmag0, (gY, gXn, gUn, _), own = _step_inputs(shape, dtype, 23 + shape[1])

    def ref(compute):
        # V = 2 Z - U - X with Z = (rho (X + U) + R) / (1 + rho): R in float64 from the float32-representable V, X and U
        c = lambda v: v.astype(np.complex128)                                                    # noqa: E731
        R = (c(V) + c(U) + c(X)) / 2 * (1 + rho) - rho * (c(X) + c(U))
        Rt, Xt, Ut = (torch.from_numpy(v.astype(cdt(compute))).requires_grad_(True) for v in (R, X, U))
        mt_ = torch.from_numpy(m.astype(compute)).requires_grad_(True)
        Xn, Un, _, Yn = gt.admm_update(Rt, Xt, Ut, mt_, rho)
        outs, cots = [Yn], [torch.from_numpy(gY.astype(cdt(compute)))]
        if later:
            outs += [Xn, Un]
            cots += [torch.from_numpy(gXn.astype(cdt(compute))), torch.from_numpy(gUn.astype(cdt(compute)))]
        return [v.numpy() for v in torch.autograd.grad(outs, [Rt, Xt, Ut, mt_], cots)]

    plan = _step_plan(shape, n_fft, twosided, dtype)
    gmag = T(gmag0)
    gR, gX, gU = plan.admm_update_adjoint(T(gY), T(gXn) if later else None, T(gUn) if later else None, T(V), T(m), rho, gmag)
    _compare_step(f"admm {shape} {np.dtype(dtype).name}", dtype, ("gR", "gX", "gU", "gmag"), (gR, gX, gU, gmag - T(gmag0)), ref(F64),
                  ref(dtype), own)


# ---- phase_init_adjoint ----------------------------------------------------------------------------------------------------------------
PHASE_CASES = [(128, 32, 9), (128, 32, 64), (128, 32, 65), (128, 32, 130), (128, 32, 200), (1024, 256, 130)]


@functools.lru_cache(maxsize=None)
def _phase_inputs(n_fft, hop, frames):
    """Magnitudes (2, F, T) of the well-conditioned signal, float32-representable, with hand-placed columns, and a complex cotangent"""
    F = n_fft // 2 + 1
    kw = dict(hop_length=hop, window=hann(n_fft, F32))
    mag = np.abs(gt.wellcond_spec(2, n_fft, frames, kw, n_fft + hop + frames)[0]).astype(F32)

    def column(peaks):
        v = np.full(F, 0.2, F32)
        for f, val in peaks.items():
            v[f] = val
        return v

    mag[0, :, 1] = column({1: 1.0, F - 2: 0.9})                                        # peaks at the first and the last bin that can be one
    pairs = column({10: 1.0, 11: 0.5, 12: 0.8, 20: 1.0, 21: 0.4, 22: 0.9, 23: 0.3, 24: 0.7})
    mag[0, :, 2] = pairs                                                               # peaks at g, g + 2 (and g + 4): bin g + 1 is the upper one's
    mag[1, :, 3] = column({30: 1.0, 31: 1.0, 40: 0.6})                                 # a plateau is no peak
    mag[1, :, 4] = 0.3                                                                 # a column without peaks
    mag[1, :, frames - 1] = pairs                                                      # ... and in the last chunk of frames
    rng = np.random.default_rng(frames)
    gC = (rng.standard_normal(mag.shape) + 1j * rng.standard_normal(mag.shape)).astype(np.complex64)
    gmag0 = rng.standard_normal(mag.shape).astype(F32)
    return mag, gC, gmag0


def _phase_plan(n_fft, hop, frames, dtype):
    a = args_helper(torch.empty(1, n_fft // 2 + 1, 1, dtype=tdt(dtype)), hop_length=hop, window=torch.from_numpy(hann(n_fft, dtype)))
    return Plan(a, 2, frames, tdt(dtype), DEV), mt._setup(n_fft // 2 + 1, torch.float64, dict(hop_length=hop, window=hann(n_fft, F64)))[0]


@pytest.mark.parametrize("n_fft,hop,frames", PHASE_CASES)
def test_phase_init_adjoint_float64(n_fft, hop, frames):
    """Against autograd on tests/_agla_torch.py::phase_init times a random complex cotangent, 1e-10; accumulated into `gmag`.  65 and
    130 frames are the ones a wrong carry between the 64-lane chunks of k_phase_init_adjoint_rows fails."""
    mag, gC, gmag0 = (v.astype(np.result_type(v.dtype, F64)) for v in _phase_inputs(n_fft, hop, frames))
    plan, a = _phase_plan(n_fft, hop, frames, F64)
    mt_ = torch.from_numpy(mag).requires_grad_(True)
    C = at.phase_init(mt_, a)
    (C.real * torch.from_numpy(gC.real.copy()) + C.imag * torch.from_numpy(gC.imag.copy())).sum().backward()
    gmag = T(gmag0)
    plan.phase_init_adjoint(T(mag), T(gC), gmag)
    err = rel_l2(N(gmag) - gmag0, mt_.grad.numpy())
    print(f"phase_init_adjoint float64 {n_fft}/{hop} x {frames}: {err:.2e}")
    assert err <= 1e-10, err


@pytest.mark.parametrize("n_fft,hop,frames", PHASE_CASES)
def test_phase_init_float64_sums_in_the_reference_order(n_fft, hop, frames):
    """The phase is a cumulative sum of up to 1e5 rad here, whose ulp is 1.5e-11: another order of summation
    moves the start by that much and the gradients of griffin_lim / ADMM by 1e-9 and more.  Summed one frame after the other, as
    torch.cumsum does on the CPU, the phase is the reference's to the bit and what is left is an ulp or two of sin and cos: 1e-14
    is thirty times that and a thousand times less than an ulp of the phase."""
    mag = _phase_inputs(n_fft, hop, frames)[0].astype(F64)
    plan, a = _phase_plan(n_fft, hop, frames, F64)
    err = rel_l2(N(plan.phase_init(T(mag))), at.phase_init(torch.from_numpy(mag), a).numpy())
    print(f"phase_init float64 {n_fft}/{hop} x {frames}: {err:.2e}")
    assert err <= 1e-14, err


@pytest.mark.parametrize("n_fft,hop,frames", PHASE_CASES)
def test_phase_init_adjoint_float32(n_fft, hop, frames):
    """The kernel recomputes phi in float32 from sums of thousands of radians, so e^{i phi} comes from the device's own forward result
    C0 = phase_init(mag): gm = Re(conj(C0 / m) gC) + d/dm <reverse cumsum over time of Re(conj(i C0) gC), phase advance(m)> in float64,
    against the same formulas in float32 on the CPU as the yardstick."""
    mag, gC, gmag0 = _phase_inputs(n_fft, hop, frames)
    plan, a = _phase_plan(n_fft, hop, frames, F32)
    C0 = N(plan.phase_init(T(mag)))

    def formulas(compute):
        m, c0, g = (torch.from_numpy(v.astype(np.result_type(v.dtype, compute))) for v in (mag, C0, gC))
        unit = c0 / m
        direct = unit.real * g.real + unit.imag * g.imag
        gphi = c0.real * g.imag - c0.imag * g.real                                     # Re(conj(i C0) gC)
        gomega = torch.flip(torch.cumsum(torch.flip(gphi, [2]), 2), [2])
        ml = m.clone().requires_grad_(True)
        (at.phase_advance(ml, a) * gomega).sum().backward()
        return (direct + ml.grad).numpy()

    ref = formulas(F64)
    gate = max(2e-5, 6 * rel_l2(formulas(F32), ref))
    gmag = T(gmag0)
    plan.phase_init_adjoint(T(mag), T(gC), gmag)
    out = N(gmag) - gmag0
    assert np.isfinite(out).all()
    err = rel_l2(out, ref)
    print(f"phase_init_adjoint float32 {n_fft}/{hop} x {frames}: {err:.2e} (gate {gate:.2e})")
    assert err <= gate, (err, gate)
