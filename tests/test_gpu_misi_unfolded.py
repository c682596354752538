"""`misi_unfolded` on the device: its gradients against autograd on the torch restatement of the MISI oracle
(tests/_misi_torch.py) and against central differences of the inference path, the two new entry points
(`specinv_misi_mix_adjoint`, `specinv_misi_step_adjoint`; csrc/kernels_misi_adjoint.h) against NumPy and against the adjoint
building blocks they replace, and the layer's properties.  Inputs as tests/test_gpu_misi.py builds them.  Needs an MI355X:
`-m gpu`."""
import functools

import numpy as np
import pytest
import torch

import _misi_torch as mt
from _util import hann, rel_l2
from test_gpu_misi import _case

pytestmark = pytest.mark.gpu

import spectrogram_inversion_amd as si                                    # noqa: E402
from spectrogram_inversion_amd import _lib                                 # noqa: E402
from spectrogram_inversion_amd.plan import Plan, args_helper, clear_plan_cache, get_plan   # noqa: E402

DEV = torch.device("cuda", 0)
N_ITER = 3
TDT = {np.float32: torch.float32, np.float64: torch.float64}


def N(t):
    return t.detach().cpu().numpy()


def T_(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# name: n_fft, hop, frames, B, K, extra stft kwargs (test_gpu_misi._case's: `rect` takes the rectangular window)
CONFIGS = {
    "128/32": (128, 32, 10, 2, 3, {}),
    "64/16 two-sided normalized": (64, 16, 11, 2, 2, dict(onesided=False, normalized=True)),
    "64/20 circular": (64, 20, 11, 2, 3, dict(pad_mode="circular")),
    "512/300/100": (512, 100, 9, 2, 2, dict(win_length=300)),
    "rect default hop": (128, None, 12, 2, 4, dict(rect=True)),
    "1024/256": (1024, 256, 16, 2, 2, {}),                # with the chunked_kernel fixture: k_fused4, two chunks, chunk tails
    "400/160": (400, 160, 12, 2, 3, {}),                  # k_wave_iter
}


@functools.lru_cache(maxsize=None)
def _inputs(name, dtype, magnitude_start):
    """(specs, mix, w, L, kw) as NumPy arrays: `specs` complex or its modulus, `w` the fixed random weights of the loss"""
    n_fft, hop, frames, B, K, extra = CONFIGS[name]
    start, mix, L, kw = _case(n_fft, hop, frames, B, K, extra, dtype, seed=n_fft + frames + K)
    if hop is None:
        del kw["hop_length"]
    w = np.random.default_rng(7).standard_normal((B, K, L)).astype(dtype)
    return (np.abs(start) if magnitude_start else start), mix, w, L, kw


@functools.lru_cache(maxsize=None)
def _reference(name, dtype, magnitude_start):
    """Autograd on the restatement, on the CPU in `dtype`: (grad specs, grad mix), computed once per case."""
    specs, mix, w, L, kw = _inputs(name, dtype, magnitude_start)
    s = torch.from_numpy(specs).requires_grad_(True)
    m = torch.from_numpy(mix).requires_grad_(True)
    (mt.misi(s, m, N_ITER, **kw) * torch.from_numpy(w)).sum().backward()
    return s.grad.numpy(), m.grad.numpy()


def _tkw(kw):
    return dict(kw, window=torch.from_numpy(kw["window"]))


def _device_grads(name, dtype, magnitude_start):
    specs, mix, w, L, kw = _inputs(name, dtype, magnitude_start)
    s, m = T_(specs).requires_grad_(True), T_(mix).requires_grad_(True)
    y = si.misi_unfolded(s, m, N_ITER, **_tkw(kw))
    assert y.requires_grad and y.shape == w.shape
    with torch.no_grad():
        # the output under grad is the inference path's, bit for bit
        assert torch.equal(y, si.misi(s, m, max_iter=N_ITER, tol=0, verbose=False, **_tkw(kw)))
    (y * T_(w)).sum().backward()
    assert s.grad.shape == s.shape and s.grad.dtype == s.dtype and m.grad.shape == m.shape
    assert not N(m.grad)[:, L:].any()                                # samples beyond L: exactly zero
    return N(s.grad), N(m.grad)


F64 = ["128/32", "64/16 two-sided normalized", "64/20 circular", "512/300/100", "rect default hop"]


@pytest.mark.parametrize("magnitude_start", [False, True], ids=["complex", "magnitude"])
@pytest.mark.parametrize("name", F64)
def test_float64_gradients_match_autograd_on_the_restatement(name, magnitude_start):
    """rel-L2 <= 1e-9, tests/test_gpu_autograd.py's float64 gate."""
    clear_plan_cache()
    gs, gm = _device_grads(name, np.float64, magnitude_start)
    rs, rm = _reference(name, np.float64, magnitude_start)
    es, em = rel_l2(gs, rs), rel_l2(gm, rm)
    print(f"{name} float64: grad specs {es:.3e}  grad mixture {em:.3e}")
    assert es <= 1e-9 and em <= 1e-9, (es, em)


def _float32(name, magnitude_start, kernel):
    """The gate is the larger of 2e-4 (the float32 gradient gate of tests/test_gpu_autograd.py) and 6 times the restatement's own
    float32-against-float64 gradient error on the case (the margin rule of DESIGN 3.12): the device cannot be asked to be closer
    to the float64 gradient than float32 arithmetic on the CPU gets."""
    clear_plan_cache()
    specs, mix, w, L, kw = _inputs(name, np.float32, magnitude_start)
    c64 = lambda a: a.astype(np.complex128 if np.iscomplexobj(a) else np.float64)        # noqa: E731
    s64, m64 = torch.from_numpy(c64(specs)).requires_grad_(True), torch.from_numpy(c64(mix)).requires_grad_(True)
    (mt.misi(s64, m64, N_ITER, **dict(kw, window=c64(kw["window"]))) * torch.from_numpy(c64(w))).sum().backward()
    rs, rm = s64.grad.numpy(), m64.grad.numpy()
    fs, fm = _reference(name, np.float32, magnitude_start)
    own_s, own_m = rel_l2(fs, rs), rel_l2(fm, rm)
    gs, gm = _device_grads(name, np.float32, magnitude_start)
    n_fft, hop, frames, B, K, extra = CONFIGS[name]
    geo = get_plan(args_helper(T_(specs).reshape(B * K, -1, frames), **_tkw(kw)), B * K, frames, torch.float32, DEV).launch_geometry
    assert geo["kernel"] == kernel, geo
    es, em = rel_l2(gs, rs), rel_l2(gm, rm)
    print(f"{name} float32 ({geo['kernel']}, {geo['chunks']} chunks): grad specs {es:.3e} (restatement {own_s:.3e})  "
          f"grad mixture {em:.3e} (restatement {own_m:.3e})")
    assert es <= max(2e-4, 6 * own_s) and em <= max(2e-4, 6 * own_m), (es, own_s, em, own_m)
    return geo


@pytest.mark.parametrize("magnitude_start", [False, True], ids=["complex", "magnitude"])
@pytest.mark.parametrize("name,kernel", [("128/32", "k_wave_iter"), ("400/160", "k_wave_iter")])
def test_float32_gradients(name, kernel, magnitude_start):
    _float32(name, magnitude_start, kernel)


@pytest.mark.parametrize("magnitude_start", [False, True], ids=["complex", "magnitude"])
def test_float32_gradients_fused_forward_with_chunk_tails(chunked_kernel, magnitude_start):
    assert _float32("1024/256", magnitude_start, "k_fused4")["chunks"] == 2


@pytest.mark.parametrize("wrt", ["specs", "mixture"])
@pytest.mark.parametrize("magnitude_start", [False, True], ids=["complex", "magnitude"])
def test_gradient_matches_a_central_difference_of_the_inference_path(magnitude_start, wrt):
    """Independent of the restatement: float64, d/dt of sum(w * misi(...)) along a random direction at h = 1e-6 against
    <grad, direction>.  Relative 1e-6: the truncation is O(h^2), the rounding about 1e-10; a wrong formula is off by O(1).
    The direction has unit length, so that h is the step: along standard-normal draws (length 25 for the mixture, 60 - 90 for
    specs) the step is that many h, and the mixture-phase start, whose third derivative grows like 1 / |STFT(mix)|^3 at the weak
    bins of a 0.1-sigma mixture, then leaves 5e-5 of truncation - on the CPU restatement to the same twelve digits, and 100
    times less at h = 1e-7."""
    clear_plan_cache()
    specs, mix, w, L, kw = _inputs("128/32", np.float64, magnitude_start)
    gs, gm = _device_grads("128/32", np.float64, magnitude_start)
    rng = np.random.default_rng(11)
    if wrt == "specs":
        d = rng.standard_normal(specs.shape) + (1j * rng.standard_normal(specs.shape) if np.iscomplexobj(specs) else 0)
        d /= np.linalg.norm(d)
        ip = float((np.conj(gs) * d).real.sum())
    else:
        d = rng.standard_normal(mix.shape)
        d /= np.linalg.norm(d)
        ip = float((gm * d).sum())
    h = 1e-6

    def f(t):
        s, m = (specs + t * d, mix) if wrt == "specs" else (specs, mix + t * d)
        y = si.misi(T_(s), T_(m), max_iter=N_ITER, tol=0, verbose=False, **_tkw(kw))
        return float((N(y) * w).sum())

    fd = (f(h) - f(-h)) / (2 * h)
    print(f"d/d{wrt}: central difference {fd:.12e}  <grad, direction> {ip:.12e}  relative {abs(fd - ip) / abs(fd):.3e}")
    assert abs(fd - ip) <= 1e-6 * abs(fd), (fd, ip)


def _small_plan(K, hop, dtype, n_mix=2, frames=8, n_fft=128, **extra):
    kw = dict(hop_length=hop, window=torch.from_numpy(hann(n_fft, dtype)), **extra)
    F = n_fft // 2 + 1 if extra.get("onesided", True) else n_fft
    cd = torch.complex64 if dtype == np.float32 else torch.complex128
    return Plan(args_helper(torch.empty((1, F, 1), dtype=cd), **kw), n_mix * K, frames, TDT[dtype], DEV)


@pytest.mark.parametrize("hop", [32, 34, 33])             # L = 7 hop: 224 = 0 (mod 4), 238 = 2 (mod 4), 231 odd
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_every_arm_of_the_mix_adjoint_kernel(dtype, hop):
    """K = 2, 3, 4 in registers and the loop (5), 16- / 8- / 4-byte accesses (float64: 16 / 8), against NumPy in float64.
    The bound is the rounding of the K additions behind c and of adding it to gmix, g_k - c rounds once more:
    (K + 2) eps max|g| <= 4 K eps max|g| (tests/test_gpu_misi.py's bound), with |gmix| <= max|g| on entry."""
    rng = np.random.default_rng(hop)
    eps = np.finfo(dtype).eps
    for K in (2, 3, 4, 5):
        p = _small_plan(K, hop, dtype)
        L = p.length
        assert L == 7 * hop
        g0 = rng.standard_normal((2, K, L)).astype(dtype)
        m0 = (0.5 * rng.uniform(-1, 1, (2, L))).astype(dtype)
        g, gmix = T_(g0.reshape(2 * K, L)), T_(m0)
        p.misi_mix_adjoint(K, g, gmix)
        c = g0.astype(np.float64).sum(1) / K
        bound = 4 * K * eps * np.abs(g0).max()
        eg = np.abs(N(g).reshape(2, K, L) - (g0.astype(np.float64) - c[:, None])).max()
        em = np.abs(N(gmix) - (m0.astype(np.float64) + c)).max()
        print(f"K {K} L {L} {np.dtype(dtype).name}: g {eg:.3e} gmix {em:.3e} bound {bound:.3e}")
        assert eg <= bound and em <= bound, (K, eg, em, bound)


STEP = [(np.float64, 32, {}, 1e-12), (np.float32, 32, {}, 2e-5), (np.float64, 34, dict(onesided=False, normalized=True), 1e-12),
        (np.float64, 33, dict(pad_mode="circular"), 1e-12), (np.float32, 64, dict(n_fft=256, pad_mode="replicate"), 2e-5)]


@pytest.mark.parametrize("dtype,hop,extra,tol", STEP)
def test_step_adjoint_equals_the_block_composition(dtype, hop, extra, tol):
    """One specinv_misi_step_adjoint call against istft_adjoint o gla_update_adjoint(lr = 0) o stft_adjoint with the coupling
    adjoint in torch, on the same x_prev: the adjoint-identity gates of tests/test_gpu_autograd.py."""
    K = 3
    p = _small_plan(K, hop, dtype, **extra)
    rng = np.random.default_rng(hop)
    L, shape = p.length, (p.batch, p.n_freq, p.n_frames)
    x_prev = T_(rng.standard_normal((p.batch, L)).astype(dtype))
    mag = T_((rng.random(shape) + 0.05).astype(dtype))
    g0 = T_(rng.standard_normal((p.batch, L)).astype(dtype))
    gmix0 = T_(rng.standard_normal((2, L)).astype(dtype))
    gm0 = T_(rng.standard_normal(shape).astype(dtype))
    # the blocks
    c = g0.reshape(2, K, L).sum(1) / K
    gm_ref = gm0.clone()
    gq = p.istft_adjoint((g0.reshape(2, K, L) - c[:, None]).reshape(p.batch, L).contiguous())
    gr, _ = p.gla_update_adjoint(gq, None, p.stft(x_prev), mag, 0.0, gm_ref)
    gx_ref = p.stft_adjoint(gr, L)
    # one call, frame-major magnitudes
    g, gmix = g0.clone(), gmix0.clone()
    gm_fm = gm0.transpose(1, 2).contiguous()
    p.misi_step_adjoint(K, x_prev, mag.transpose(1, 2).contiguous(), g, gmix, gm_fm)
    errs = (rel_l2(N(g), N(gx_ref)), rel_l2(N(gm_fm.transpose(1, 2)), N(gm_ref)), rel_l2(N(gmix), N(gmix0 + c)))
    print(f"{np.dtype(dtype).name} hop {hop} {extra}: g {errs[0]:.3e} gmag {errs[1]:.3e} gmix {errs[2]:.3e}")
    assert max(errs) <= tol, errs


def test_mix_adjoint_is_the_adjoint_of_the_coupling_step():
    """<J v, g> = <v, J^T g> for J (x, mix) = x_k + (mix - sum_j x_j) / K, and the argument errors that need a plan."""
    K = 4
    p = _small_plan(K, 33, np.float64)
    rng = np.random.default_rng(5)
    L = p.length
    vx, vmix = rng.standard_normal((2, K, L)), rng.standard_normal((2, L))
    g0 = rng.standard_normal((2, K, L))
    jv = vx + ((vmix - vx.sum(1)) / K)[:, None]
    g, gmix = T_(g0.reshape(2 * K, L)), torch.zeros((2, L), dtype=torch.float64, device=DEV)
    p.misi_mix_adjoint(K, g, gmix)
    lhs, rhs = (jv * g0).sum(), (vx * N(g).reshape(2, K, L)).sum() + (vmix * N(gmix)).sum()
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs), (lhs, rhs)
    before = N(g).copy()
    with pytest.raises(AssertionError, match="multiple"):                 # 8 items are not groups of 3
        p.misi_mix_adjoint(3, g, gmix)
    x, fm = torch.zeros_like(g), torch.zeros((p.batch, p.n_frames, p.n_freq), dtype=torch.float64, device=DEV)
    with pytest.raises(AssertionError, match="multiple"):
        p.misi_step_adjoint(3, x, fm, g, gmix, fm.clone())
    assert p.lib.specinv_misi_mix_adjoint(p._h, 0, g.data_ptr(), gmix.data_ptr()) == _lib.EINVAL
    assert np.array_equal(N(g), before)                                   # refused before anything ran


def _layer_case(dtype=np.float32):
    specs, mix, w, L, kw = _inputs("128/32", dtype, True)
    return specs, mix, w, L, _tkw(kw)


def test_backward_twice_gives_identical_gradients():
    specs, mix, w, L, kw = _layer_case()
    s, m = T_(specs).requires_grad_(True), T_(mix).requires_grad_(True)
    loss = (si.misi_unfolded(s, m, N_ITER, **kw) * T_(w)).sum()
    first = torch.autograd.grad(loss, (s, m), retain_graph=True)
    second = torch.autograd.grad(loss, (s, m))
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    assert all(torch.isfinite(a).all() and a.abs().max() > 0 for a in first)


def test_no_grad_requested_is_the_inference_path():
    specs, mix, w, L, kw = _layer_case()
    ref = si.misi(T_(specs), T_(mix), max_iter=N_ITER, tol=0, verbose=False, **kw)
    y = si.misi_unfolded(T_(specs), T_(mix), N_ITER, **kw)
    assert not y.requires_grad and torch.equal(y, ref)
    with torch.no_grad():
        y2 = si.misi_unfolded(T_(specs).requires_grad_(True), T_(mix).requires_grad_(True), N_ITER, **kw)
    assert not y2.requires_grad and torch.equal(y2, ref)
    # one input alone requiring grad: the other gets none
    s = T_(specs).requires_grad_(True)
    si.misi_unfolded(s, T_(mix), N_ITER, **kw).sum().backward()
    assert s.grad is not None and torch.isfinite(s.grad).all()
    m = T_(mix).requires_grad_(True)
    si.misi_unfolded(T_(specs), m, N_ITER, **kw).sum().backward()
    assert m.grad is not None and torch.isfinite(m.grad).all() and m.grad.abs().max() > 0


def test_a_backward_leaves_the_cached_plan_as_it_was():
    clear_plan_cache()
    specs, mix, w, L, kw = _layer_case()
    before = si.misi(T_(specs), T_(mix), max_iter=5, tol=0, verbose=False, **kw)
    s = T_(specs).requires_grad_(True)
    y = si.misi_unfolded(s, T_(mix), N_ITER, **kw)
    running = si.misi(T_(specs), T_(mix), max_iter=5, tol=0, verbose=False, **kw)     # the same plan, between forward and backward
    (y * T_(w)).sum().backward()
    after = si.misi(T_(specs), T_(mix), max_iter=5, tol=0, verbose=False, **kw)
    assert torch.equal(before, running) and torch.equal(before, after)
    g = s.grad.clone()
    s.grad = None
    (si.misi_unfolded(s, T_(mix), N_ITER, **kw) * T_(w)).sum().backward()
    assert torch.equal(g, s.grad)


def test_cpu_and_narrow_inputs_get_gradients_of_their_own_kind():
    specs, mix, w, L, kw = _layer_case()
    s, m = torch.from_numpy(specs).requires_grad_(True), torch.from_numpy(mix).requires_grad_(True)
    y = si.misi_unfolded(s, m, N_ITER, **kw)
    assert y.device.type == "cpu" and y.shape == w.shape
    (y * torch.from_numpy(w)).sum().backward()
    assert s.grad.device.type == "cpu" and m.grad.device.type == "cpu"
    dev_s, dev_m = T_(specs).requires_grad_(True), T_(mix).requires_grad_(True)
    (si.misi_unfolded(dev_s, dev_m, N_ITER, **kw) * T_(w)).sum().backward()
    assert torch.equal(s.grad, dev_s.grad.cpu()) and torch.equal(m.grad, dev_m.grad.cpu())
    s1, m1 = torch.from_numpy(specs[0]).requires_grad_(True), torch.from_numpy(mix[0]).requires_grad_(True)
    y1 = si.misi_unfolded(s1, m1, N_ITER, **kw)                           # (K, F, T) with a (L_m,) mixture
    assert y1.shape == w.shape[1:]
    y1.sum().backward()
    assert s1.grad.shape == s1.shape and m1.grad.shape == m1.shape and not m1.grad[L:].any()
    hs = T_(specs).to(torch.bfloat16).requires_grad_(True)
    hm = T_(mix).to(torch.bfloat16).requires_grad_(True)
    hy = si.misi_unfolded(hs, hm, N_ITER, **kw)
    assert hy.dtype == torch.bfloat16
    hy.float().sum().backward()
    assert hs.grad.dtype == torch.bfloat16 and hm.grad.dtype == torch.bfloat16 and torch.isfinite(hs.grad.float()).all()
