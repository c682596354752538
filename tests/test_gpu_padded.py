"""Every forward kernel family over zero-padded batches, silence and quiet audio (tests/_padded.py) against the oracle: frames whose
target and estimate are both exactly 0 - the projection S m / (|S| + 1e-16) at S = 0, m = 0 - items that are silent throughout, and
passages at 2^-20 of the rest next to full-scale ones.  Each family guards that point in its own way (the squared floor of the
float32 wave-level chain, the hypot + division fallback of the coverage kernels, the selects of the L-BFGS objective and of
phase_init); one 0 x inf there puts a NaN into a frame, and the overlap-add carries it through the item.

Per case: (a) the finite mask is the oracle's; (b) dead samples - covered by silent frames alone - and the all-silent item are
exactly 0.0 wherever tests/test_padded_host.py established that for the reference; (c) the per-item rel-L2 against the float32
oracle is within the suite's gate, max(floor, 6 x the oracle's own float32-against-float64 figure); (d) so is the largest error of a
hop-length block, relative to the item's RMS block, which a whole-item norm would hide next to a silence boundary; (e) the sums of
an evaluating last iteration agree with the oracle's to 1e-5.  Needs an MI355X: `-m gpu`."""
import math

import numpy as np
import pytest
import torch

import _padded as pd
from _util import rel_l2

pytestmark = pytest.mark.gpu

import spectrogram_inversion_amd as si                                     # noqa: E402
from spectrogram_inversion_amd.constrained import _begin as cgla_begin      # noqa: E402
from spectrogram_inversion_amd.metrics import _from_sums                    # noqa: E402
from spectrogram_inversion_amd.plan import Plan, args_helper, clear_plan_cache   # noqa: E402

DEV = torch.device("cuda", 0)
f32, f64 = np.float32, np.float64


def N(t):
    return t.detach().cpu().numpy()


def T_(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _tkw(kw):
    return dict(kw, window=torch.from_numpy(np.array(kw["window"])))


def _make_plan(name, batch, monkeypatch):
    """the plan of a case on its route (see _padded.CASES); the environment is read when the plan is set up"""
    n_fft, hop, frames, extra, dtype, route = pd.CASES[name]
    chunk = pd.GEOMETRY[name][3]
    if route == "chunked":
        monkeypatch.setenv("SPECINV_SMALL_FRAMES", "0")
    if route == "generic":
        monkeypatch.setenv("SPECINV_GENERIC_WAVE", "0")
    if chunk is not None:                                        # as make_plan(..., chunk=...) of tests/test_gpu_fast.py
        monkeypatch.setenv("SPECINV_FAST_CHUNK", str(chunk))
    if name.endswith("skewed"):
        monkeypatch.setenv("SPECINV_TD_SKEW", "4")
    c = pd.case(name)
    F = c.mag.shape[1]
    probe = torch.empty((1, F, 1), dtype=torch.complex64 if dtype == f32 else torch.complex128)
    p = Plan(args_helper(probe, **_tkw(c.kw)), batch, frames, torch.float32 if dtype == f32 else torch.float64, DEV)
    if route == "generic":
        p.force_generic(True)
    return p


def _run(p, name, method, c, keep=False):
    """`method` on the plan, the last iteration evaluating where the method has an evaluation of its own: (y, sums or None)"""
    kind, iters, prm = pd.method_of(name, method)
    if kind == "gla":
        p.keep_state(keep)
        if method == "gla_mag":
            p.gla_init(None, T_(c.mag), prm)                     # phase_init on the device (k_phase_init_pairs on the fast paths)
        else:
            p.gla_init(T_(c.start), None, prm)
    elif kind == "admm":
        p.admm_init(T_(c.start), None, prm)
    elif kind == "agla":
        p.agla_init(T_(c.start), None, prm[0], prm[0] if prm[1] is None else prm[1], prm[2])
    elif kind == "misi":
        p.misi_init(T_(c.start[:2]), None, T_((c.x[0] + c.x[1])[None]), 2)
    elif kind == "cgla":
        K, M, xk, W = pd.cgla_constraint(c)
        cgla_begin(p, T_(c.start), T_(K), T_(M), T_(xk), T_(W), prm[0], prm[1], prm[2])
        p.agla_iterate(iters)
        return N(p.wave()), None
    p.iterate(iters - 1)
    sums = p.iterate(1, eval_last=True)
    return N(p.wave()), sums


def _check(y, name, method, dtype, quiet_pow=-20, scale=1.0, blocks=True):
    """(a) - (d) of the module's docstring; returns the per-item (rel-L2, block measure)"""
    c = pd.case(name, None, quiet_pow, scale)
    items = pd.items_of(method)
    ref, _ = pd.reference(name, method, dtype, quiet_pow, scale)
    assert y.shape == ref.shape and y.dtype == ref.dtype
    assert np.array_equal(np.isfinite(y), np.isfinite(ref)), f"{(~np.isfinite(y)).sum(1)} samples per item are not finite"    # (a)
    if 3 in items:                                                                                                           # (b)
        assert not y[3].any(), "the all-silent item"
    if method in pd.DEAD_ZERO:
        bad = (y != 0) & c.dead[items]
        assert not bad.any(), f"{bad.sum(1)} dead samples per item are not 0.0"
    hop = pd.CASES[name][1]
    e, blk = pd.item_rel_l2(y, ref), pd.block_measure(y, ref, hop)
    gate, bgate = pd.gates(name, method, dtype, quiet_pow, scale)
    print(f"{name} {method} 2^{quiet_pow} x{scale:g}: rel_l2 {e} gate {gate}; block {blk} gate {bgate}")
    live = [i for i, b in enumerate(items) if b != 3]
    assert (e[live] <= gate[live]).all(), (e, gate)                                                                           # (c)
    if blocks:
        assert (blk[live] <= bgate[live]).all(), (blk, bgate)                                                                 # (d)
    return e, blk


def _check_sums(sums, name, method, dtype):
    """(e): sum (|S| - m)^2 / count and sum m^2 of the last iteration against the oracle's float64 accumulation"""
    _, osums = pd.reference(name, method, dtype)
    print(f"sums {sums} oracle mse {osums[0]:.9e} sum m^2 {osums[1]:.9e}")
    np.testing.assert_allclose([sums[0] / sums[3], sums[2]], osums, rtol=1e-5)


def _geometry(p, name, method, keep=False):
    gla_kernel, other_kernel, chunks, _ = pd.GEOMETRY[name]
    geo = p.launch_geometry
    want = gla_kernel if pd.METHODS[method][0] == "gla" and not keep else other_kernel
    assert geo["kernel"] == want and geo["chunks"] >= chunks, (want, chunks, geo)
    if pd.CASES[name][5] == "chunked":
        assert p.fast_path
    if name in pd.OVERLAP_ADD:
        assert geo["overlap_add"] == pd.OVERLAP_ADD[name] and geo["chunks"] >= 2, geo
    return geo


@pytest.mark.parametrize("name,method", pd.CASE_METHODS)
def test_padded_batch_matches_the_oracle(monkeypatch, name, method):
    dtype = pd.CASES[name][4]
    c = pd.case(name)
    p = _make_plan(name, len(pd.items_of(method)), monkeypatch)
    y, sums = _run(p, name, method, c)
    _geometry(p, name, method)
    _check(y, name, method, dtype)
    if sums is not None and method != "gla_mag":                 # (a start from the magnitudes carries phase_init's 1e-4 ... 1e-3)
        _check_sums(sums, name, method, dtype)


@pytest.mark.parametrize("name", ["1024/256", "2048/512"])
def test_griffin_lim_on_the_spectral_state_kernel(monkeypatch, name):
    """keep_state: Griffin-Lim iterates on pre_spec itself (k_fused4) instead of carrying the momentum as a signal"""
    c = pd.case(name)
    p = _make_plan(name, pd.BATCH, monkeypatch)
    y, sums = _run(p, name, "gla", c, keep=True)
    _geometry(p, name, "gla", keep=True)
    _check(y, name, "gla", f32)
    _check_sums(sums, name, "gla", f32)
    P = N(p.state_spec(0))
    assert np.isfinite(P).all() and not P[3].any()


@pytest.mark.parametrize("method", pd.SCALE_METHODS)
@pytest.mark.parametrize("name,quiet_pow,scale", pd.SCALE_CASES)
def test_int16_range_and_very_quiet_audio(monkeypatch, name, quiet_pow, scale, method):
    """The whole batch times 2^15 and 2^-20: the gates are those of the unscaled case, against the oracle on the scaled input.  (At
    2^-20 the bins of the quiet stretch, 2^-40 of full scale, are below the |S| = 3e-9 from which the float32 wave-level chain
    differs from the reference by design; at 2^-40 of the item they are far below what either gate resolves.)"""
    c = pd.case(name, None, quiet_pow, scale)
    p = _make_plan(name, pd.BATCH, monkeypatch)
    y, _ = _run(p, name, method, c)
    _geometry(p, name, method)
    _check(y, name, method, f32, quiet_pow, scale)


@pytest.mark.parametrize("name,quiet_pow,scale", pd.DEEP_CASES)
def test_a_quiet_stretch_below_the_floor_of_the_fast_chain(monkeypatch, name, quiet_pow, scale):
    """A stretch at 2^-40: |S| there is below 3e-9, where the float32 wave-level chain (squared floor 1e-32) differs from the
    reference's additive 1e-16 by design (fast_core.h) and the coverage kernels do not.  Asserted: the finite mask, the whole-item
    rel-L2, and that the stretch comes back as quiet as the oracle's - its peak within a factor of 2.  The coverage kernels take the
    reference's own operations there (proj_inv's fallback): on them the stretch alone is held to the suite's gate, max(2e-5, 6 x
    the oracle's float32-against-float64 figure on the stretch) - the squared floor in its place is 5e-5 off (CPU emulation)."""
    c = pd.case(name, None, quiet_pow, scale)
    p = _make_plan(name, pd.BATCH, monkeypatch)
    y, _ = _run(p, name, "gla", c)
    _geometry(p, name, "gla")
    _check(y, name, "gla", f32, quiet_pow, scale, blocks=False)
    ref, _ = pd.reference(name, "gla", f32, quiet_pow, scale)
    n_fft = pd.CASES[name][0]
    inner = pd.stretch_of(c, n_fft)                                # the samples that frames inside the stretch alone cover
    peak, opeak = np.abs(y[2, inner]).max(), np.abs(ref[2, inner]).max()
    print(f"peak of the quiet stretch {peak:.3e} oracle {opeak:.3e}, of the item {np.abs(ref[2]).max():.3e}")
    assert 0 < opeak < 2.0 ** -30 * np.abs(ref[2]).max() and 0.5 * opeak <= peak <= 2 * opeak
    if pd.CASES[name][5] != "chunked":
        e, noise = rel_l2(y[2, inner], ref[2, inner]), pd.stretch_noise(name, "gla", quiet_pow, scale)
        print(f"rel_l2 on the stretch {e:.3e}, the oracle's float32 against float64 there {noise:.3e}")
        assert e <= max(2e-5, 6 * noise), (e, noise)


@pytest.mark.parametrize("name", ["1024/256", "512/77", "512/128 semi", "256/77", "512/128 f64", "256/77 generic"])
def test_an_all_silent_batch_runs_to_max_iter_and_returns_zeros(monkeypatch, name):
    """tol = 1e-6 on zero magnitudes: the loss of every evaluation is 0, `init_loss` stays unset and the stop rule never fires - the
    reference runs to max_iter (tests/test_padded_host.py) and reports the metric of zero sums."""
    c = pd.case(name)
    p = _make_plan(name, pd.BATCH, monkeypatch)
    mag = torch.zeros(c.mag.shape, dtype=p.dtype, device=DEV)
    for method in ("gla", "admm", "agla"):
        if method == "agla":
            p.agla_init(None, mag, 0.99, 0.99, 1.0)
        else:
            getattr(p, method + "_init")(None, mag, 0.99 if method == "gla" else 0.5)
        done, evals = p.run(12, 2, 1e-6, "sc")
        assert done == 12 and [e[0] for e in evals] == [1, 3, 5, 7, 9, 11], (method, done, evals)
        want = _from_sums("SC", [0.0, 0.0, 0.0, float(mag.numel())])
        assert math.isnan(want) and all(math.isnan(m) and loss == 0.0 for _, m, loss in evals), (method, evals)
        assert not N(p.wave()).any(), method
    clear_plan_cache()
    y = si.griffin_lim(mag, max_iter=12, tol=1e-6, eva_iter=2, verbose=False, **_tkw(c.kw))
    assert tuple(y.shape) == (pd.BATCH, c.length) and not N(y).any()
    clear_plan_cache()


# ---- RTISI_LA ------------------------------------------------------------------------------------------------------------------------
def _rtisi(name, asym, c=None):
    n_fft, hop, frames, dtype, la = pd.RTISI_CASES[name]
    c = c or pd.case(name)
    return si.RTISI_LA(T_(c.mag), look_ahead=la, asymmetric_window=asym, max_iter=pd.RTISI_ITERS, alpha=pd.RTISI_ALPHA,
                       verbose=False, **_tkw(c.kw))


@pytest.mark.parametrize("asym", [True, False], ids=["asymmetric", "symmetric"])
@pytest.mark.parametrize("name", list(pd.RTISI_CASES))
def test_rtisi_on_a_padded_batch(name, asym):
    """Exact zeros under both window forms: dead samples, the all-silent item, and the item with leading silence - the recursion
    never leaves S = 0 there, in the reference as here.  The comparison is on the item with trailing silence under the asymmetric
    window, at test_gpu_rtisi.py's rule, max(1e-4, 3 x the oracle's own float32-against-float64 figure)."""
    clear_plan_cache()
    n_fft, hop, frames, dtype, la = pd.RTISI_CASES[name]
    c = pd.case(name)
    y = N(_rtisi(name, asym))
    ref = pd.rtisi_reference(name, asym, dtype)
    assert y.shape == ref.shape and y.dtype == ref.dtype
    assert np.array_equal(np.isfinite(y), np.isfinite(ref)) and np.isfinite(y).all()
    assert not y[3].any() and not y[1].any() and not ((y != 0) & c.dead).any()
    assert y[0].any() and y[2].any()
    if asym:
        e, blk = pd.item_rel_l2(y, ref)[0], pd.block_measure(y, ref, hop)[0]
        noise, block = pd.rtisi_measures(name)
        gate = pd.F64_GATE if dtype == f64 else max(1e-4, 3 * noise[0])
        bgate = pd.F64_BLOCK_GATE if dtype == f64 else max(1e-4, 6 * block[0])
        print(f"{name}: item 0 rel_l2 {e:.3e} gate {gate:.3e} (noise32 {noise[0]:.3e}); block {blk:.3e} gate {bgate:.3e}")
        assert e <= gate and blk <= bgate, (e, gate, blk, bgate)
    clear_plan_cache()


def test_rtisi_stream_on_a_padded_batch_equals_the_whole_signal_call():
    """bit for bit, as tests/test_gpu_stream.py demands: pushes that begin and end inside silence"""
    name = "2048/512 LA3"
    n_fft, hop, frames, dtype, la = pd.RTISI_CASES[name]
    c = pd.case(name)
    whole = _rtisi(name, True)
    s = si.RTISIStream(c.mag.shape[1], batch=pd.BATCH, look_ahead=la, asymmetric_window=True, max_iter=pd.RTISI_ITERS,
                       alpha=pd.RTISI_ALPHA, max_push=5, device=DEV, **_tkw(c.kw))
    mag = T_(c.mag)
    out = [s.push(mag[:, :, t:t + 5]) for t in range(0, frames, 5)] + [s.flush()]
    y = torch.cat(out, 1)
    assert y.shape == whole.shape and torch.equal(y, whole), rel_l2(N(y), N(whole))
    clear_plan_cache()


# ---- the L-BFGS objective at silent frames ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["walk", "bands", "matrix", "chain", "chain64", "mag", "mag64"])
def test_objective_gradient_at_silent_frames(monkeypatch, mode):
    """The harness of test_gpu_fast.py::test_fast_logmel_gradient_vs_autograd_f32 with x the padded signals of items 0 and 3 and the
    log-mel of item 1 for the target: |S| is exactly 0 in whole frames of x, of the target, or of both.  Every route of the log-mel
    objective - the frame walk, the band form, the matrix cores, the kernel chain in float32 and float64 - and the magnitude
    transform, against torch autograd in float64 on the CPU.  The gradient is finite, exactly 0 on dead samples (abs's subgradient 0
    at 0, the kernels' select), and within that test's tolerance elsewhere."""
    n_fft, hop = 2048, 512
    c = pd.case("2048/512")
    dt = torch.float64 if mode.endswith("64") else torch.float32
    x = torch.from_numpy(np.array(c.x[[0, 3]]))
    xt = torch.from_numpy(np.array(c.x[[1, 1]]))
    dead = c.dead[[0, 3]]
    fb = si.mel_filterbank(22050, n_fft, 80)
    win64 = torch.from_numpy(np.array(c.kw["window"])).double()
    fb64 = torch.from_numpy(fb).double()

    def fn(v):
        s = torch.stft(v, n_fft, hop_length=hop, window=win64, return_complex=True).abs()
        return s if mode.startswith("mag") else torch.log1p(torch.matmul(fb64, s))

    target64 = fn(xt.double())
    xr = x.double().requires_grad_(True)
    loss_ref = torch.nn.functional.mse_loss(fn(xr), target64)
    (g_ref,) = torch.autograd.grad(loss_ref, xr)
    assert torch.isfinite(g_ref).all() and not g_ref.numpy()[dead].any() and g_ref[0].abs().max() > 0

    fused = mode in ("walk", "bands", "matrix")
    monkeypatch.setenv("SPECINV_DISABLE_FUSED_OBJECTIVE", "0" if fused else "1")
    monkeypatch.setenv("SPECINV_REQUIRE_FUSED_OBJECTIVE", "1" if fused else "0")
    monkeypatch.setenv("SPECINV_OBJ_SPARSE", "0" if mode == "matrix" else "1")
    monkeypatch.setenv("SPECINV_OBJ_WALK", "1" if mode == "walk" else "0")
    win = win64.to(dt).to(DEV)
    if mode.startswith("mag"):
        tr = si.MagSTFT(n_fft, hop_length=hop, window=win)
    else:
        tr = si.LogMelSTFT(torch.from_numpy(fb).to(dt).to(DEV), n_fft, hop_length=hop, window=win)
    xd = x.to(dt).to(DEV)
    target = tr(xt.to(dt).to(DEV))
    assert rel_l2(N(target), target64.numpy()) < 2e-6 and not N(tr(xd))[1].any()
    _, fg = tr.bind(xd, target)
    loss, grad = fg(xd)
    if not mode.startswith("mag"):
        assert fg.device_objective[0].objective_kind == ("chain" if not fused else mode)
    g = N(grad)
    assert np.isfinite(g).all() and math.isfinite(loss)
    assert not g[dead].any(), f"{np.count_nonzero(g[dead])} dead samples with a gradient"
    e = rel_l2(g, g_ref.numpy())
    print(f"{mode}: loss {loss:.9e} autograd {loss_ref.item():.9e}; gradient rel_l2 {e:.3e}")
    assert abs(loss - loss_ref.item()) < 2e-5 * loss_ref.item()
    assert e < 2e-5
    clear_plan_cache()
