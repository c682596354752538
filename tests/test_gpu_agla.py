"""Accelerated Griffin-Lim on the device (`specinv_agla_*`, csrc/kernels_agla.h) through `Plan` and
`spectrogram_inversion_amd.accelerated_griffin_lim`, against its NumPy restatement (tests/_agla_oracle.py): every kernel family
the projection can take - the extrapolation kernel has to edit the state each of them reads next - both arms of the kernel
(gamma = 1 without d, the general one) and its 16- / 8- / 4-byte accesses.  Needs an MI355X: `-m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch

import _agla_oracle as ao
import oracle
from _util import hann, rel_l2
from oracle.stftlib import args_helper as np_args, signal_length

pytestmark = pytest.mark.gpu

import spectrogram_inversion_amd as si                                    # noqa: E402
from spectrogram_inversion_amd import _lib                                 # noqa: E402
from spectrogram_inversion_amd import agla as agla_mod                      # noqa: E402
from spectrogram_inversion_amd import plan as plan_mod                      # noqa: E402
from spectrogram_inversion_amd.plan import Plan, args_helper, clear_plan_cache, get_plan   # noqa: E402

DEV = torch.device("cuda", 0)
F64_GATE = 1e-10
F32_FLOOR = 2e-5                # tests/test_gpu_misi.py's float32 gate
PARAMS = [(0.99, None, 1.0), (0.5, 1.2, 0.7)]          # Fast Griffin-Lim at the default momentum; all three sequences live
ITERS = 5


def N(t):
    return t.detach().cpu().numpy()


def T_(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _case(n_fft, hop, frames, batch, extra, dtype, seed=None):
    """mag = rng.random + 0.05, uniform phases: a complex start (batch, F, frames), its stft kwargs, the signal length"""
    rng = np.random.default_rng(n_fft + hop + frames + batch if seed is None else seed)
    extra = dict(extra)
    rect = extra.pop("rect", False)
    wl = extra.get("win_length", n_fft)
    kw = dict(hop_length=hop, window=np.ones(wl, dtype) if rect else hann(wl, dtype), **extra)
    F = n_fft // 2 + 1 if extra.get("onesided", True) else n_fft
    mag = (rng.random((batch, F, frames)) + 0.05).astype(dtype)
    start = (mag * np.exp(1j * rng.uniform(-np.pi, np.pi, mag.shape))).astype(np.complex64 if dtype == np.float32 else np.complex128)
    return start, kw, signal_length(frames, np_args(F, dtype, **kw))


def _tkw(kw):
    return dict(kw, window=torch.from_numpy(kw["window"]))


def _plan(start, kw, dtype, generic=False):
    batch, F, frames = start.shape
    p = Plan(args_helper(torch.empty((1, F, 1), dtype=torch.complex64 if dtype == np.float32 else torch.complex128), **_tkw(kw)),
             batch, frames, torch.float32 if dtype == np.float32 else torch.float64, DEV)
    if generic:
        p.force_generic(True)
    return p


def _run(p, start, params, iters=ITERS):
    """`iters` iterations, the last one evaluating: (t_N, its sums)"""
    alpha, beta, gamma = params
    p.agla_init(T_(start), None, alpha, alpha if beta is None else beta, gamma)
    p.agla_iterate(iters - 1)
    sums = p.agla_iterate(1, eval_last=True)
    return N(p.wave()), sums


def _oracle(start, kw, params, iters=ITERS, sums=None):
    alpha, beta, gamma = params
    with np.errstate(all="ignore"):
        return ao.agla(start, iters, alpha=alpha, beta=beta, gamma=gamma, eva_iter=iters, sums=sums, **kw)


def _reference_and_gate(start, kw, params, dtype, iters=ITERS, sums=None):
    """The oracle in the case's dtype and the gate on rel-L2 against it.  float32: the larger of MISI's 2e-5 and 6 x the oracle's own
    float32-against-float64 rel-L2 on this case (the project's rule: 6 x the reference's own noise) - extrapolation with
    alpha + beta > 1 amplifies rounding more than MISI's coupling does."""
    ref = _oracle(start, kw, params, iters, sums)
    if dtype == np.float64:
        return ref, F64_GATE
    ref64 = _oracle(start.astype(np.complex128), dict(kw, window=kw["window"].astype(np.float64)), params, iters)
    fin = np.isfinite(ref) & np.isfinite(ref64)
    spread = rel_l2(ref[fin], ref64[fin])
    print(f"oracle float32 vs float64 {spread:.3e}")
    return ref, max(F32_FLOOR, 6 * spread)


def _check(y, ref, gate, L, what="vs oracle"):
    fin = np.isfinite(ref)
    assert y.shape == ref.shape and y.shape[-1] == L and np.array_equal(np.isfinite(y), fin)
    e = rel_l2(y[fin], ref[fin])
    print(f"rel_l2 {what} {e:.3e} gate {gate:.3e}")
    assert e <= gate, (e, gate)
    return e


# The shape lists of tests/test_gpu_misi.py, its B * K as the batch.
# n_fft, hop, frames, batch, extra stft kwargs, dtype, the kernel launch_geometry must report (None: not asserted)
GENERIC = [
    (512, 128, 12, 6, {}, np.float32, "k_semi"),
    (2048, 512, 9, 2, {}, np.float32, "k_semi"),
    (1024, 256, 10, 8, {}, np.float32, "k_semi"),
    (256, 64, 19, 3, dict(pad_mode="constant"), np.float32, "k_wave_iter"),
    (512, 128, 9, 5, {}, np.float32, "k_semi"),
    (400, 160, 13, 2, {}, np.float32, None),
    (512, 100, 11, 3, dict(onesided=False, win_length=300), np.float32, "k_semi"),     # L = 1000
    (512, 128, 12, 6, {}, np.float64, "k_wave_iter"),
    (1024, 256, 10, 2, dict(onesided=False), np.float32, "k_semi"),
    (256, 64, 12, 3, dict(center=False, rect=True), np.float32, "k_wave_iter"),        # the envelope does not vanish
    (256, 77, 10, 8, {}, np.float32, "k_wave_iter"),                                   # L = 693: 4-byte accesses
    (256, 77, 10, 5, {}, np.float64, "k_wave_iter"),                                   # ... 8-byte in float64
    (256, 50, 10, 3, dict(win_length=200), np.float32, "k_wave_iter"),                 # L = 450: 8-byte accesses
    (1000, 250, 7, 2, {}, np.float64, None),
    (32768, 8192, 5, 2, {}, np.float32, "k_iter_pair"),                                # kernels_big.h
]


@pytest.mark.parametrize("params", PARAMS, ids=["fgla", "general"])
@pytest.mark.parametrize("n_fft,hop,frames,batch,extra,dtype,kernel", GENERIC)
def test_agla_matches_the_oracle(n_fft, hop, frames, batch, extra, dtype, kernel, params):
    """5 iterations (the last evaluating) from a random complex start, the plan's own routing for small problems."""
    clear_plan_cache()
    start, kw, L = _case(n_fft, hop, frames, batch, extra, dtype)
    p = _plan(start, kw, dtype)
    y, sums = _run(p, start, params)
    assert kernel is None or p.launch_geometry["kernel"] == kernel, p.launch_geometry
    osums = []
    ref, gate = _reference_and_gate(start, kw, params, dtype, sums=osums)
    print(f"sums {sums[:2]} oracle {osums[-1][:2]}")
    _check(y, ref, gate, L)


# The float32 wave-level kernels with their chunk-walking forms switched on for small problems (conftest: chunked_kernel); frame
# counts as in tests/test_gpu_misi.py: the chunk tails (fused kernels) and the mended seams (k_hop) are really exercised.
CHUNKED = [
    (1024, 256, 16, 6, {}, "k_fused4", 2),
    (2048, 512, 16, 2, {}, "k_fused4", 2),
    (512, 128, 16, 8, {}, "k_fused", 2),
    (1024, 512, 16, 5, {}, "k_fused", 2),                         # hop = n_fft / 2
    (2048, 256, 32, 3, {}, "k_fused", 2),                         # hop = n_fft / 8
    (4096, 1024, 16, 2, {}, "k_fused", 2),
    (1024, 256, 26, 3, {}, "k_fused4", 3),                        # chunks of 8, 9, 9 frames
    (1024, 77, 28, 3, {}, "k_hop", 2),                            # L = 2079
    (512, 100, 16, 4, dict(win_length=300), "k_hop", 2),
    (1024, 300, 16, 4, dict(onesided=False), "k_hop", 2),         # k_hop2
    (1024, 256, 7, 3, {}, "k_fused4", 1),                         # one chunk: the fused kernel without tails
    (1024, 256, 5, 3, {}, "k_hop", 1),                            # fewer than n_fft / hop + 2 frames: k_hop, one chunk, no seams
]


@pytest.mark.parametrize("params", PARAMS, ids=["fgla", "general"])
@pytest.mark.parametrize("n_fft,hop,frames,batch,extra,kernel,chunks", CHUNKED)
def test_agla_on_every_fast_kernel_family(chunked_kernel, n_fft, hop, frames, batch, extra, kernel, chunks, params):
    start, kw, L = _case(n_fft, hop, frames, batch, extra, np.float32)
    p = _plan(start, kw, np.float32)
    y, sums = _run(p, start, params)
    geo = p.launch_geometry
    assert p.fast_path and geo["kernel"] == kernel and geo["chunks"] == chunks, geo
    osums = []
    ref, gate = _reference_and_gate(start, kw, params, np.float32, sums=osums)
    print(f"sums {sums[:2]} oracle {osums[-1][:2]}")
    _check(y, ref, gate, L)


# ---- ties to the existing paths -----------------------------------------------------------------------------------------
def _tie_to_griffin_lim(shape, dtype, kernel):
    """alpha = 0, gamma = 1 is Griffin-Lim without momentum: `gla_init(alpha=0)` + 5 iterations on the kernels griffin_lim takes."""
    start, kw, L = _case(*shape, dtype)
    p = _plan(start, kw, dtype)
    p.gla_init(T_(start), None, 0.0)
    p.iterate(ITERS)
    g, ggeo = N(p.wave()), p.launch_geometry
    y, _ = _run(p, start, (0.0, None, 1.0))
    assert p.launch_geometry["kernel"] == kernel, p.launch_geometry
    ref, gate = _reference_and_gate(start, kw, (0.0, None, 1.0), dtype)
    with np.errstate(all="ignore"):
        assert np.array_equal(ref, oracle.griffin_lim(start, max_iter=ITERS, alpha=0.0, tol=0, **kw))
    _check(y, ref, gate, L)
    _check(y, g, gate, L, f"vs griffin_lim(alpha=0) on {ggeo['kernel']}")


def test_without_extrapolation_it_is_griffin_lim_fused(chunked_kernel):
    _tie_to_griffin_lim((1024, 256, 16, 6, {}), np.float32, "k_fused4")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_without_extrapolation_it_is_griffin_lim_coverage(dtype):
    clear_plan_cache()
    _tie_to_griffin_lim((256, 77, 10, 4, {}), dtype, "k_wave_iter")


@pytest.mark.parametrize("chunked", [False, True], ids=["rows", "rows_and_tails"])
def test_gamma_one_ignores_beta_and_keeps_no_d(chunked, monkeypatch):
    if chunked:
        monkeypatch.setenv("SPECINV_SMALL_FRAMES", "0")
    clear_plan_cache()
    start, kw, L = _case(1024, 256, 16, 3, {}, np.float32)
    p = _plan(start, kw, np.float32)
    y0, _ = _run(p, start, (0.7, 0.0, 1.0))
    geo = p.launch_geometry
    assert (geo["kernel"], geo["chunks"]) == ("k_fused4", 2) if chunked else geo["kernel"] == "k_semi", geo
    bytes0 = p.device_bytes
    y3, _ = _run(p, start, (0.7, 3.0, 1.0))
    assert np.array_equal(y0, y3) and p.device_bytes == bytes0
    yg, _ = _run(p, start, (0.7, 3.0, 0.7))
    assert p.device_bytes == bytes0 + start.shape[0] * L * 4, (p.device_bytes, bytes0)     # d: one more (B, L) buffer
    assert not np.array_equal(yg, y0)
    y0b, _ = _run(p, start, (0.7, 0.0, 1.0))
    assert np.array_equal(y0, y0b) and p.device_bytes == bytes0                             # ... gone again with gamma = 1
    clear_plan_cache()


def test_default_and_generic_paths_agree(chunked_kernel):
    start, kw, L = _case(1024, 256, 16, 6, {}, np.float32)
    ref, gate = _reference_and_gate(start, kw, PARAMS[1], np.float32)
    out = {}
    for generic in (False, True):
        p = _plan(start, kw, np.float32, generic)
        out[generic], _ = _run(p, start, PARAMS[1])
        assert p.fast_path != generic
        if not generic:
            assert p.launch_geometry["kernel"] == "k_fused4" and p.launch_geometry["chunks"] == 2, p.launch_geometry
    _check(out[False], out[True], gate, L, "fast vs generic")
    _check(out[True], ref, gate, L, "generic vs oracle")


@pytest.mark.parametrize("chunked", [False, True], ids=["k_semi", "k_fused4"])
def test_real_magnitudes_start_from_the_device_phase_init(chunked, monkeypatch):
    """A real input is the target as it is and starts from `phase_init` on the device: the same bits as a start from
    `plan.phase_init(mag)` with `mag` as the target.  (The public complex-input call takes |start| for the target, which is mag
    only to a rounding: that one is compared at the float32 gate.)"""
    if chunked:
        monkeypatch.setenv("SPECINV_SMALL_FRAMES", "0")
    clear_plan_cache()
    start, kw, L = _case(1024, 256, 16, 3, {}, np.float32)
    mag = T_(np.abs(start))
    tk = dict(max_iter=ITERS, tol=0, eva_iter=2, verbose=False, alpha=0.5, beta=1.2, gamma=0.7, **_tkw(kw))
    y = si.accelerated_griffin_lim(mag, **tk)
    assert tuple(y.shape) == (3, L) and y.device.type == "cuda"
    p = _plan(start, kw, np.float32)
    c0 = p.phase_init(mag)
    p.agla_init(c0, mag, 0.5, 1.2, 0.7)
    p.run(ITERS, 2, 0.0)
    assert p.launch_geometry["kernel"] == ("k_fused4" if chunked else "k_semi"), p.launch_geometry
    assert torch.equal(y, p.wave())
    yc = si.accelerated_griffin_lim(c0, **tk)
    _, gate = _reference_and_gate(N(c0), kw, (0.5, 1.2, 0.7), np.float32)
    _check(N(yc), N(y), gate, L, "complex-input call vs real-input call")
    clear_plan_cache()


def test_evaluation_and_stop_rule():
    """eva_iter = 2, max_iter = 6: the second evaluation (after iteration 4) stops the run when the loss fell by less than tol x the
    first; tol is set half as large again as the oracle's own relative decrease there - and two thirds of it would not stop."""
    clear_plan_cache()
    start, kw, L = _case(512, 128, 12, 3, {}, np.float32, seed=11)
    prm = dict(alpha=0.99, beta=None, gamma=1.0)
    free = []
    with np.errstate(all="ignore"):
        ao.agla(start, 6, eva_iter=2, trace=free, **prm, **kw)
    assert [t[0] for t in free] == [1, 3, 5]
    r1 = (free[0][2] - free[1][2]) / free[0][2]
    assert r1 > 0, free
    tol = 1.5 * r1
    trace, osums, loose = [], [], []
    with np.errstate(all="ignore"):
        ref = ao.agla(start, 6, tol=tol, eva_iter=2, trace=trace, sums=osums, **prm, **kw)
        ao.agla(start, 6, tol=r1 / 1.5, eva_iter=2, trace=loose, **prm, **kw)
        longer = ao.agla(start, 6, eva_iter=2, **prm, **kw)
    assert [t[0] for t in trace] == [1, 3] and len(osums) == 4 and len(loose) == 3      # the rule fires at iteration 4, and only just
    _, gate = _reference_and_gate(start, kw, (0.99, None, 1.0), np.float32, iters=4)
    p = _plan(start, kw, np.float32)
    p.agla_init(T_(start), None, 0.99, 0.99, 1.0)
    done, evals = p.run(6, 2, tol)
    print(f"tol {tol:.4e} oracle trace {trace} device {evals}")
    assert done == 4 and [e[0] for e in evals] == [1, 3], (done, evals)
    for (_, m, loss), (_, om_, oloss) in zip(evals, trace):
        np.testing.assert_allclose([m, loss], [om_, oloss], rtol=1e-5)
    _check(N(p.wave()), ref, gate, L)
    # the sums themselves, stepping by hand
    p.agla_init(T_(start), None, 0.99, 0.99, 1.0)
    for k in (1, 3):
        s = p.agla_iterate(2, eval_last=True)
        print(f"sums at {k}: {s} oracle {osums[k]}")
        np.testing.assert_allclose(s, osums[k], rtol=1e-5)
    # and the public function stops where the oracle does
    y = si.accelerated_griffin_lim(T_(start), max_iter=6, tol=tol, eva_iter=2, verbose=False, **_tkw(kw))
    e = _check(N(y), ref, gate, L, "api vs oracle stopped at 4")
    assert e < rel_l2(longer, ref), (e, rel_l2(longer, ref))


def test_neighbours_are_untouched(chunked_kernel):
    """griffin_lim(alpha=0.3) and misi on one cached plan, an AGLA run on it, both again: the same bits."""
    start, kw, L = _case(1024, 256, 16, 6, {}, np.float32)
    rng = np.random.default_rng(5)
    mix = T_((0.1 * rng.standard_normal((2, L))).astype(np.float32))
    tk = dict(max_iter=4, tol=0, eva_iter=2, verbose=False, **_tkw(kw))
    s3 = T_(start)

    def both():
        g = si.griffin_lim(s3, alpha=0.3, **tk)
        m = si.misi(s3.reshape(2, 3, *s3.shape[1:]), mix, **tk)
        return g, m.reshape(6, L)

    plan = get_plan(args_helper(s3, **_tkw(kw)), 6, 16, torch.float32, DEV)
    g0, m0 = both()
    y = si.accelerated_griffin_lim(s3, alpha=0.5, beta=1.2, gamma=0.7, **tk)
    assert get_plan(args_helper(s3, **_tkw(kw)), 6, 16, torch.float32, DEV) is plan and plan._method == "agla"
    assert plan.launch_geometry["kernel"] == "k_fused4", plan.launch_geometry
    g1, m1 = both()
    assert torch.equal(g0, g1) and torch.equal(m0, m1)
    assert not torch.equal(y, g0) and torch.isfinite(y).all()


def test_c_abi_state_and_argument_errors():
    clear_plan_cache()
    start, kw, L = _case(512, 128, 8, 3, {}, np.float32)
    p = _plan(start, kw, np.float32)
    lib, h = p.lib, p._h
    sums = (C.c_double * 4)()
    err = lambda: lib.specinv_last_error().decode()
    run = lambda fn: fn(h, 10, 5, 0.0, 0, None, None, None, _lib.EVAL_CB(), None)
    flat = T_(start)
    mix = T_(np.zeros((1, L), np.float32))
    # before any init
    assert lib.specinv_agla_iterate(h, 1, 0, sums) == _lib.ESTATE and "specinv_agla_init" in err()
    assert run(lib.specinv_agla_run) == _lib.ESTATE and "specinv_agla_init" in err()
    # argument errors on a real plan leave no state behind
    for a, b, g in ((-1.0, 0.5, 1.0), (0.5, -1.0, 1.0), (0.5, 0.5, 0.0)):
        assert lib.specinv_agla_init(h, flat.data_ptr(), None, a, b, g) == _lib.EINVAL
    assert lib.specinv_agla_init(h, None, None, 0.5, 0.5, 1.0) == _lib.EINVAL          # neither pointer, as specinv_gla_init
    assert lib.specinv_agla_iterate(h, 1, 0, sums) == _lib.ESTATE
    # the other methods' entry points on a plan in the AGLA state
    p.agla_init(flat, None, 0.99, 0.99, 1.0)
    assert lib.specinv_agla_iterate(h, 2, 1, sums) == _lib.OK
    for fn in (lib.specinv_gla_iterate, lib.specinv_admm_iterate, lib.specinv_misi_iterate):
        assert fn(h, 1, 0, sums) == _lib.ESTATE and "AGLA" in err()
    for fn in (lib.specinv_gla_run, lib.specinv_admm_run, lib.specinv_misi_run):
        assert run(fn) == _lib.ESTATE and "AGLA" in err()
    t2 = p.wave()
    assert lib.specinv_agla_iterate(h, 1, 0, sums) == _lib.OK and not torch.equal(p.wave(), t2)     # the refusals changed nothing
    # ... and AGLA's on a plan in theirs
    p.gla_init(flat, None, 0.0)
    assert lib.specinv_agla_iterate(h, 1, 0, sums) == _lib.ESTATE and run(lib.specinv_agla_run) == _lib.ESTATE
    p.admm_init(flat, None, 0.1)
    assert lib.specinv_agla_iterate(h, 1, 0, sums) == _lib.ESTATE and run(lib.specinv_agla_run) == _lib.ESTATE
    p.misi_init(flat, None, mix, 3)
    assert lib.specinv_agla_iterate(h, 1, 0, sums) == _lib.ESTATE and run(lib.specinv_agla_run) == _lib.ESTATE
    assert lib.specinv_misi_iterate(h, 1, 0, sums) == _lib.OK


# ---- spectrogram_inversion_amd.accelerated_griffin_lim ------------------------------------------------------------------
def test_api_shapes_devices_and_narrow_dtypes():
    clear_plan_cache()
    start, kw, L = _case(512, 128, 10, 3, {}, np.float32)
    tk = dict(max_iter=5, tol=0, eva_iter=2, verbose=False, **_tkw(kw))
    y3 = si.accelerated_griffin_lim(T_(start), **tk)
    y2 = si.accelerated_griffin_lim(T_(start[0]), **tk)                     # (F, T) in, (L,) out
    y1 = si.accelerated_griffin_lim(T_(start[:1]), **tk)                    # exactly (1, F, T) keeps its batch axis, as griffin_lim
    assert tuple(y3.shape) == (3, L) and tuple(y2.shape) == (L,) and tuple(y1.shape) == (1, L)
    assert torch.equal(y2, y1[0])
    ref, gate = _reference_and_gate(start, kw, (0.99, None, 1.0), np.float32)           # the defaults: Fast Griffin-Lim at 0.99
    _check(N(y3), ref, gate, L)
    ycpu = si.accelerated_griffin_lim(torch.from_numpy(start), **tk)          # CPU in, CPU out
    assert ycpu.device.type == "cpu" and torch.equal(ycpu, y3.cpu())
    mag = T_(np.abs(start))
    yh = si.accelerated_griffin_lim(mag.half(), **tk)                         # narrow inputs: computed in float32, rounded back
    assert yh.dtype == torch.float16 and tuple(yh.shape) == (3, L) and torch.isfinite(yh).all()
    assert torch.equal(yh, si.accelerated_griffin_lim(mag.half().float(), **tk).half())
    yb = si.accelerated_griffin_lim(mag.bfloat16(), **tk)
    assert yb.dtype == torch.bfloat16 and torch.equal(yb, si.accelerated_griffin_lim(mag.bfloat16().float(), **tk).bfloat16())
    y64 = si.accelerated_griffin_lim(T_(start.astype(np.complex128)), **dict(tk, window=tk["window"].double()))
    assert y64.dtype == torch.float64


def test_api_batches_beyond_one_plan_run_as_slices(monkeypatch):
    """7 items with 3 to a plan: slices of 3, 3 and 1 stepped in lockstep - the bits of the one-plan run (tol = 0: the stop rule,
    which sees the summed sums, never fires)."""
    clear_plan_cache()
    start, kw, L = _case(512, 128, 10, 7, {}, np.float32)
    tk = dict(max_iter=5, tol=0, eva_iter=2, verbose=False, alpha=0.5, beta=1.2, gamma=0.7, **_tkw(kw))
    whole = si.accelerated_griffin_lim(T_(start), **tk)
    monkeypatch.setattr(agla_mod, "_MAX_PLAN_BATCH", 3)
    made = []
    monkeypatch.setattr(plan_mod, "Plan", lambda *a, **k: made.append(a[1]) or Plan(*a, **k))      # (Plan: the class as imported above)
    sliced = si.accelerated_griffin_lim(T_(start), **tk)
    assert made == [3, 3, 1] and tuple(sliced.shape) == (7, L)
    assert torch.equal(whole, sliced)
