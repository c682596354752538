"""constrained_griffin_lim on the device (`specinv_agla_constrain`, csrc/kernels_agla.h) through `Plan` and the public function,
against its NumPy restatement (tests/_cgla_oracle.py): every kernel family the projection can take - the step kernel edits the
state each of them reads next - both arms of the kernel, its 16- / 8- / 4-byte accesses, mask edges inside a thread's vector and
masks that differ from item to item.  Needs an MI355X: `-m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch

import _cgla_oracle as co
from _util import hann, rel_l2
from oracle.stftlib import args_helper as np_args, signal_length, stft as np_stft

pytestmark = pytest.mark.gpu

import spectrogram_inversion_amd as si                                    # noqa: E402
from spectrogram_inversion_amd import _lib                                 # noqa: E402
from spectrogram_inversion_amd import constrained as cg                     # noqa: E402
from spectrogram_inversion_amd.plan import Plan, args_helper, clear_plan_cache, get_plan   # noqa: E402

DEV = torch.device("cuda", 0)
F64_GATE = 1e-10
F32_FLOOR = 2e-5                # tests/test_gpu_agla.py's float32 gate
PARAMS = [(0.99, None, 1.0), (0.5, 1.2, 0.7)]          # Fast Griffin-Lim at the default momentum; all three sequences live
ITERS = 5


def N(t):
    return t.detach().cpu().numpy()


def T_(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _case(n_fft, hop, frames, batch, extra, dtype, spec=True, wave=True):
    """A real test signal gives the known values: K its STFT, xk itself.  The start has |K| with random phases.  spec_mask: the bins
    below F / 4 plus two whole frames in the middle (two-sided: the frames alone, which keeps the mask Hermitian); wave_mask:
    [0, L / 3) plus a run of 37 samples from an odd index, so mask edges fall inside a thread's vector; item b's masks are shifted
    by b."""
    rng = np.random.default_rng(n_fft + hop + frames + batch)
    extra = dict(extra)
    wl = extra.get("win_length", n_fft)
    kw = dict(hop_length=hop, window=hann(wl, dtype), **extra)
    onesided = extra.get("onesided", True)
    F = n_fft // 2 + 1 if onesided else n_fft
    a = np_args(F, dtype, **kw)
    L = signal_length(frames, a)
    n = np.arange(L)
    x = np.stack([np.sin(2 * np.pi * (0.013 + 0.007 * b) * n) * (1 + 0.5 * np.sin(2 * np.pi * n / 211)) for b in range(batch)])
    x = (x + 0.1 * rng.standard_normal(x.shape)).astype(dtype)
    K = np_stft(x, a)
    start = (np.abs(K) * np.exp(1j * rng.uniform(-np.pi, np.pi, K.shape))).astype(K.dtype)
    M = np.zeros((batch, F, frames), bool)
    W = np.zeros((batch, L), bool)
    for b in range(batch):
        if onesided:
            M[b, : F // 4 + b] = True
        M[b, :, [(frames // 2 - 1 + b) % frames, (frames // 2 + b) % frames]] = True
        W[b, : L // 3 + b] = True
        lo = (L // 2 | 1) + 2 * b
        assert lo % 2 == 1 and lo + 37 <= L
        W[b, lo: lo + 37] = True
    con = {}
    if spec:
        con.update(known_spec=K, spec_mask=M)
    if wave:
        con.update(known_wave=x, wave_mask=W)
    return dict(start=start, con=con, kw=kw, L=L, x=x, W=W, K=K, M=M, dtype=dtype)


def _tkw(kw):
    return dict(kw, window=torch.from_numpy(kw["window"]))


def _tcon(con, dev=DEV):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in con.items()}


def _plan(c):
    batch, F, frames = c["start"].shape
    f32 = c["dtype"] == np.float32
    return Plan(args_helper(torch.empty((1, F, 1), dtype=torch.complex64 if f32 else torch.complex128), **_tkw(c["kw"])),
                batch, frames, torch.float32 if f32 else torch.float64, DEV)


def _run(p, c, params, iters=ITERS):
    """The plan under the constraint as the public function sets it up, `iters` iterations: t_N"""
    alpha, beta, gamma = params
    tc = _tcon(c["con"])
    cg._begin(p, T_(c["start"]), tc.get("known_spec"), tc.get("spec_mask"), tc.get("known_wave"), tc.get("wave_mask"),
              alpha, alpha if beta is None else beta, gamma)
    p.agla_iterate(iters)
    return N(p.wave())


def _oracle(c, params, iters=ITERS, f64=False, **more):
    alpha, beta, gamma = params
    start, con, kw = c["start"], c["con"], c["kw"]
    if f64:
        start = start.astype(np.complex128)
        kw = dict(kw, window=kw["window"].astype(np.float64))
        con = {k: (v if v.dtype == bool else v.astype(np.complex128 if np.iscomplexobj(v) else np.float64)) for k, v in con.items()}
    with np.errstate(all="ignore"):
        return co.cgla(start, iters, alpha=alpha, beta=beta, gamma=gamma, **dict(dict(eva_iter=iters), **more), **con, **kw)


def _reference_and_gate(c, params, iters=ITERS):
    """The oracle in the case's dtype and the gate on rel-L2 against it: float64 1e-10; float32 the larger of 2e-5 and 6 x the
    oracle's own float32-against-float64 rel-L2 on this case (tests/test_gpu_agla.py's rule).  Every case's oracle output is
    finite: no sample is left out of the comparison."""
    ref = _oracle(c, params, iters)
    assert np.isfinite(ref).all()
    if c["dtype"] == np.float64:
        return ref, F64_GATE
    ref64 = _oracle(c, params, iters, f64=True)
    assert np.isfinite(ref64).all()
    spread = rel_l2(ref, ref64)
    print(f"oracle float32 vs float64 {spread:.3e}")
    return ref, max(F32_FLOOR, 6 * spread)


def _check(y, ref, gate, what="vs oracle"):
    assert y.shape == ref.shape and np.isfinite(y).all()
    e = rel_l2(y, ref)
    print(f"rel_l2 {what} {e:.3e} gate {gate:.3e}")
    assert e <= gate, (e, gate)
    return e


def _known_samples_exact(y, c):
    if "known_wave" in c["con"]:
        assert np.array_equal(y[c["W"]], c["x"][c["W"]])


# ---- 1. parity through Plan ------------------------------------------------------------------------------------------------
# Shapes from tests/test_gpu_agla.py's lists: the smallest that reach each kernel family and access width.
# n_fft, hop, frames, batch, extra stft kwargs, dtype, the kernel launch_geometry must report (None: not asserted)
DEFAULT = [
    (512, 128, 12, 6, {}, np.float32, "k_semi"),
    (256, 64, 19, 3, dict(pad_mode="constant"), np.float32, "k_wave_iter"),
    (512, 128, 12, 6, {}, np.float64, "k_wave_iter"),
    (256, 77, 10, 8, {}, np.float32, None),                                            # L = 693: 4-byte accesses
    (256, 77, 10, 5, {}, np.float64, None),                                            # ... 8-byte in float64
    (256, 50, 10, 3, dict(win_length=200), np.float32, None),                          # L = 450: 8-byte accesses
    (512, 100, 11, 3, dict(onesided=False, win_length=300), np.float32, None),         # two-sided: whole frames masked
    (1000, 250, 7, 2, {}, np.float64, None),
]


@pytest.mark.parametrize("params", PARAMS, ids=["fgla", "general"])
@pytest.mark.parametrize("n_fft,hop,frames,batch,extra,dtype,kernel", DEFAULT)
def test_both_constraints_match_the_oracle(n_fft, hop, frames, batch, extra, dtype, kernel, params):
    """5 iterations under both constraints, the plan's own routing for small problems."""
    clear_plan_cache()
    c = _case(n_fft, hop, frames, batch, extra, dtype)
    p = _plan(c)
    y = _run(p, c, params)
    assert kernel is None or p.launch_geometry["kernel"] == kernel, p.launch_geometry
    ref, gate = _reference_and_gate(c, params)
    _check(y, ref, gate)
    _known_samples_exact(y, c)


# The float32 wave-level kernels with their chunk-walking forms switched on for small problems (conftest: chunked_kernel): the
# step kernel reads and writes the state beside the chunk tails.
CHUNKED = [
    (1024, 256, 16, 6, {}, "k_fused4", 2),
    (512, 128, 16, 8, {}, "k_fused", 2),
    (1024, 256, 26, 3, {}, "k_fused4", 3),                        # chunks of 8, 9, 9 frames
    (1024, 77, 28, 3, {}, "k_hop", 2),                            # L = 2079
    (1024, 256, 7, 3, {}, "k_fused4", 1),                         # one chunk: the fused kernel without tails
]


@pytest.mark.parametrize("params", PARAMS, ids=["fgla", "general"])
@pytest.mark.parametrize("n_fft,hop,frames,batch,extra,kernel,chunks", CHUNKED)
def test_both_constraints_on_every_fast_kernel_family(chunked_kernel, n_fft, hop, frames, batch, extra, kernel, chunks, params):
    c = _case(n_fft, hop, frames, batch, extra, np.float32)
    p = _plan(c)
    y = _run(p, c, params)
    geo = p.launch_geometry
    assert p.fast_path and geo["kernel"] == kernel and geo["chunks"] == chunks, geo
    ref, gate = _reference_and_gate(c, params)
    _check(y, ref, gate)
    _known_samples_exact(y, c)


@pytest.mark.parametrize("params", PARAMS, ids=["fgla", "general"])
@pytest.mark.parametrize("which", ["spec", "wave"])
@pytest.mark.parametrize("chunked", [False, True], ids=["k_semi", "k_fused4"])
def test_one_constraint_alone(chunked, which, params, monkeypatch):
    """Known bins without a sample mask (the kernel's mask pointer is NULL) and known samples without a known bin (offset is the
    known wave under the mask and 0 elsewhere)."""
    if chunked:
        monkeypatch.setenv("SPECINV_SMALL_FRAMES", "0")
    clear_plan_cache()
    shape = (1024, 256, 16, 6) if chunked else (512, 128, 12, 6)
    c = _case(*shape, {}, np.float32, spec=which == "spec", wave=which == "wave")
    p = _plan(c)
    y = _run(p, c, params)
    geo = p.launch_geometry
    assert (geo["kernel"], geo["chunks"]) == ("k_fused4", 2) if chunked else geo["kernel"] == "k_semi", geo
    ref, gate = _reference_and_gate(c, params)
    _check(y, ref, gate)
    _known_samples_exact(y, c)
    clear_plan_cache()


# ---- 2. exact invariants ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", PARAMS, ids=["fgla", "general"])
@pytest.mark.parametrize("chunked", [False, True], ids=["k_semi", "k_fused4"])
def test_known_samples_come_back_bit_for_bit(chunked, params, monkeypatch):
    if chunked:
        monkeypatch.setenv("SPECINV_SMALL_FRAMES", "0")
    clear_plan_cache()
    c = _case(*((1024, 256, 16, 6) if chunked else (512, 128, 12, 6)), {}, np.float32)
    p = _plan(c)
    xk, W = T_(c["x"]), T_(c["W"])
    for iters in (1, 2, ITERS):
        _run(p, c, params, iters)
        y = p.wave()
        assert torch.equal(y[W], xk[W]) and not torch.equal(y[~W], xk[~W])
    clear_plan_cache()


def test_with_every_bin_known_one_iteration_is_the_inverse_transform():
    clear_plan_cache()
    c = _case(512, 128, 12, 6, {}, np.float32, wave=False)
    c["con"]["spec_mask"] = np.ones_like(c["M"])
    p = _plan(c)
    y = _run(p, c, PARAMS[1], 1)
    ref = N(p.istft(T_(c["K"])))
    _check(y, ref, F32_FLOOR, "vs Plan.istft(known_spec)")
    _check(y, c["x"], F32_FLOOR, "vs the signal the bins came from")


# ---- 3. ties ---------------------------------------------------------------------------------------------------------------
def test_without_a_constraint_it_is_accelerated_griffin_lim():
    clear_plan_cache()
    c = _case(512, 128, 12, 3, {}, np.float32)
    tk = dict(max_iter=ITERS, tol=0, eva_iter=2, verbose=False, alpha=0.5, beta=1.2, gamma=0.7, **_tkw(c["kw"]))
    for spec in (T_(c["start"]), T_(np.abs(c["start"])), T_(c["start"][0])):
        assert torch.equal(si.constrained_griffin_lim(spec, **tk), si.accelerated_griffin_lim(spec, **tk))


@pytest.mark.parametrize("chunked", [False, True], ids=["k_semi", "k_fused4"])
def test_neighbours_on_the_same_plan_are_untouched(chunked, monkeypatch):
    """Unconstrained AGLA and griffin_lim on one cached plan, a constrained run on it, both again: the same bits, and the plan
    holds the constraint's B L (sizeof(T) + 1) bytes only while it is set."""
    if chunked:
        monkeypatch.setenv("SPECINV_SMALL_FRAMES", "0")
    clear_plan_cache()
    c = _case(*((1024, 256, 16, 6) if chunked else (512, 128, 12, 6)), {}, np.float32)
    s3, tc = T_(c["start"]), _tcon(c["con"])
    tk = dict(max_iter=4, tol=0, eva_iter=2, verbose=False, **_tkw(c["kw"]))
    prm = dict(alpha=0.5, beta=1.2, gamma=0.7)

    def both():
        return si.accelerated_griffin_lim(s3, **prm, **tk), si.griffin_lim(s3, alpha=0.3, **tk)

    plan = get_plan(args_helper(s3, **_tkw(c["kw"])), s3.shape[0], s3.shape[2], torch.float32, DEV)
    a0, g0 = both()
    y = si.constrained_griffin_lim(s3, **tc, **prm, **tk)
    assert get_plan(args_helper(s3, **_tkw(c["kw"])), s3.shape[0], s3.shape[2], torch.float32, DEV) is plan
    assert plan.launch_geometry["kernel"] == ("k_fused4" if chunked else "k_semi"), plan.launch_geometry
    assert not torch.equal(y, a0) and torch.isfinite(y).all()
    a1, g1 = both()
    assert torch.equal(a0, a1) and torch.equal(g0, g1)
    # through Plan: the constraint's bytes; an init clears it
    plan.agla_init(s3, None, 0.5, 1.2, 0.7)
    bytes1 = plan.device_bytes
    n = s3.shape[0] * c["L"]
    plan.agla_constrain(tc["known_wave"], tc["wave_mask"])
    assert plan.device_bytes == bytes1 + n * 5
    plan.agla_constrain(tc["known_wave"])
    assert plan.device_bytes == bytes1 + n * 4
    plan.agla_constrain(tc["known_wave"], tc["wave_mask"])
    plan.agla_init(s3, None, 0.5, 1.2, 0.7)
    assert plan.device_bytes == bytes1
    plan.agla_iterate(4)
    assert torch.equal(plan.wave(), a0)
    # ... another method's too
    plan.agla_constrain(tc["known_wave"], tc["wave_mask"])
    a2, g2 = both()
    assert torch.equal(a0, a2) and torch.equal(g0, g2)
    clear_plan_cache()


# ---- 4. the public function ------------------------------------------------------------------------------------------------
def test_public_function_trace_and_stop_rule(monkeypatch):
    """(B, F, T) and (F, T) inputs, CPU tensors in and out: the evaluations and the stop iteration are the oracle's."""
    clear_plan_cache()
    c = _case(512, 128, 12, 3, {}, np.float32)
    runs = []
    loop = cg._loop
    monkeypatch.setattr(cg, "_loop", lambda *a, **k: runs.append(loop(*a, **k)) or runs[-1])
    tk = dict(max_iter=20, tol=1e-3, eva_iter=2, verbose=False, **_tkw(c["kw"]))
    for item in (None, 1):
        sel = (lambda v: v) if item is None else (lambda v: v[item])
        ci = dict(c, start=sel(c["start"]), con={k: sel(v) for k, v in c["con"].items()})
        trace = []
        ref = _oracle(ci, PARAMS[0], 20, tol=1e-3, eva_iter=2, trace=trace)
        y = si.constrained_griffin_lim(torch.from_numpy(ci["start"]), **_tcon(ci["con"], "cpu"), **tk)
        done, evals = runs[-1]
        print(f"oracle trace {trace}\ndevice done {done} {evals}")
        assert y.device.type == "cpu" and y.dtype == torch.float32 and tuple(y.shape) == ref.shape
        assert ref.shape == ((3, c["L"]) if item is None else (c["L"],))
        assert [e[0] for e in evals] == [t[0] for t in trace] and done == trace[-1][0] + 1
        for (_, m, loss), (_, om_, oloss) in zip(evals, trace):
            np.testing.assert_allclose([m, loss], [om_, oloss], rtol=1e-5)
        _, gate = _reference_and_gate(ci, PARAMS[0], done)
        _check(N(y), ref, gate)
        assert np.array_equal(N(y)[ci["con"]["wave_mask"]], ci["con"]["known_wave"][ci["con"]["wave_mask"]])
    # the rule firing: tol half as large again as the oracle's own relative decrease at the second evaluation stops the run there
    r1 = (trace[0][2] - trace[1][2]) / trace[0][2]
    assert r1 > 0, trace
    stopped = []
    ref = _oracle(ci, PARAMS[0], 20, tol=1.5 * r1, eva_iter=2, trace=stopped)
    y = si.constrained_griffin_lim(torch.from_numpy(ci["start"]), **_tcon(ci["con"], "cpu"), **dict(tk, tol=1.5 * r1))
    done, evals = runs[-1]
    print(f"tol {1.5 * r1:.4e} oracle trace {stopped} device done {done} {evals}")
    assert [t[0] for t in stopped] == [1, 3] and done == 4 and [e[0] for e in evals] == [1, 3]
    _, gate = _reference_and_gate(ci, PARAMS[0], 4)
    _check(N(y), ref, gate, "vs oracle stopped at 4")


def test_public_function_magnitudes_devices_and_narrow_dtypes():
    clear_plan_cache()
    c = _case(512, 128, 12, 3, {}, np.float32)
    tc = _tcon(c["con"])
    tk = dict(max_iter=ITERS, tol=0, eva_iter=2, verbose=False, alpha=0.5, beta=1.2, gamma=0.7, **_tkw(c["kw"]))
    # real magnitudes start from phase_init(m_full) on the device, the known bins put in
    mag = T_(np.abs(c["start"]))
    y = si.constrained_griffin_lim(mag, **tc, **tk)
    assert y.device.type == "cuda" and tuple(y.shape) == (3, c["L"]) and torch.isfinite(y).all()
    p = _plan(c)
    m_full = torch.where(tc["spec_mask"], tc["known_spec"].abs(), mag)
    yc = si.constrained_griffin_lim(p.phase_init(m_full), **tc, **tk)          # (its modulus is mag to a rounding only)
    cc = dict(c, start=N(p.phase_init(m_full)))
    _, gate = _reference_and_gate(cc, (0.5, 1.2, 0.7))
    _check(N(y), N(yc), gate, "real-input call vs complex-input call")
    # masks that broadcast: one (F, T) mask and one (L,) mask for every item
    M1, W1 = tc["spec_mask"][0], tc["wave_mask"][0]
    yb = si.constrained_griffin_lim(T_(c["start"]), known_spec=tc["known_spec"], spec_mask=M1, known_wave=tc["known_wave"],
                                    wave_mask=W1, **tk)
    ye = si.constrained_griffin_lim(T_(c["start"]), known_spec=tc["known_spec"], spec_mask=M1.expand(3, -1, -1).contiguous(),
                                    known_wave=tc["known_wave"], wave_mask=W1.expand(3, -1).contiguous(), **tk)
    assert torch.equal(yb, ye)
    # narrow inputs: computed in float32, rounded back
    yh = si.constrained_griffin_lim(mag.half(), **tc, **tk)
    assert yh.dtype == torch.float16 and torch.equal(yh, si.constrained_griffin_lim(mag.half().float(), **tc, **tk).half())
    # float64
    c64 = _case(512, 128, 12, 3, {}, np.float64)
    y64 = si.constrained_griffin_lim(T_(c64["start"]), **_tcon(c64["con"]), **dict(tk, **_tkw(c64["kw"])))
    ref64, gate64 = _reference_and_gate(c64, (0.5, 1.2, 0.7))
    _check(N(y64), ref64, gate64)


# ---- 5. the C ABI's states -------------------------------------------------------------------------------------------------
def test_c_abi_state_and_argument_errors():
    clear_plan_cache()
    c = _case(512, 128, 8, 3, {}, np.float32)
    p = _plan(c)
    lib, h = p.lib, p._h
    err = lambda: lib.specinv_last_error().decode()
    off, w = T_(c["x"]), T_(c["W"]).to(torch.uint8)
    flat = T_(c["start"])
    # before specinv_agla_init, and on a plan in another method's state
    assert lib.specinv_agla_constrain(h, off.data_ptr(), w.data_ptr()) == _lib.ESTATE and "specinv_agla_init" in err()
    p.gla_init(flat, None, 0.3)
    assert lib.specinv_agla_constrain(h, off.data_ptr(), None) == _lib.ESTATE
    assert lib.specinv_agla_constrain(h, None, None) == _lib.ESTATE
    # a mask without an offset
    p.agla_init(flat, None, 0.99, 0.99, 1.0)
    bytes0 = p.device_bytes
    assert lib.specinv_agla_constrain(h, None, w.data_ptr()) == _lib.EINVAL and "offset" in err()
    assert p.device_bytes == bytes0
    sums = (C.c_double * 4)()
    assert lib.specinv_agla_iterate(h, 2, 0, sums) == _lib.OK
    free = p.wave()
    # set, cleared by both NULL: the unconstrained run again
    p.agla_init(flat, None, 0.99, 0.99, 1.0)
    assert lib.specinv_agla_constrain(h, off.data_ptr(), w.data_ptr()) == _lib.OK
    assert lib.specinv_agla_constrain(h, None, None) == _lib.OK and p.device_bytes == bytes0
    assert lib.specinv_agla_iterate(h, 2, 0, sums) == _lib.OK and torch.equal(p.wave(), free)
    # ... and set: the known samples
    p.agla_init(flat, None, 0.99, 0.99, 1.0)
    assert lib.specinv_agla_constrain(h, off.data_ptr(), w.data_ptr()) == _lib.OK
    assert lib.specinv_agla_iterate(h, 2, 0, sums) == _lib.OK
    y = p.wave()
    assert torch.equal(y[w.bool()], off[w.bool()]) and not torch.equal(y, free)
