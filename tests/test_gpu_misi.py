"""MISI on the device (`specinv_misi_*`, csrc/kernels_misi.h) through `Plan` and `spectrogram_inversion_amd.misi`, against its
NumPy restatement (tests/_misi_oracle.py): every kernel family the projection can take - the coupling kernel has to edit the state
each of them reads next - every arm of the coupling kernel (K = 2, 3, 4 in registers, the loop, 16- / 8- / 4-byte accesses).
Needs an MI355X: `-m gpu`."""
import ctypes as C

import numpy as np
import pytest
import torch

import _misi_oracle as mo
from _util import hann, rel_l2
from oracle.stftlib import args_helper as np_args, signal_length

pytestmark = pytest.mark.gpu

import spectrogram_inversion_amd as si                                    # noqa: E402
from spectrogram_inversion_amd import _lib                                 # noqa: E402
from spectrogram_inversion_amd.plan import Plan, args_helper, clear_plan_cache   # noqa: E402

DEV = torch.device("cuda", 0)
TOL = {np.float32: 2e-5, np.float64: 1e-10}       # tests/test_gpu_wave.py's gates for the same kind of run


def N(t):
    return t.detach().cpu().numpy()


def T_(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _case(n_fft, hop, frames, B, K, extra, dtype, seed=None):
    """mag = rng.random + 0.05, uniform phases, mix = 0.1 standard_normal (a few samples longer than the signal)"""
    rng = np.random.default_rng(n_fft + hop + frames + K if seed is None else seed)
    extra = dict(extra)
    rect = extra.pop("rect", False)
    wl = extra.get("win_length", n_fft)
    kw = dict(hop_length=hop, window=np.ones(wl, dtype) if rect else hann(wl, dtype), **extra)
    F = n_fft // 2 + 1 if extra.get("onesided", True) else n_fft
    mag = (rng.random((B, K, F, frames)) + 0.05).astype(dtype)
    start = (mag * np.exp(1j * rng.uniform(-np.pi, np.pi, mag.shape))).astype(np.complex64 if dtype == np.float32 else np.complex128)
    L = signal_length(frames, np_args(F, dtype, **kw))
    mix = (0.1 * rng.standard_normal((B, L + 3))).astype(dtype)
    return start, mix, L, kw


def _plan(start, kw, dtype, generic=False):
    B, K, F, frames = start.shape
    tkw = dict(kw, window=torch.from_numpy(kw["window"]))
    p = Plan(args_helper(torch.empty((1, F, 1), dtype=torch.complex64 if dtype == np.float32 else torch.complex128), **tkw),
             B * K, frames, torch.float32 if dtype == np.float32 else torch.float64, DEV)
    if generic:
        p.force_generic(True)
    return p


def _run(p, start, mix, iters=3):
    B, K, F, frames = start.shape
    p.misi_init(T_(start.reshape(B * K, F, frames)), None, T_(mix), K)
    p.misi_iterate(iters)
    sums = p.misi_iterate(1, eval_last=True)
    return N(p.wave()).reshape(B, K, -1), sums


def _check(y, sums, start, mix, L, kw, dtype, iters=3):
    B, K = start.shape[:2]
    osums = []
    with np.errstate(all="ignore"):
        ref = mo.misi(start, mix, iters + 1, eva_iter=iters + 1, sums=osums, **kw)
    fin = np.isfinite(ref)
    assert y.shape == ref.shape == (B, K, L) and np.array_equal(np.isfinite(y), fin)
    e = rel_l2(y[fin], ref[fin])
    print(f"rel_l2 vs oracle {e:.3e}  sums {sums[:2]} oracle {osums[-1][:2]}")
    assert e <= TOL[dtype], e
    np.testing.assert_allclose(sums[:2], osums[-1][:2], rtol=1e-5)
    np.testing.assert_allclose(sums[2:], osums[-1][2:], rtol=1e-5)
    # the sources add up to the mixture: the rounding of K additions (a condition, not a measurement)
    if fin.all():
        eps = np.finfo(dtype).eps
        gap = np.abs(y.astype(np.float64).sum(1) - mix[:, :L].astype(np.float64)).max()
        print(f"sum gap {gap:.3e} bound {4 * K * eps * np.abs(y).max():.3e}")
        assert gap <= 4 * K * eps * np.abs(y).max(), gap


# n_fft, hop, frames, B, K, extra stft kwargs, dtype, the kernel launch_geometry must report (None: not asserted)
GENERIC = [
    (512, 128, 12, 2, 3, {}, np.float32, "k_semi"),
    (2048, 512, 9, 1, 2, {}, np.float32, "k_semi"),
    (1024, 256, 10, 2, 4, {}, np.float32, "k_semi"),
    (256, 64, 19, 1, 3, dict(pad_mode="constant"), np.float32, "k_wave_iter"),
    (512, 128, 9, 1, 5, {}, np.float32, "k_semi"),                                      # K = 5: the loop
    (400, 160, 13, 1, 2, {}, np.float32, None),
    (512, 100, 11, 1, 3, dict(onesided=False, win_length=300), np.float32, "k_semi"),   # L = 1000
    (512, 128, 12, 2, 3, {}, np.float64, "k_wave_iter"),
    (1024, 256, 10, 1, 2, dict(onesided=False), np.float32, "k_semi"),
    (256, 64, 12, 1, 3, dict(center=False, rect=True), np.float32, "k_wave_iter"),      # the envelope does not vanish
    (256, 77, 10, 2, 4, {}, np.float32, "k_wave_iter"),                                 # L = 693: 4-byte accesses
    (256, 77, 10, 1, 5, {}, np.float64, "k_wave_iter"),                                 # ... 8-byte in float64, the loop
    (256, 50, 10, 1, 3, dict(win_length=200), np.float32, "k_wave_iter"),               # L = 450: 8-byte accesses
    (1000, 250, 7, 1, 2, {}, np.float64, None),
    (32768, 8192, 5, 1, 2, {}, np.float32, "k_iter_pair"),                              # kernels_big.h
]


@pytest.mark.parametrize("n_fft,hop,frames,B,K,extra,dtype,kernel", GENERIC)
def test_misi_matches_the_oracle(n_fft, hop, frames, B, K, extra, dtype, kernel):
    """3 iterations and an evaluating one from a random complex start, the plan's own routing for small problems."""
    clear_plan_cache()
    start, mix, L, kw = _case(n_fft, hop, frames, B, K, extra, dtype)
    p = _plan(start, kw, dtype)
    y, sums = _run(p, start, mix)
    assert kernel is None or p.launch_geometry["kernel"] == kernel, p.launch_geometry
    _check(y, sums, start, mix, L, kw, dtype)


# The float32 wave-level kernels with their chunk-walking forms switched on for small problems (conftest: chunked_kernel).  Frame
# counts: the smallest at which the planner cuts an item into two chunks - a chunk is at least 8 frames, 16 at hop = n_fft / 8,
# (n_fft - 1) // hop + 1 for k_hop - so that the chunk tails (fused kernels) and the mended seams (k_hop) are really exercised.
CHUNKED = [
    (1024, 256, 16, 2, 3, {}, "k_fused4", 2),
    (2048, 512, 16, 1, 2, {}, "k_fused4", 2),
    (512, 128, 16, 2, 4, {}, "k_fused", 2),
    (1024, 512, 16, 1, 5, {}, "k_fused", 2),                      # hop = n_fft / 2
    (2048, 256, 32, 1, 3, {}, "k_fused", 2),                      # hop = n_fft / 8
    (4096, 1024, 16, 1, 2, {}, "k_fused", 2),
    (1024, 256, 26, 1, 3, {}, "k_fused4", 3),                     # chunks of 8, 9, 9 frames
    (1024, 77, 28, 1, 3, {}, "k_hop", 2),                         # L = 2079
    (512, 100, 16, 2, 2, dict(win_length=300), "k_hop", 2),
    (1024, 300, 16, 1, 4, dict(onesided=False), "k_hop", 2),      # k_hop2
    (1024, 256, 7, 1, 3, {}, "k_fused4", 1),                      # one chunk: the fused kernel without tails
    (1024, 256, 5, 1, 3, {}, "k_hop", 1),                         # fewer than n_fft / hop + 2 frames: k_hop, one chunk, no seams
]


@pytest.mark.parametrize("n_fft,hop,frames,B,K,extra,kernel,chunks", CHUNKED)
def test_misi_on_every_fast_kernel_family(chunked_kernel, n_fft, hop, frames, B, K, extra, kernel, chunks):
    start, mix, L, kw = _case(n_fft, hop, frames, B, K, extra, np.float32)
    p = _plan(start, kw, np.float32)
    y, sums = _run(p, start, mix)
    geo = p.launch_geometry
    assert p.fast_path and geo["kernel"] == kernel and geo["chunks"] == chunks, geo
    _check(y, sums, start, mix, L, kw, np.float32)


def test_default_and_generic_paths_agree():
    start, mix, L, kw = _case(1024, 256, 12, 2, 3, {}, np.float32)
    out = {}
    for generic in (False, True):
        p = _plan(start, kw, np.float32, generic)
        out[generic], _ = _run(p, start, mix)
        assert p.fast_path != generic
    e = rel_l2(out[False], out[True])
    print(f"fast vs generic {e:.3e}")
    assert e <= TOL[np.float32], e


def test_skewed_chunk_triples_agree_with_the_generic_path():
    """n_fft 1024 / hop 256 on a full chip (3072 waves and more: 12-wave workgroups) walks skewed chunk triples; the coupling
    kernel has to find the same chunk boundaries.  Too large for the NumPy oracle within a test's seconds: against the coverage
    kernels, which keep no tails."""
    clear_plan_cache()
    start, mix, L, kw = _case(1024, 256, 384, 2, 4, {}, np.float32)
    start, mix = np.tile(start, (16, 1, 1, 1)), np.tile(mix, (16, 1))       # 128 items x 24 chunks of 16 frames = 3072 waves
    out = {}
    for generic in (False, True):
        p = _plan(start, kw, np.float32, generic)
        out[generic], _ = _run(p, start, mix, iters=2)
        if not generic:
            geo = p.launch_geometry
            assert geo["kernel"] == "k_fused4" and geo["waves_per_workgroup"] == 12 and geo["chunks"] % 3 == 0 and geo["waves"] >= 3072, geo
        del p
    e = rel_l2(out[False], out[True])
    print(f"skewed fused vs generic {e:.3e}")
    assert e <= TOL[np.float32], e
    eps = np.finfo(np.float32).eps
    assert np.abs(out[False].astype(np.float64).sum(1) - mix[:, :L]).max() <= 4 * 4 * eps * np.abs(out[False]).max()


def test_misi_leaves_griffin_lim_as_it_was(chunked_kernel):
    """gla_init + 3 iterations, a MISI run, gla_init + 3 iterations on one plan: the same bits, the same launch."""
    start, mix, L, kw = _case(1024, 256, 16, 2, 3, {}, np.float32)
    B, K, F, frames = start.shape
    p = _plan(start, kw, np.float32)
    flat = T_(start.reshape(B * K, F, frames))

    def gla():
        p.gla_init(flat, None, 0.99)
        p.iterate(3)
        return N(p.wave()), p.launch_geometry

    y0, g0 = gla()
    _run(p, start, mix)
    assert p.launch_geometry["kernel"] == "k_fused4"
    y1, g1 = gla()
    assert g0 == g1 and g0["kernel"].endswith("_td"), (g0, g1)     # Griffin-Lim is back on its signal-form kernel
    assert np.array_equal(y0, y1)


def test_c_abi_state_and_argument_errors():
    start, mix, L, kw = _case(512, 128, 8, 1, 3, {}, np.float32)
    p = _plan(start, kw, np.float32)
    lib, h = p.lib, p._h
    sums = (C.c_double * 4)()
    err = lambda: lib.specinv_last_error().decode()
    assert lib.specinv_misi_iterate(h, 1, 0, sums) == _lib.ESTATE and "specinv_misi_init" in err()
    assert lib.specinv_misi_run(h, 10, 5, 0.0, 0, None, None, None, _lib.EVAL_CB(), None) == _lib.ESTATE
    flat, mx = T_(start.reshape(3, 257, 8)), T_(mix)
    assert lib.specinv_misi_init(h, flat.data_ptr(), None, mx.data_ptr(), mx.shape[1], 2) == _lib.EINVAL and "multiple" in err()
    assert lib.specinv_misi_init(h, flat.data_ptr(), None, mx.data_ptr(), L - 1, 3) == _lib.EINVAL and "mix_stride" in err()
    assert lib.specinv_misi_iterate(h, 1, 0, sums) == _lib.ESTATE                     # the refused inits left no state behind
    p.misi_init(flat, None, mx, 3)
    for fn in (lib.specinv_gla_iterate, lib.specinv_admm_iterate):
        assert fn(h, 1, 0, sums) == _lib.ESTATE and "MISI" in err()
    p.gla_init(flat, None, 0.0)
    assert lib.specinv_misi_iterate(h, 1, 0, sums) == _lib.ESTATE


# ---- spectrogram_inversion_amd.misi -----------------------------------------------------------------------------------------
def test_api_magnitudes_start_from_the_mixture_phase():
    """float64: the start's phase is that of a computed spectrogram, and the angle of a weak bin amplifies the transform's rounding
    by 1 / |bin| - in float64 that stays far inside the gate."""
    start, mix, L, kw = _case(512, 128, 10, 2, 3, {}, np.float64)
    mag = np.abs(start)
    c0 = mo.mixture_phase_start(mag, mix, **kw)
    ref = mo.misi(c0, mix, 6, eva_iter=3, **kw)
    y = si.misi(T_(mag), T_(mix), max_iter=6, tol=0, eva_iter=3, verbose=False, hop_length=128, window=torch.from_numpy(kw["window"]))
    assert y.device.type == "cuda" and tuple(y.shape) == (2, 3, L)
    e = rel_l2(N(y), ref)
    print(f"api float64 {e:.3e}")
    assert e <= TOL[np.float64], e


def test_api_shapes_devices_and_truncation():
    start, mix, L, kw = _case(512, 128, 10, 1, 3, {}, np.float32)
    tk = dict(max_iter=5, tol=0, eva_iter=2, verbose=False, hop_length=128, window=torch.from_numpy(kw["window"]))
    y4 = si.misi(T_(start), T_(mix), **tk)
    y3 = si.misi(T_(start[0]), T_(mix[0]), **tk)
    assert tuple(y4.shape) == (1, 3, L) and tuple(y3.shape) == (3, L) and torch.equal(y4[0], y3)
    ycpu = si.misi(torch.from_numpy(start[0]), torch.from_numpy(mix[0]), **tk)                 # CPU in, CPU out
    assert ycpu.device.type == "cpu" and torch.equal(ycpu, y3.cpu())
    yshort = si.misi(T_(start[0]), T_(mix[0, :L].copy()), **tk)                               # samples beyond L are ignored
    assert torch.equal(yshort, y3)
    ref = mo.misi(start, mix, 5, eva_iter=2, **kw)
    assert rel_l2(N(y4), ref) <= TOL[np.float32]
    mag = np.abs(start[0])
    yh = si.misi(T_(mag).half(), T_(mix[0]).half(), **tk)                                     # narrow inputs: computed in float32
    assert yh.dtype == torch.float16 and tuple(yh.shape) == (3, L) and torch.isfinite(yh).all()


def test_api_tol_stops_at_the_oracles_iteration():
    start, mix, L, kw = _case(512, 128, 12, 1, 2, {}, np.float64, seed=7)
    trace = []
    mo.misi(start, mix, 60, tol=0.05, eva_iter=2, trace=trace, **kw)
    assert 2 <= len(trace) < 30, len(trace)                     # the rule fires before max_iter: the case means something
    ref = mo.misi(start, mix, 60, tol=0.05, eva_iter=2, **kw)
    y = si.misi(T_(start), T_(mix), max_iter=60, tol=0.05, eva_iter=2, verbose=False, hop_length=128,
                window=torch.from_numpy(kw["window"]))
    longer = mo.misi(start, mix, 2 * len(trace) + 2, eva_iter=2, **kw)
    e = rel_l2(N(y), ref)
    assert e <= TOL[np.float64] < rel_l2(longer, ref), (e, rel_l2(longer, ref))
