"""Admission of every case of tests/test_gpu_padded.py on the CPU: the oracle in float32 and in float64 on the zero-padded batches of
tests/_padded.py.  What the device tests then assert about silence is established here for the reference - finite results, dead
samples (covered by silent frames alone) and the all-silent item exactly 0, leading silence all zeros under RTISI_LA - and every
case's `noise32`, the per-item rel-L2 between the float32 and the float64 oracle, is within its cap.  The caps are conditions, not
measurements: 1e-5 from the complex start (measured <= 2.6e-6), 1e-3 from the magnitudes (<= 8e-4; a case beyond it takes 3
iterations at alpha 0.3, _padded.MAG_GENTLE), 5e-3 for RTISI_LA on the trailing-silence item.  A case over its cap is replaced in
_padded.CASES by another shape of its kernel family, never skipped and never given a wider gate."""
import numpy as np
import pytest

import _padded as pd
from oracle import metrics as om

f32, f64 = np.float32, np.float64


def _scaled():
    return [(k, m, q, s) for k, q, s in pd.SCALE_CASES for m in pd.SCALE_METHODS] + [(k, "gla", q, s) for k, q, s in pd.DEEP_CASES]


@pytest.mark.parametrize("name", list(pd.CASES) + list(pd.RTISI_CASES))
def test_the_input_is_what_it_says(name):
    c32, c64 = pd.case(name, f32), pd.case(name, f64)
    assert np.array_equal(c32.mag.astype(f64), c64.mag) and np.array_equal(c32.start.astype(np.complex128), c64.start)
    assert np.array_equal(c32.kw["window"].astype(f64), c64.kw["window"])
    hop = c32.kw["hop_length"]
    n_fft = len(c32.kw["window"])
    for b in (0, 1, 3):
        assert pd._runs(c32.silent[b]) >= n_fft / hop + 2
        assert not c32.mag[b][:, c32.silent[b]].any() and not c32.start[b][:, c32.silent[b]].any()
        assert not c32.x[b][c32.dead[b]].any()
    if name in pd.CASES and pd.CASES[name][5] == "generic":
        # the workgroup-level kernels transform frames 2k and 2k + 1 as one complex frame: some pair holds one silent frame
        live = c32.mag.max(1) > 0
        assert (live[:, 0:-1:2] != live[:, 1::2]).any()
    # the frames next to a silence boundary are not silent, and the quiet stretch sits at 2^-20 of the rest
    q0, q1 = c32.quiet
    inner = c32.x[2, q0 + n_fft:q1 - n_fft]
    assert 0 < np.abs(inner).max() < 2.0 ** -17 and np.abs(c32.x[2]).max() > 0.1


@pytest.mark.parametrize("name,method", pd.CASE_METHODS)
def test_the_oracle_on_padded_batches(name, method):
    _admit(name, method, -20, 1.0)


@pytest.mark.parametrize("name,method,quiet_pow,scale", _scaled())
def test_the_oracle_on_scaled_and_deep_quiet_batches(name, method, quiet_pow, scale):
    _admit(name, method, quiet_pow, scale)


def _admit(name, method, quiet_pow, scale):
    c = pd.case(name, f32, quiet_pow, scale)
    items = pd.items_of(method)
    noise, block = pd.measures(name, method, quiet_pow, scale)
    print(f"{name} {method} 2^{quiet_pow} x{scale:g}: noise32 {noise} block {block}")
    for dt in (f32, f64):
        y, _ = pd.reference(name, method, dt, quiet_pow, scale)
        assert y.shape == (len(items), c.length) and y.dtype == dt
        assert np.isfinite(y).all()                              # (center=False runs under a Hamming window: no 0 / 0)
        if 3 in items:
            assert not y[3].any()
        if method in pd.DEAD_ZERO:
            assert not y[c.dead[items]].any()
    live = [i for i in range(len(items)) if items[i] != 3]
    assert np.isfinite(noise[live]).all() and np.nanmax(noise) <= pd.CAP[method], (noise, pd.CAP[method])


def test_admm_does_leak_into_dead_samples():
    """why ADMM is not in DEAD_ZERO: its dual variable carries the first iterations' error into frames whose target is 0"""
    c = pd.case("512/128 semi", f32)
    y, _ = pd.reference("512/128 semi", "admm", f32)
    assert y[:3][c.dead[:3]].any() and not y[3].any()


@pytest.mark.parametrize("asym", [True, False], ids=["asymmetric", "symmetric"])
@pytest.mark.parametrize("name", list(pd.RTISI_CASES))
def test_the_rtisi_oracle_on_padded_batches(name, asym):
    c = pd.case(name, f32)
    for dt in (f32, f64):
        y = pd.rtisi_reference(name, asym, dt)
        assert y.shape == (pd.BATCH, c.length) and np.isfinite(y).all()
        assert not y[c.dead].any() and not y[3].any()
        assert not y[1].any()                   # leading silence: the recursion never leaves S = 0
        assert y[0].any() and y[2].any()
    if asym:
        noise, block = pd.rtisi_measures(name)
        print(f"{name}: noise32 {noise} block {block}")
        assert noise[0] <= pd.CAP["rtisi"], noise


def test_the_all_silent_batch_runs_to_max_iter_in_the_reference():
    """tol = 1e-6 on zero magnitudes: every evaluation's loss is 0, `init_loss` stays unset and the stop rule never fires
    (torch_specinv/methods.py:183-190); the metric of zero sums is what the device must report."""
    import oracle
    c = pd.case("512/128 semi", f32)
    mag = np.zeros_like(c.mag)
    trace = []
    with np.errstate(all="ignore"):
        y, st = oracle.griffin_lim(mag, max_iter=12, tol=1e-6, eva_iter=2, trace=trace, return_state=True, **c.kw)
    assert st["iters"] == 12 and len(trace) == 6 and not y.any()
    assert all(l2 == 0 and np.isnan(m) for _, m, l2 in trace)         # sc: log10(0) - log10(0)
    with np.errstate(all="ignore"):
        assert np.isnan(om.sc(mag, mag))
