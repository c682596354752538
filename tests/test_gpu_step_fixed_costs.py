"""What a Griffin-Lim step does around its frame loop, bit for bit: the evaluation sums of a run with deferred read-back (every
evaluation's partial sums in a slab of their own, finished by one launch in read_deferred), the final waveform pass (k_wave_out:
rows + chunk tails in one kernel that leaves the plan's state alone) and the fused initial ISTFT with its spectrum requested a
frame ahead.  No tolerance anywhere: sums and samples are compared as bit patterns, the initial waveform and the shapes the
frame-loop fixture lacks (one item; waves that do not fill the last workgroup) against SHA-256 digests recorded from an earlier
build (tests/golden/step_fixed_costs.json, written by tools/record_step_fixed_costs.py; `commit` names the build).

The inputs are the small cases of tools/record_frame_loop_bits.py: 3 items, 24 iterations, at least two chunks per item, n_fft
2048 / hop 512 in every padding mode, 1024 / 256 and 2048 / 1024.  Needs an MI355X: `-m gpu`."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("chunked_kernel")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_step_fixed_costs as rec          # noqa: E402  (the entries and how one is run: the recorder's own)
sys.path.pop(0)

with open(rec.FIXTURE) as _fh:
    GOLD = json.load(_fh)

RUN_CASES = sorted(n for n, e in rec.ENTRIES.items() if e[4] and "@" not in n)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _rows(evals):
    return np.array(evals, dtype=np.float64).reshape(-1, 3)


def _same_rows(got, want, what):
    assert got.shape == want.shape and got.shape[0] > 0, (what, got.shape, want.shape)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (what, got, want)


def _run(p, mag, alpha, max_iter, eva_iter, watched):
    """a fresh run on plan `p`; watched: with a callback that never stops it (one finishing launch per evaluation)"""
    p.gla_init(None, mag, alpha)
    done, evals = p.run(max_iter, eva_iter, 0.0, "sc", callback=(lambda it, metric, loss: 0) if watched else None)
    assert done == max_iter and len(evals) == max_iter // eva_iter, (done, evals)
    return _rows(evals)


def test_fixture_covers_every_entry():
    assert sorted(GOLD["entries"]) == sorted(rec.ENTRIES) and GOLD["commit"]
    assert (GOLD["iterations"], GOLD["eva_iter"]) == (rec.ITERATIONS, rec.EVA_ITER)
    for name, e in GOLD["entries"].items():
        assert e["kernel"].endswith("_td") and e["chunks"] >= 2, (name, e)
    for name in ("2048_512@one_item", "1024_256@one_item"):
        e = GOLD["entries"][name]
        assert e["batch"] == 1 and e["waves"] % e["waves_per_workgroup"] != 0, (name, e)
    e = GOLD["entries"]["2048_512@chunks_of_4"]
    assert e["frames"] == 4 * e["chunks"], e            # NB + 1 = 4 frames per chunk at n_fft / hop = 4


@pytest.mark.parametrize("name", RUN_CASES)
def test_deferred_evaluation_sums_equal_watched_ones(name):
    """run(24, 5, 0) and run(12, 1, 0) - five and twelve slabs, one finishing launch - against the same runs watched by a callback"""
    p, mag, alpha = rec.make_plan(name)
    for max_iter, eva_iter in ((rec.ITERATIONS, rec.EVA_ITER), (12, 1)):
        deferred = _run(p, mag, alpha, max_iter, eva_iter, watched=False)
        watched = _run(p, mag, alpha, max_iter, eva_iter, watched=True)
        assert list(deferred[:, 0]) == [float((i + 1) * eva_iter - 1) for i in range(max_iter // eva_iter)], deferred
        _same_rows(deferred, watched, (name, max_iter, eva_iter))
    if name in GOLD["entries"] and "evals_sha256" in GOLD["entries"][name]:
        assert _sha(_run(p, mag, alpha, rec.ITERATIONS, rec.EVA_ITER, watched=False)) == GOLD["entries"][name]["evals_sha256"], name


def test_deferred_slabs_of_two_plans_run_alternately():
    """plans of 3 and of 5 items take turns: each one's slabs are its own and sized for its own launch"""
    small, mag_s, alpha = rec.make_plan("2048_512", batch=3)
    large, mag_l, _ = rec.make_plan("2048_512", batch=5)
    want_s = _run(small, mag_s, alpha, 12, 1, watched=True)
    want_l = _run(large, mag_l, alpha, 12, 1, watched=True)
    assert small.launch_geometry["waves"] != large.launch_geometry["waves"]
    for _ in range(2):
        _same_rows(_run(large, mag_l, alpha, 12, 1, watched=False), want_l, "5 items")
        _same_rows(_run(small, mag_s, alpha, 12, 1, watched=False), want_s, "3 items")
    _same_rows(_run(small, mag_s, alpha, rec.ITERATIONS, rec.EVA_ITER, watched=False),
               _run(small, mag_s, alpha, rec.ITERATIONS, rec.EVA_ITER, watched=True), "3 items, five slots after twelve")


@pytest.mark.parametrize("name", RUN_CASES + ["2048_512@one_item", "1024_256@one_item"])
def test_wave_leaves_the_state_alone(name):
    """wave() twice after 3 iterations: equal bits; 21 more iterations: the waveform of 24 uninterrupted ones.  (The last chunk of
    every item ends on the item's last frame; the `@one_item` entries run a batch of one.)"""
    p, mag, alpha = rec.make_plan(name)
    p.gla_init(None, mag, alpha)
    p.iterate(rec.ITERATIONS)
    whole = p.wave().cpu().numpy()
    p.gla_init(None, mag, alpha)
    p.iterate(3)
    first = p.wave().cpu().numpy()
    second = p.wave().cpu().numpy()
    assert np.isfinite(first).all() and np.array_equal(first.view(np.uint32), second.view(np.uint32)), name
    p.iterate(rec.ITERATIONS - 3)
    resumed = p.wave().cpu().numpy()
    assert not np.array_equal(first, resumed), name
    assert np.array_equal(resumed.view(np.uint32), whole.view(np.uint32)), name


@pytest.mark.parametrize("name", sorted(rec.ENTRIES))
def test_recorded_bits(name):
    """the initial ISTFT's waveform and, where the entry iterates, the final waveform and the evaluation rows against the digests"""
    want = GOLD["entries"][name]
    wave0, wave, evals, geo = rec.run_entry(name)
    assert (geo["kernel"], geo["chunks"], geo["waves"], geo["waves_per_workgroup"]) == \
        (want["kernel"], want["chunks"], want["waves"], want["waves_per_workgroup"]), (geo, want)
    assert wave0.shape[0] == want["batch"] and _sha(wave0) == want["initial_wave_sha256"], name
    if wave is not None:
        assert _sha(wave) == want["wave_sha256"], name
        assert _sha(evals) == want["evals_sha256"], name
