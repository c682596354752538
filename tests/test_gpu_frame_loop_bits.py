"""The signal-form Griffin-Lim kernels (kernels_fast_td.h: k_fused4_td, k_fused_td<R, OV>, k_eval_td) bit for bit against outputs
recorded from an earlier build (tests/golden/frame_loop_bits.npz, written by tools/record_frame_loop_bits.py; its `meta` entry names
the commit).  Changes to the frame loop that only move registers, addresses or the packing of independent operations must leave
every sample and every evaluation sum where it was: no tolerance anywhere.

Per case: 3 items, 24 iterations at alpha 0.3 with an evaluation every 5 - the early (+ c0) launches, the late ones, four
evaluations and the launches that write x - on a shape of at least two chunks per item, so that the first frames of an item, interior
frames, the tail blocks and the chunk seams are all walked.  n_fft 2048 / hop 512 (two waves per SIMD) and 1024 / 256 (three) run
k_fused4_td, 2048 / 1024, 2048 / 256 and 512 / 128 the other overlaps of the same body; every padding mode; one plan made for a chip
of fewer compute units (other seams).  Needs an MI355X: `-m gpu`."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from _util import load_golden

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("chunked_kernel")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_frame_loop_bits as rec          # noqa: E402  (the cases and how one is run: the recorder's own)
sys.path.pop(0)

GOLD = load_golden("frame_loop_bits")
META = json.loads(str(GOLD["meta"]))


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_fixture_covers_every_case():
    assert sorted(META["cases"]) == sorted(rec.CASES) and META["commit"]
    assert (META["iterations"], META["eva_iter"], META["batch"]) == (rec.ITERATIONS, rec.EVA_ITER, rec.BATCH)
    for name, c in META["cases"].items():
        assert c["kernel"].endswith("_td") and c["chunks"] >= 2, (name, c)
    assert META["cases"]["2048_512_alpha0"]["equals_spectral_kernel"]


@pytest.mark.parametrize("name", sorted(rec.CASES))
def test_signal_form_kernels_keep_their_bits(name):
    want = META["cases"][name]
    wave, evals, geo = rec.run_case(name, want["frames"])
    # the launch the fixture was recorded on: the _td kernel, seams crossed
    assert geo["kernel"] == want["kernel"] and geo["kernel"].endswith("_td"), geo
    assert geo["chunks"] == want["chunks"] >= 2 and geo["waves"] == want["waves"], geo
    head = GOLD[name + "__head"]
    first = np.flatnonzero(wave[0, :64].view(np.uint32) != head.view(np.uint32))
    assert first.size == 0, (name, "item 0 differs from sample", int(first[0]), wave[0, first[:4]], head[first[:4]])
    assert _sha(wave) == want["wave_sha256"], name
    rows = GOLD[name + "__evals"]
    assert evals.shape == rows.shape and np.array_equal(evals.view(np.uint64), rows.view(np.uint64)), (name, evals, rows)
    assert _sha(evals) == want["evals_sha256"], name


def test_alpha_zero_equals_the_spectral_kernel():
    """Without momentum z_t = x_t and the c0 term is zero: k_fused4_td computes what k_fused4 does, bit for bit."""
    name = "2048_512_alpha0"
    frames = META["cases"][name]["frames"]
    wave, _, geo = rec.run_case(name, frames)
    spectral, _, sgeo = rec.run_case(name, frames, keep_state=True)
    assert geo["kernel"] == "k_fused4_td" and sgeo["kernel"] == "k_fused4", (geo, sgeo)
    assert np.array_equal(wave.view(np.uint32), spectral.view(np.uint32))
