"""AGLA's step kernels (kernels_agla.h: k_agla_step) and their adjoints (kernels_agla_adjoint.h: k_agla_step_adjoint), with and
without a constraint, bit for bit against outputs recorded from an earlier build (tests/golden/agla_step_bits.npz, written by
tools/record_agla_step_bits.py; its `meta` entry names the commit).  A change that only moves code - one kernel body for the
constrained and the unconstrained step, one launcher - must leave every sample, every cotangent and every inner product where it
was: no tolerance anywhere.

Forward: a complex start, no constraint / an offset alone (the mask pointer is NULL) / an offset and a mask with odd edges, five
iterations with the result read after each, gamma = 1 and the general scheme, the 16- / 8- / 4-byte accesses in both dtypes and
the three chunk-walking float32 kernel families (chunk tails beside the state).  Adjoint: the shapes and random inputs of
tests/test_gpu_cgla_unfolded.py through `agla_extrap_adjoint`, `cgla_extrap_adjoint` without and with a mask, n = 2 and 3, and the
closing arm through both `*_first_adjoint`.  Needs an MI355X: `-m gpu`."""
import json
import os
import sys

import numpy as np
import pytest

from _util import load_golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_agla_step_bits as rec          # noqa: E402  (the cases and how one is run: the recorder's own)
sys.path.pop(0)

GOLD = load_golden("agla_step_bits")
META = json.loads(str(GOLD["meta"]))
PACKED = {"float32": GOLD["f32"], "float64": GOLD["f64"]}
UINT = {"float32": np.uint32, "float64": np.uint64}


def _compare(name, arrays, keep):
    want = META["cases"][name]
    assert len(keep) == len(want["kept"]), name
    for k, (a, (dt, at, n)) in enumerate(zip(rec.kept(keep), want["kept"])):
        assert a.dtype.name == dt and a.size == n, (name, k, a.dtype, a.size)
        gold = PACKED[dt][at: at + n]
        first = np.flatnonzero(a.view(UINT[dt]) != gold.view(UINT[dt]))
        assert first.size == 0, (name, "array", k, "differs from element", int(first[0]), a[first[:4]], gold[first[:4]])
    assert rec.digest(arrays) == want["sha256"], name


def test_fixture_covers_every_case():
    names = [rec.forward_name(c) for c in rec.FORWARD] + [rec.adjoint_name(c) for c in rec.ADJOINT]
    assert sorted(META["cases"]) == sorted(names) and len(set(names)) == len(names) and META["commit"]
    assert (META["iters"], META["head"]) == (rec.ITERS, rec.HEAD)
    for c in rec.FORWARD:
        want, got = rec.SHAPES[c[0]][6], META["cases"][rec.forward_name(c)]
        assert want is None or (got["kernel"] == want[0] and got["chunks"] >= want[1] >= 2), (c, got)


@pytest.mark.parametrize("case", rec.FORWARD, ids=rec.forward_name)
def test_forward_step_keeps_its_bits(case, request):
    if rec.SHAPES[case[0]][6] is not None:
        request.getfixturevalue("chunked_kernel")
    name = rec.forward_name(case)
    arrays, keep, geo = rec.forward_outputs(case)
    want = META["cases"][name]
    assert geo["kernel"] == want["kernel"] and geo["chunks"] == want["chunks"], geo      # the launch the fixture was recorded on
    _compare(name, arrays, keep)


@pytest.mark.parametrize("case", rec.ADJOINT, ids=rec.adjoint_name)
def test_adjoint_step_keeps_its_bits(case):
    arrays, keep, _ = rec.adjoint_outputs(case)
    _compare(rec.adjoint_name(case), arrays, keep)
