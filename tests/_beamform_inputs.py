"""The inputs, cases and measured figures that tests/test_beamform_host.py and tests/test_gpu_beamform.py share.

Input: a seeded scene X = a s_t + n_t per item and bin - a complex steering vector `a` over the channels, a complex Gaussian
source that is on in about half the frames, and white complex Gaussian noise at 0.3 of the source's amplitude.  The target mask is
the ideal ratio mask |s|^2 / (|s|^2 + sigma^2) plus Gaussian noise of deviation 0.1, clipped to [0, 1].  Bin 1 is silent when
there are at least three bins.

A case is (name, (B, C, F, T), options) for one solution; `SHAPES` lists the shapes with the solutions each is run for, the name
is "<shape>-<solution>".  Options: `ref` (the reference channel), `noise_given` (a seeded mask_noise is passed instead of None),
`mask` ("full": (F, T); "profile": a broadcast (F, 1) mask; "zero": all zero), `zero_item` (that item of the batch is all zero),
`diag_load`, `n_power_iter`, `mu`.  The shapes exercise the kernel's own edges, with TILE = 64 frames a tile:
T = 1, TILE - 1, TILE, TILE + 1, 2 TILE + 2; C = 1, 2, 3 (not a power of two), 8, 9 (the first size with more than one entry a
lane) and 16 (the limit); fewer frames than channels (8 channels x 5 frames, 16 x 3: rank-deficient covariances, carried by the
loading); F = 1; ref = C - 1; mask_noise given; a broadcast mask; an all-zero mask; a batch of 3 with an all-zero item;
diag_load = 0 on a well-conditioned case; n_power_iter 1 and 5; mu 0 and 4.

D_MEASURED[name] = (d_Y, d_w, d_Phi): the relative L2 distance between the oracle as written and the same oracle with the frame
sums reversed and a Cholesky solve (tests/_beamform_oracle.py: reverse=True; d_Phi the larger of Phi_s's and Phi_n's), measured by
test_beamform_host.py, which prints the table and asserts that a fresh measurement is at most 4 times it.  The device tolerance is
FACTOR x max(d, 2^-53): a tree-shaped float64 sum and another elimination order move the result by a small multiple of what a
reversed sum does, a distance below one rounding of float64 says nothing, and an indexing mistake shows at 1e-3 or above."""
import functools

import numpy as np

import _beamform_oracle as bo

TILE = 64
FACTOR = 100.0
FLOOR = 2.0 ** -53

_BASE = dict(ref=0, noise_given=False, mask="full", zero_item=None, diag_load=1e-7, n_power_iter=3, mu=1.0)
_ALL = bo.SOLUTIONS

# (shape name, (B, C, F, T), solutions, options)
SHAPES = [
    ("t1", (1, 2, 2, 1), _ALL, {}),
    ("t_tile_minus_1", (1, 2, 2, TILE - 1), _ALL, {}),
    ("t_tile", (1, 2, 2, TILE), _ALL, {}),
    ("t_tile_plus_1_c3", (1, 3, 2, TILE + 1), _ALL, {}),
    ("t_two_tiles_c4", (1, 4, 3, 2 * TILE + 2), _ALL, {}),
    ("c1", (1, 1, 3, 70), _ALL, {}),
    ("c8", (1, 8, 2, 70), _ALL, {}),
    ("c9", (1, 9, 2, 70), _ALL, {}),
    ("c16", (1, 16, 2, 100), _ALL, {}),
    ("c8_t5", (1, 8, 2, 5), _ALL, {}),
    ("c16_t3", (1, 16, 1, 3), _ALL, {}),
    ("f1", (1, 2, 1, 50), _ALL, {}),
    ("ref_last", (1, 4, 3, 40), _ALL, dict(ref=3)),
    ("noise_given", (1, 3, 3, 50), _ALL, dict(noise_given=True)),
    ("mask_profile", (1, 3, 3, 50), _ALL, dict(mask="profile")),
    ("zero_mask", (1, 2, 2, 40), _ALL, dict(mask="zero")),
    ("batch3_zero_item", (3, 2, 3, 45), _ALL, dict(zero_item=1)),
    ("diag_load0", (1, 3, 2, 80), _ALL, dict(diag_load=0.0)),
    ("power_iter1", (1, 4, 2, 60), ("rtf_power",), dict(n_power_iter=1)),
    ("power_iter5", (1, 4, 2, 60), ("rtf_power",), dict(n_power_iter=5)),
    ("mu0", (1, 3, 2, 80), ("mwf",), dict(mu=0.0)),
    ("mu4", (1, 3, 2, 80), ("mwf",), dict(mu=4.0)),
]
_SHAPE_NAMES = [s[0] for s in SHAPES]

CASES = [(f"{sname}-{sol}", shape, dict(_BASE, solution=sol, shape_name=sname, **opt))
         for sname, shape, sols, opt in SHAPES for sol in sols]
NAMES = [c[0] for c in CASES]
BY_NAME = {c[0]: c for c in CASES}

# measured by tests/test_beamform_host.py::test_order_sensitivity_table (it prints this dictionary)
D_MEASURED = {
    "t1-souden": (2.4e-10, 2.2e-09, 0.0e+00),   # (1, 2, 2, 1): one frame, two channels - the loading carries the solve
    "t1-rtf_power": (1.2e-16, 2.2e-09, 0.0e+00),   # (1, 2, 2, 1)
    "t1-mwf": (8.5e-17, 4.2e-10, 0.0e+00),   # (1, 2, 2, 1)
    "t_tile_minus_1-souden": (1.8e-16, 1.7e-16, 3.7e-16),   # (1, 2, 2, 63)
    "t_tile_minus_1-rtf_power": (2.5e-16, 3.2e-16, 3.7e-16),   # (1, 2, 2, 63)
    "t_tile_minus_1-mwf": (3.4e-16, 8.7e-16, 3.7e-16),   # (1, 2, 2, 63)
    "t_tile-souden": (1.9e-16, 3.2e-16, 4.2e-16),   # (1, 2, 2, 64)
    "t_tile-rtf_power": (1.6e-16, 3.1e-16, 4.2e-16),   # (1, 2, 2, 64)
    "t_tile-mwf": (3.4e-16, 4.6e-16, 4.2e-16),   # (1, 2, 2, 64)
    "t_tile_plus_1_c3-souden": (6.2e-16, 1.0e-15, 3.8e-16),   # (1, 3, 2, 65)
    "t_tile_plus_1_c3-rtf_power": (3.6e-16, 1.1e-15, 3.8e-16),   # (1, 3, 2, 65)
    "t_tile_plus_1_c3-mwf": (9.5e-16, 3.3e-15, 3.8e-16),   # (1, 3, 2, 65)
    "t_two_tiles_c4-souden": (1.4e-15, 1.9e-15, 6.3e-16),   # (1, 4, 3, 130)
    "t_two_tiles_c4-rtf_power": (5.0e-16, 1.3e-15, 6.3e-16),   # (1, 4, 3, 130)
    "t_two_tiles_c4-mwf": (1.2e-15, 4.6e-15, 6.3e-16),   # (1, 4, 3, 130)
    "c1-souden": (1.2e-16, 7.9e-17, 2.8e-16),   # (1, 1, 3, 70)
    "c1-rtf_power": (0.0e+00, 3.0e-33, 2.8e-16),   # (1, 1, 3, 70)
    "c1-mwf": (1.4e-16, 1.3e-16, 2.8e-16),   # (1, 1, 3, 70)
    "c8-souden": (1.0e-15, 1.8e-15, 5.5e-16),   # (1, 8, 2, 70)
    "c8-rtf_power": (2.5e-16, 9.1e-16, 5.5e-16),   # (1, 8, 2, 70)
    "c8-mwf": (1.9e-15, 5.6e-15, 5.5e-16),   # (1, 8, 2, 70)
    "c9-souden": (5.3e-16, 1.4e-15, 3.7e-16),   # (1, 9, 2, 70)
    "c9-rtf_power": (4.5e-16, 1.6e-15, 3.7e-16),   # (1, 9, 2, 70)
    "c9-mwf": (1.1e-15, 2.7e-15, 3.7e-16),   # (1, 9, 2, 70)
    "c16-souden": (7.7e-16, 3.7e-15, 3.9e-16),   # (1, 16, 2, 100)
    "c16-rtf_power": (6.6e-16, 2.9e-15, 3.9e-16),   # (1, 16, 2, 100)
    "c16-mwf": (2.4e-15, 8.8e-15, 3.9e-16),   # (1, 16, 2, 100)
    "c8_t5-souden": (7.4e-10, 2.7e-09, 1.2e-16),   # (1, 8, 2, 5): rank 5 of 8, the loading of 1e-7 carries the rest
    "c8_t5-rtf_power": (2.1e-15, 2.6e-09, 1.2e-16),   # (1, 8, 2, 5)
    "c8_t5-mwf": (1.1e-15, 3.0e-09, 1.2e-16),   # (1, 8, 2, 5)
    "c16_t3-souden": (1.0e-09, 6.6e-09, 7.9e-17),   # (1, 16, 1, 3): rank 3 of 16
    "c16_t3-rtf_power": (1.0e-15, 8.6e-09, 7.9e-17),   # (1, 16, 1, 3)
    "c16_t3-mwf": (2.4e-16, 6.3e-09, 7.9e-17),   # (1, 16, 1, 3)
    "f1-souden": (3.0e-16, 6.1e-16, 2.7e-16),   # (1, 2, 1, 50)
    "f1-rtf_power": (2.3e-16, 6.9e-16, 2.7e-16),   # (1, 2, 1, 50)
    "f1-mwf": (1.8e-16, 3.7e-16, 2.7e-16),   # (1, 2, 1, 50)
    "ref_last-souden": (1.1e-15, 2.8e-15, 3.1e-16),   # (1, 4, 3, 40)
    "ref_last-rtf_power": (5.0e-16, 1.9e-15, 3.1e-16),   # (1, 4, 3, 40)
    "ref_last-mwf": (7.4e-16, 2.8e-15, 3.1e-16),   # (1, 4, 3, 40)
    "noise_given-souden": (2.2e-16, 5.3e-16, 4.4e-16),   # (1, 3, 3, 50)
    "noise_given-rtf_power": (3.0e-16, 6.8e-16, 4.4e-16),   # (1, 3, 3, 50)
    "noise_given-mwf": (5.0e-16, 1.2e-15, 4.4e-16),   # (1, 3, 3, 50)
    "mask_profile-souden": (4.8e-16, 1.3e-15, 2.4e-16),   # (1, 3, 3, 50)
    "mask_profile-rtf_power": (2.9e-15, 7.3e-15, 2.4e-16),   # (1, 3, 3, 50)
    "mask_profile-mwf": (6.2e-16, 1.5e-15, 2.4e-16),   # (1, 3, 3, 50)
    "zero_mask-souden": (0.0e+00, 0.0e+00, 2.7e-16),   # (1, 2, 2, 40)
    "zero_mask-rtf_power": (0.0e+00, 0.0e+00, 2.7e-16),   # (1, 2, 2, 40)
    "zero_mask-mwf": (0.0e+00, 0.0e+00, 2.7e-16),   # (1, 2, 2, 40)
    "batch3_zero_item-souden": (4.8e-16, 4.3e-16, 3.4e-16),   # (3, 2, 3, 45)
    "batch3_zero_item-rtf_power": (2.2e-16, 3.4e-16, 3.4e-16),   # (3, 2, 3, 45)
    "batch3_zero_item-mwf": (3.3e-16, 7.2e-16, 3.4e-16),   # (3, 2, 3, 45)
    "diag_load0-souden": (6.2e-16, 1.1e-15, 5.6e-16),   # (1, 3, 2, 80)
    "diag_load0-rtf_power": (4.1e-16, 1.4e-15, 5.6e-16),   # (1, 3, 2, 80)
    "diag_load0-mwf": (8.2e-16, 3.7e-15, 5.6e-16),   # (1, 3, 2, 80)
    "power_iter1-rtf_power": (5.0e-16, 1.4e-15, 3.2e-16),   # (1, 4, 2, 60)
    "power_iter5-rtf_power": (2.4e-16, 4.8e-16, 3.3e-16),   # (1, 4, 2, 60)
    "mu0-mwf": (5.3e-16, 7.7e-16, 6.0e-16),   # (1, 3, 2, 80)
    "mu4-mwf": (4.5e-16, 2.6e-15, 5.4e-16),   # (1, 3, 2, 80)
}


def _rng(name, salt):
    return np.random.default_rng(salt + _SHAPE_NAMES.index(BY_NAME[name][2]["shape_name"]))


@functools.lru_cache(maxsize=None)
def _scene(shape_name):
    name = next(n for n in NAMES if BY_NAME[n][2]["shape_name"] == shape_name)
    _, (B, C, F, T), opt = BY_NAME[name]
    rng = _rng(name, 2000)
    cg = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)) / np.sqrt(2.0)      # noqa: E731
    a = cg(B, C, F, 1)
    on = (rng.random((B, 1, 1, T)) < 0.5) | (T == 1)
    s = cg(B, 1, F, T) * on
    sigma = 0.3
    X = a * s + sigma * cg(B, C, F, T)
    irm = np.abs(s[:, 0]) ** 2 / (np.abs(s[:, 0]) ** 2 + sigma ** 2)
    mt = np.clip(irm + 0.1 * rng.standard_normal((B, F, T)), 0.0, 1.0)
    mn = np.clip(1.0 - irm + 0.1 * rng.standard_normal((B, F, T)), 0.0, 1.0)
    if F >= 3:
        X[:, :, 1, :] = 0.0
    if opt["zero_item"] is not None:
        X[opt["zero_item"]] = 0.0
    if opt["mask"] == "profile":
        mt = mt[..., :1].copy()
    elif opt["mask"] == "zero":
        mt = np.zeros_like(mt)
    if B == 1:
        mt, mn = mt[0], mn[0]                   # (F, T): no batch axis
    for arr in (X, mt, mn):
        arr.setflags(write=False)
    return X, mt, (mn if opt["noise_given"] else None)


def make_input(name):
    """X (B, C, F, T) complex128 of a case (read-only, shared)."""
    return _scene(BY_NAME[name][2]["shape_name"])[0]


def make_masks(name):
    """(mask_target, mask_noise or None): float64, (F, T) - (F, 1) for the profile case - or (B, F, T) for a batch."""
    return _scene(BY_NAME[name][2]["shape_name"])[1:]


def oracle_options(name):
    opt = BY_NAME[name][2]
    return dict(solution=opt["solution"], ref=opt["ref"], diag_load=opt["diag_load"], n_power_iter=opt["n_power_iter"], mu=opt["mu"])


@functools.lru_cache(maxsize=None)
def oracle(name, single=False, reverse=False):
    """(Y, w, Phi_s, Phi_n) of the case over its items, float64; `single`: on the input rounded to complex64 first.  Computed once
    and shared; callers must not write into it."""
    X = make_input(name)
    if single:
        X = X.astype(np.complex64)
    mt, mn = make_masks(name)
    res = bo.beamform_batch(X, mt, mn, reverse=reverse, **oracle_options(name))
    for r in res:
        r.setflags(write=False)
    return res


def rel_l2(a, b):
    den = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / den) if den > 0 else float(np.linalg.norm(a - b))


def measure(name):
    """(d_Y, d_w, d_Phi) of a case, fresh."""
    a, b = oracle(name), oracle(name, reverse=True)
    d = [rel_l2(y, x) for x, y in zip(a, b)]
    return d[0], d[1], max(d[2], d[3])


def tolerances(name):
    """(tol_Y, tol_w, tol_Phi), relative L2, for the device against the oracle."""
    return tuple(FACTOR * max(d, FLOOR) for d in D_MEASURED[name])
