"""The inputs, cases and measured figures that tests/test_wpe_host.py and tests/test_gpu_wpe.py share.

Input: complex Gaussian noise smoothed along the frames by an AR(1) filter with pole 0.8 (neighbouring frames correlate, as the
frames of a reverberant recording do), bin 1 silent when there are at least three bins.  Seeded per case.

A case is (name, (B, C, F, T), options): `taps`, `delay`, `n_iter`, `psd_context`, `power` (True: a seeded positive (F, T) array
is passed) and `zero_item` (that item of the batch is all zero).  The first four are the issue's prototype shapes; the rest
exercise the kernel's own edges, with TILE = 32 frames a tile and halo = delay + taps - 1:
T = TILE - 1, TILE, TILE + halo + 1; T < delay + taps; T <= delay; D = C taps = 1, 63 (C = 3), 64; the frame slices 8 / 4 / 2 / 1 of
the accumulation (block counts <= 32, <= 64, <= 128, more); two register blocks a thread (C 32, K 2: 264 blocks); the 16-frame
tile beyond 32 channels; psd_context 2; `power`; a batch of 3 with an all-zero item; F = 1; n_iter = 0.

D_MEASURED[name] = (d_Y, d_G, d_lam): the relative L2 distance between the oracle as written and the same oracle with the frame
sums reversed and a Cholesky solve (tests/_wpe_oracle.py: reverse=True), measured by test_wpe_host.py, which prints the table and
asserts that a fresh measurement is at most 4 times it.  The device tolerance is FACTOR x max(d, 2^-53): a tree-shaped
float64 sum and another elimination order move the result by a small multiple of what a reversed sum does, a distance below one
rounding of float64 says nothing, and an indexing or halo mistake shows at 1e-3 or above."""
import functools

import numpy as np

import _wpe_oracle as wo

TILE = 32
FACTOR = 100.0
FLOOR = 2.0 ** -53

_BASE = dict(taps=10, delay=3, n_iter=3, psd_context=0, power=False, zero_item=None)


def _case(name, shape, **kw):
    return name, shape, dict(_BASE, **kw)


CASES = [
    _case("proto_c1", (1, 1, 5, 70), taps=10, delay=3, n_iter=3),
    _case("proto_c2", (1, 2, 5, 70), taps=8, delay=2, n_iter=3),
    _case("proto_c4_d64", (1, 4, 3, 150), taps=16, delay=1, n_iter=2),
    _case("proto_few_frames", (1, 1, 3, 9), taps=10, delay=3, n_iter=2),
    _case("t_tile_minus_1", (1, 2, 2, TILE - 1), taps=4, delay=2, n_iter=2),
    _case("t_tile", (1, 2, 2, TILE), taps=4, delay=2, n_iter=2),
    _case("t_tile_halo_1", (1, 2, 2, TILE + 5 + 1), taps=4, delay=2, n_iter=2),
    _case("t_le_delay", (1, 1, 2, 3), taps=2, delay=3, n_iter=2),
    _case("d1", (1, 1, 2, 40), taps=1, delay=1, n_iter=2),
    _case("d63_c3", (1, 3, 2, 100), taps=21, delay=2, n_iter=2),
    _case("slices4_d28", (1, 2, 2, 60), taps=14, delay=1, n_iter=2),
    _case("slices2_d40", (1, 4, 2, 60), taps=10, delay=3, n_iter=2),
    _case("two_blocks_c32", (1, 32, 1, 150), taps=2, delay=1, n_iter=1),
    _case("wide_tile_c33", (1, 33, 1, 40), taps=1, delay=1, n_iter=2),
    _case("context2", (1, 2, 3, 70), taps=5, delay=2, n_iter=3, psd_context=2),
    _case("power_given", (1, 2, 3, 50), taps=5, delay=2, n_iter=2, power=True),
    _case("batch3_zero_item", (3, 2, 3, 45), taps=4, delay=2, n_iter=2, zero_item=1),
    _case("f1", (1, 2, 1, 50), taps=4, delay=3, n_iter=2),
    _case("n_iter0", (1, 2, 2, 20), taps=3, delay=2, n_iter=0),
]
NAMES = [c[0] for c in CASES]
BY_NAME = {c[0]: c for c in CASES}

# measured by tests/test_wpe_host.py::test_order_sensitivity_table (it prints this dictionary)
D_MEASURED = {
    "proto_c1": (2.9e-09, 1.0e-08, 1.3e-12),   # (1, 5, 70, 10, 3, 3), cond(R) 2.9e+08: one channel's own |y_t|^2 nears 0 at some frames
    "proto_c2": (3.9e-13, 8.2e-13, 9.6e-15),   # (2, 5, 70, 8, 2, 3), cond(R) 4.1e+04
    "proto_c4_d64": (1.3e-14, 2.1e-14, 6.2e-15),   # (4, 3, 150, 16, 1, 2), cond(R) 9.2e+02
    "proto_few_frames": (1.2e-14, 3.5e-14, 0.0e+00),   # (1, 3, 9, 10, 3, 2), cond(R) 8.4e+10
    "t_tile_minus_1": (3.1e-15, 6.5e-15, 9.2e-16),   # (2, 2, 31, 4, 2, 2), cond(R) 1.6e+02
    "t_tile": (1.7e-15, 4.0e-15, 8.2e-16),   # (2, 2, 32, 4, 2, 2), cond(R) 7.8e+01
    "t_tile_halo_1": (3.8e-15, 8.9e-15, 8.6e-16),   # (2, 2, 38, 4, 2, 2), cond(R) 2.6e+02
    "t_le_delay": (0.0e+00, 0.0e+00, 0.0e+00),   # (1, 2, 3, 2, 3, 2), cond(R) 1.0e+00
    "d1": (2.0e-16, 2.3e-16, 0.0e+00),   # (1, 2, 40, 1, 1, 2), cond(R) 1.0e+00
    "d63_c3": (1.5e-13, 2.8e-13, 2.1e-14),   # (3, 2, 100, 21, 2, 2), cond(R) 2.6e+04
    "slices4_d28": (1.8e-14, 2.9e-14, 6.6e-15),   # (2, 2, 60, 14, 1, 2), cond(R) 1.1e+03
    "slices2_d40": (8.2e-14, 1.1e-13, 1.2e-14),   # (4, 2, 60, 10, 3, 2), cond(R) 1.6e+04
    "two_blocks_c32": (7.3e-15, 1.0e-14, 0.0e+00),   # (32, 1, 150, 2, 1, 1), cond(R) 1.7e+02
    "wide_tile_c33": (8.5e-14, 1.1e-13, 8.4e-15),   # (33, 1, 40, 1, 1, 2), cond(R) 6.2e+03
    "context2": (1.8e-15, 4.5e-15, 9.7e-16),   # (2, 3, 70, 5, 2, 3), cond(R) 6.4e+01
    "power_given": (2.6e-15, 5.5e-15, 1.4e-15),   # (2, 3, 50, 5, 2, 2), cond(R) 7.8e+01
    "batch3_zero_item": (3.5e-15, 7.9e-15, 1.8e-15),   # (2, 3, 45, 4, 2, 2), cond(R) 2.4e+02
    "f1": (1.2e-15, 3.8e-15, 5.7e-16),   # (2, 1, 50, 4, 3, 2), cond(R) 6.0e+01
    "n_iter0": (0.0e+00, 0.0e+00, 0.0e+00),   # (2, 2, 20, 3, 2, 0), cond(R) 1.0e+00
}


def make_input(name):
    """X (B, C, F, T) complex128 of a case."""
    _, (B, C, F, T), opt = BY_NAME[name]
    rng = np.random.default_rng(1000 + NAMES.index(name))
    e = rng.standard_normal((B, C, F, T)) + 1j * rng.standard_normal((B, C, F, T))
    X = np.empty_like(e)
    acc = np.zeros((B, C, F), dtype=np.complex128)
    for t in range(T):
        acc = 0.8 * acc + e[..., t]
        X[..., t] = acc
    if F >= 3:
        X[:, :, 1, :] = 0.0
    if opt["zero_item"] is not None:
        X[opt["zero_item"]] = 0.0
    return X


def make_power(name):
    _, (B, C, F, T), opt = BY_NAME[name]
    if not opt["power"]:
        return None
    rng = np.random.default_rng(5000 + NAMES.index(name))
    return 0.5 + rng.random((F, T))


def oracle_options(name):
    opt = BY_NAME[name][2]
    return dict(taps=opt["taps"], delay=opt["delay"], n_iter=opt["n_iter"], psd_context=opt["psd_context"], power=make_power(name))


@functools.lru_cache(maxsize=None)
def oracle(name, single=False, reverse=False):
    """(Y, G, lam) of the case over its items, float64; `single`: on the input rounded to complex64 first.  Computed once and
    shared; callers must not write into it."""
    X = make_input(name)
    if single:
        X = X.astype(np.complex64)
    res = wo.wpe_batch(X, reverse=reverse, **oracle_options(name))
    for r in res:
        r.setflags(write=False)
    return res


def rel_l2(a, b):
    den = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / den) if den > 0 else float(np.linalg.norm(a - b))


def tolerances(name):
    """(tol_Y, tol_G, tol_lam), relative L2, for the device against the oracle."""
    return tuple(FACTOR * max(d, FLOOR) for d in D_MEASURED[name])
