#!/usr/bin/env python3
"""Records what AGLA's step kernels (kernels_agla.h: k_agla_step) and their adjoints (kernels_agla_adjoint.h: k_agla_step_adjoint)
compute, with and without a constraint, for tests/test_gpu_agla_step_bits.py.

    python tools/record_agla_step_bits.py <commit the library was built from> [out.npz]

Run it ONCE, on the build whose bits are to be kept (the parent of a change that must not move them), on an MI355X.  Every case is
run twice and the two runs must agree; `meta` names the commit.  The test imports the case lists, run_forward and run_adjoint from
here, so that both sides run the same inputs; it never regenerates the fixture.

Per case the fixture holds one SHA-256 over every output array (each array's bytes, in the order the case returns them): that is the
comparison of every value.  Beside it, for reading a failure: every array of at most 64 elements in full, the first 64 values of a
larger one; the three inner products of an adjoint case always.  The stored values are packed into one array per dtype (`f32`,
`f64`), `meta` holds where each case's values lie.

Forward: agla_init_sched from a complex start, an optional agla_constrain, 5 x agla_iterate(1) with wave() after each - t_2
already depends on the c_1 written to the state.  Adjoint: the random inputs and the odd-edged mask of
tests/test_gpu_cgla_unfolded.py (_extrap_case, _odd_mask, test_the_closing_arm), restated here."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "agla_step_bits.npz")
ITERS, HEAD = 5, 64
TDT = {"float32": torch.float32, "float64": torch.float64}

# name: n_fft, hop, frames, batch, win_length, dtype, (kernel, chunks at least) of a chunked case or None
SHAPES = {
    "256_64_f32": (256, 64, 12, 3, 256, "float32", None),           # L = 704: 16-byte accesses
    "256_64_f64": (256, 64, 12, 3, 256, "float64", None),
    "256_50_f32": (256, 50, 10, 3, 200, "float32", None),           # L = 450: 8-byte
    "256_77_f32": (256, 77, 10, 3, 256, "float32", None),           # L = 693: 4-byte
    "256_77_f64": (256, 77, 10, 3, 256, "float64", None),           # ... 8-byte
    "1024_256_fused4": (1024, 256, 16, 6, 1024, "float32", ("k_fused4", 2)),   # chunk tails
    "512_128_fused": (512, 128, 16, 8, 512, "float32", ("k_fused", 2)),
    "1024_77_hop": (1024, 77, 28, 3, 1024, "float32", ("k_hop", 2)),           # L = 2079
}
PARAMS = {"fgla": (0.99, 0.99, 1.0), "general": (0.5, 1.2, 0.7)}
CONSTRAINTS = ("none", "offset", "offset_mask")
FORWARD = [(s, p, c) for s in SHAPES for p in PARAMS for c in CONSTRAINTS]

# hop, frames, batch at n_fft 16: tests/test_gpu_cgla_unfolded.py's EXTRAP
EXTRAP = [(4, 4, 1), (6, 4, 3), (5, 4, 3), (8, 301, 5)]
ROUTES = ("agla", "cgla_null_mask", "cgla_mask")
# (hop, frames, batch), dtype, n (1: the closing arm through *_first_adjoint), general, route
ADJOINT = [(e, d, n, g, r) for e in EXTRAP for d in ("float32", "float64") for n in (2, 3, 1) for g in (True, False) for r in ROUTES]


def forward_name(case):
    return "fwd/" + "/".join(case)


def adjoint_name(case):
    (hop, frames, batch), dtype, n, general, route = case
    return f"adj/{hop}_{frames}_{batch}/{dtype}/n{n}/{'general' if general else 'fgla'}/{route}"


def hann(n, dtype):
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)).astype(dtype)


def odd_mask(B, L):
    """Known samples whose edges fall at odd indices, inside a thread's vector, shifted from item to item"""
    W = np.zeros((B, L), bool)
    for b in range(B):
        W[b, : (L // 3 | 1) + 2 * (b % 2)] = True
        lo = (L // 2 | 1)
        W[b, lo: lo + 3 + 2 * b] = True
    return W


def make_plan(n_fft, hop, frames, batch, win_length, dtype, chunked, device):
    from spectrogram_inversion_amd.plan import Plan, args_helper
    cd = torch.complex64 if dtype == "float32" else torch.complex128
    a = args_helper(torch.empty((1, n_fft // 2 + 1, 1), dtype=cd), hop_length=hop, win_length=win_length,
                    window=torch.from_numpy(hann(win_length, dtype)))
    # small problems normally go to the one-frame-per-wave kernel: SPECINV_SMALL_FRAMES=0 puts them on the chunk-walking ones
    old = os.environ.get("SPECINV_SMALL_FRAMES")
    try:
        os.environ.pop("SPECINV_SMALL_FRAMES", None)
        if chunked:
            os.environ["SPECINV_SMALL_FRAMES"] = "0"
        return Plan(a, batch, frames, TDT[dtype], device)
    finally:
        os.environ.pop("SPECINV_SMALL_FRAMES", None)
        if old is not None:
            os.environ["SPECINV_SMALL_FRAMES"] = old


def run_forward(case, device=None):
    """-> ([wave after iteration 1 .. ITERS], launch geometry) of the forward case (shape, params, constraint)"""
    shape, params, constraint = case
    n_fft, hop, frames, batch, win_length, dtype, chunked = SHAPES[shape]
    device = torch.device("cuda", 0) if device is None else device
    rng = np.random.default_rng(n_fft + hop + frames)
    p = make_plan(n_fft, hop, frames, batch, win_length, dtype, chunked is not None, device)
    F = n_fft // 2 + 1
    start = (rng.standard_normal((batch, F, frames)) + 1j * rng.standard_normal((batch, F, frames)))
    start = start.astype(np.complex64 if dtype == "float32" else np.complex128)
    off = (0.25 * rng.standard_normal((batch, p.length))).astype(dtype)
    alpha, beta, gamma = PARAMS[params]
    p.agla_init_sched(torch.from_numpy(start).to(device), None, [alpha], [beta], [gamma])
    if constraint != "none":
        W = torch.from_numpy(odd_mask(batch, p.length)).to(device) if constraint == "offset_mask" else None
        p.agla_constrain(torch.from_numpy(off).to(device), W)
    geo = p.launch_geometry
    waves = []
    for _ in range(ITERS):
        p.agla_iterate(1)
        waves.append(np.ascontiguousarray(p.wave().cpu().numpy()))
    return waves, geo


def run_adjoint(case, device=None):
    """-> the output arrays of the adjoint case in a fixed order, the three inner products (float64) last where there are any"""
    from spectrogram_inversion_amd.plan import Plan, args_helper
    (hop, frames, batch), dtype, n, general, route = case
    device = torch.device("cuda", 0) if device is None else device
    npdt = np.dtype(dtype).type
    cd = torch.complex64 if dtype == "float32" else torch.complex128
    p = Plan(args_helper(torch.empty((1, 9, 1), dtype=cd), hop_length=hop, window=torch.from_numpy(hann(16, npdt))), batch, frames,
             TDT[dtype], device)
    B, L = p.batch, p.length
    T_ = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(device)         # noqa: E731
    W = T_(odd_mask(B, L)) if route == "cgla_mask" else None
    if n == 1:
        rng = np.random.default_rng(hop)
        a0, gc0, gd0, go0, c0 = (rng.standard_normal((B, L)).astype(npdt) for _ in range(5))
        fm = (B, p.n_frames, p.n_freq)
        mag_fm = T_((rng.random(fm) + 0.05).astype(npdt))
        a, gc, gd, goff = T_(a0), T_(gc0), (T_(gd0) if general else None), T_(go0)
        gm = torch.zeros(fm, dtype=TDT[dtype], device=device)
        if route == "agla":
            p.agla_first_adjoint(T_(c0), a, gc, gd, mag_fm, gm)
            out = [gc, gm]                                    # (a and gd are left as they were)
        else:
            p.cgla_first_adjoint(T_(c0), W, a, gc, gd, goff, mag_fm, gm)
            out = [gc, goff, gm]
        return [np.ascontiguousarray(x.cpu().numpy()) for x in out if x is not None]
    rng = np.random.default_rng(hop + n)
    a0, gc0, gd0, tn, tp, tpp, go0 = (rng.standard_normal((B, L)).astype(npdt) for _ in range(7))
    coef = (0.5, 1.2, 0.7, 0.45, 1.1) if general else (0.99, 0.3, 1.0, 0.9, 0.8)
    a, gc, gd, goff = T_(a0), T_(gc0), (T_(gd0) if general else None), T_(go0)
    c_prev = torch.full((B, L), float("nan"), dtype=TDT[dtype], device=device)
    dots = torch.full((3,), float("nan"), dtype=torch.float64, device=device)
    t_nm2 = T_(tpp) if n > 2 else None
    if route == "agla":
        p.agla_extrap_adjoint(T_(tn), T_(tp), t_nm2, coef, a, gc, gd, c_prev, dots)
        out = [a, gc, gd, c_prev, dots]
    else:
        p.cgla_extrap_adjoint(T_(tn), T_(tp), t_nm2, coef, W, a, gc, gd, goff, c_prev, dots)
        out = [a, gc, gd, goff, c_prev, dots]
    return [np.ascontiguousarray(x.cpu().numpy()) for x in out if x is not None]


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def kept(arrays):
    """What the fixture stores of a case's arrays beside the digest: each one whole up to HEAD elements, its first HEAD beyond"""
    return [a.reshape(-1)[:HEAD] for a in arrays]


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def forward_outputs(case):
    """-> (the arrays the digest covers, the arrays whose values are kept, the geometry)"""
    waves, geo = run_forward(case)
    return waves, [waves[-1]], geo


def adjoint_outputs(case):
    out = run_adjoint(case)
    return out, out, None


def main():
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    packed = {"float32": [], "float64": []}
    fill = {"float32": 0, "float64": 0}
    cases, unstable = {}, []
    todo = [(forward_name(c), forward_outputs, c) for c in FORWARD] + [(adjoint_name(c), adjoint_outputs, c) for c in ADJOINT]
    for name, fn, case in todo:
        arrays, keep, geo = fn(case)
        again = fn(case)[0]                                   # (the recorded bits are the build's, not one run's)
        assert all(np.isfinite(a).all() for a in arrays), name
        if len(arrays) != len(again) or not all(same_bits(a, b) for a, b in zip(arrays, again)):
            unstable.append(name)
            continue
        entry = {"sha256": digest(arrays), "kept": []}
        if geo is not None:
            want = SHAPES[case[0]][6]
            assert want is None or (geo["kernel"] == want[0] and geo["chunks"] >= want[1]), (name, geo)
            entry.update(kernel=geo["kernel"], chunks=geo["chunks"])
        for a in kept(keep):
            dt = a.dtype.name
            packed[dt].append(a)
            entry["kept"].append([dt, fill[dt], int(a.size)])
            fill[dt] += int(a.size)
        cases[name] = entry
        print(name, entry["sha256"][:16], entry.get("kernel", ""), entry.get("chunks", ""), flush=True)
    assert not unstable, ("two runs disagree", unstable)
    meta = {"commit": commit, "iters": ITERS, "head": HEAD, "cases": cases}
    rec = {"f32": np.concatenate(packed["float32"]), "f64": np.concatenate(packed["float64"]),
           "meta": np.array(json.dumps(meta, sort_keys=True, separators=(",", ":")))}
    os.makedirs(os.path.dirname(out), exist_ok=True)
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
