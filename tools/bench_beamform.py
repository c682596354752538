#!/usr/bin/env python3
"""beamform (k_beamform) in complex64 for each solution at B 16, C 8, F 257, T 512; B 16, C 2, F 257, T 512 and B 4,
C 16, F 513, T 512, against the same definition written as torch ops (`einsum` covariances, `torch.linalg.solve`, an `einsum`
apply, complex128) on the same GPU in the same run.  One JSON line, also written to profiles/beamform_bench.json.

    python tools/bench_beamform.py [--window MS] [--repeats M] [--out PATH]

per shape and solution:
launch_ms        specinv_beamform on preallocated arrays: events around as many calls as fill `window` ms, the median of `repeats`
                 such windows (tools/bench_yin.py's `timed`)
call_ms          si.beamform(x, mask, solution=...), the public function (it expands the mask to float64 first)
torch_ms         the definition in torch ops, timed the same way (the same `timed`, after a run at full size)
agreement        the relative L2 distance of the two results
per shape:
covariance_ms    the covariance-only launch (the walk with the sums, no solve, no apply)
filter_ms        the filter-only launch (one read of X, one write of Y)
bytes            what a full launch has to move at least - X once (the second read should come from cache), the mask, Y - and
                 the rate that is of launch_ms ("souden")
fp64_fma_rate    the float64 fused multiply-adds of the sums, 8 C^2 a frame and bin as the kernel runs them (both matrices, all
                 entries), plus 4 C for the apply, over launch_ms ("souden"), and its share of the chip's vector float64 peak
                 (78.6 TFLOP/s = 39.3e12 FMA/s, the public datasheet figure)
`library` names the library measured: a variant built with -DSPECINV_BEAMFORM_WAVES=2 or 4 (build_lib(extra_flags=..., out=...),
selected with SPECINV_LIB) gives the figures of more waves a workgroup.  Nothing is required of the ratio; the tool writes down
what comes out.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch

import spectrogram_inversion_amd as si
from bench_yin import timed
from spectrogram_inversion_amd import _lib

LOAD, N_POWER, MU = 1e-7, 3, 1.0
PEAK_FMA = 39.3e12
TINY = 2.2250738585072014e-308
SHAPES = ((16, 8, 257, 512), (16, 2, 257, 512), (4, 16, 513, 512))


def beamform_torch(X, m, solution, ref=0, diag_load=LOAD, n_power_iter=N_POWER, mu=MU):
    """Y (B, F, T) complex128: the module's definition in torch ops"""
    X = X.to(torch.complex128)
    m = m.to(torch.float64)
    Cn = X.shape[1]
    eye = torch.eye(Cn, dtype=torch.complex128, device=X.device)

    def cov(w):
        acc = torch.einsum("bft,bcft,bdft->bfcd", w.to(torch.complex128), X, X.conj())
        return acc / w.sum(-1).clamp(min=TINY)[..., None, None]

    def load(A):
        tr = torch.diagonal(A, dim1=-2, dim2=-1).real.sum(-1)
        return A + (diag_load * tr / Cn + TINY)[..., None, None] * eye

    Ps, Pn = cov(m), cov(1.0 - m)
    if solution == "mwf":
        w = torch.linalg.solve(load(Ps + mu * Pn), Ps[..., ref])
    else:
        A = load(Pn)
        N = torch.linalg.solve(A, Ps)
        if solution == "souden":
            tr = torch.diagonal(N, dim1=-2, dim2=-1).real.sum(-1).clamp(min=TINY)
            w = N[..., ref] / tr[..., None]
        else:
            v = N[..., ref]
            for _ in range(n_power_iter - 1):
                s = torch.maximum(v.real.abs().amax(-1), v.imag.abs().amax(-1)).clamp(min=TINY)
                v = torch.einsum("bfcd,bfd->bfc", N, v / s[..., None])
            a = torch.einsum("bfcd,bfd->bfc", A, v)
            den = (a.conj() * v).sum(-1).real.clamp(min=TINY)
            w = v * a[..., ref].conj()[..., None] / den[..., None]
    return torch.einsum("bfc,bcft->bft", w.conj(), X)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=200.0, help="ms of work per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beamform_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    gen = torch.Generator(device=dev).manual_seed(0)
    res = {"tool": "tools/bench_beamform.py", "device": torch.cuda.get_device_name(0), "library": os.path.basename(_lib.LIB_PATH),
           "config": dict(diag_load=LOAD, n_power_iter=N_POWER, mu=MU, dtype="complex64", window_ms=a.window, repeats=a.repeats,
                          peak_fp64_fma_per_s=PEAK_FMA), "cases": {}}

    def rounded(v):
        return {k: rounded(w) for k, w in v.items()} if isinstance(v, dict) else (float(f"{v:.5g}") if isinstance(v, float) else v)

    for (B, Cn, F, T) in SHAPES:
        # a scene: a steering vector times a source that is on in half the frames, plus white noise; the mask is the noisy ideal one
        cg = lambda *s: torch.view_as_complex(torch.randn(s + (2,), device=dev, generator=gen))      # noqa: E731
        on = (torch.rand((B, 1, 1, T), device=dev, generator=gen) < 0.5).to(torch.float32)
        s = cg(B, 1, F, T) * on
        x = (cg(B, Cn, F, 1) * s + 0.3 * cg(B, Cn, F, T)).contiguous()
        p = s[:, 0].abs() ** 2
        mask = (p / (p + 0.18) + 0.1 * torch.randn((B, F, T), device=dev, generator=gen)).clamp(0.0, 1.0).to(torch.float64).contiguous()
        out = torch.empty((B, F, T), dtype=torch.complex64, device=dev)
        scm = torch.empty((B, F, Cn, Cn), dtype=torch.complex128, device=dev)
        w_in = si.beamform(x, mask, return_weights=True)[1].contiguous()

        def launcher(solution=0, mode="full"):
            mt = None if mode == "filter" else mask.data_ptr()
            wi = w_in.data_ptr() if mode == "filter" else None
            o = None if mode == "covariance" else out.data_ptr()
            sc = scm.data_ptr() if mode == "covariance" else None

            def launch():
                _lib.check(lib.specinv_beamform(x.data_ptr(), mt, None, wi, o, None, sc, None, B, Cn, F, T, solution, 0, N_POWER, LOAD, MU,
                                                _lib.F32, 0, sp))
            return launch

        r = {"covariance_ms": timed(launcher(mode="covariance"), a.window, a.repeats),
             "filter_ms": timed(launcher(mode="filter"), a.window, a.repeats), "solutions": {}}
        for solution, sid in _lib.BEAMFORM_SOLUTIONS.items():
            q = {"launch_ms": timed(launcher(sid), a.window, a.repeats),
                 "call_ms": timed(lambda: si.beamform(x, mask, solution=solution), a.window, a.repeats)}
            Yt = beamform_torch(x, mask, solution)                                  # (also `timed`'s kind of warm-up, at full size)
            q["torch_ms"] = timed(lambda: beamform_torch(x, mask, solution), a.window, a.repeats)
            q["torch_over_launch"] = q["torch_ms"] / q["launch_ms"]
            q["torch_over_call"] = q["torch_ms"] / q["call_ms"]
            launcher(sid)()
            torch.cuda.synchronize()
            q["agreement"] = {"rel_l2": float(torch.linalg.vector_norm(out.to(torch.complex128) - Yt) / torch.linalg.vector_norm(Yt))}
            del Yt
            r["solutions"][solution] = q
        ms = r["solutions"]["souden"]["launch_ms"]
        nbytes = B * F * T * (8 * Cn + 8 + 8)
        r["bytes"] = {"at_least": nbytes, "bytes_per_s": nbytes / (ms * 1e-3)}
        rate = B * F * T * (8 * Cn * Cn + 4 * Cn) / (ms * 1e-3)
        r["fp64_fma_rate"] = {"fma_per_s": rate, "share_of_peak": rate / PEAK_FMA}
        res["cases"][f"B {B} C {Cn} F {F} T {T}"] = rounded(r)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
