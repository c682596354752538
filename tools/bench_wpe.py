#!/usr/bin/env python3
"""wpe (k_wpe) in complex64 with taps 10, delay 3 and 3 iterations at B 16, C 1, F 257, T 512 (D 10) and B 4, C 4,
F 257, T 512 (D 40), against the same definition written as torch ops (`unfold`, `einsum`, `torch.linalg.solve`, complex128) on the
same GPU in the same run.  One JSON line, also written to profiles/wpe_bench.json.

    python tools/bench_wpe.py [--window MS] [--repeats M] [--out PATH]

per shape:
launch_ms        specinv_wpe on preallocated arrays: events around as many calls as fill `window` ms, the median of `repeats`
                 such windows (tools/bench_yin.py's `timed`)
call_ms          si.wpe(x, 10, 3, 3), the public function
torch_ms         the definition in torch ops, timed the same way (the same `timed`, after a run at full size)
agreement        the relative L2 distance of the two results
fp64_fma_rate    the float64 fused multiply-adds the definition needs - 4 T (D (D + 1) / 2 + D C) a bin and iteration for R and P,
                 4 T D C a bin for each of the n_iter filterings - over launch_ms, and its share of the chip's vector float64
                 peak (78.6 TFLOP/s = 39.3e12 FMA/s, the public datasheet figure)
split            where the launch's time goes, without instrumenting the kernel: filter_ms is the filter-only launch (one
                 walk), power_filter_ms the n_iter = 0 launch (the power pass and one walk), iteration_ms = (launch_ms -
                 power_filter_ms) / 3, one iteration's power pass, accumulation and solve; the same at T 256 gives the part of an
                 iteration that does not grow with T, solve_ms_fit = 2 iteration_ms(256) - iteration_ms(512) (the factorisation
                 and the solves), and frames_ms_fit = iteration_ms(512) - solve_ms_fit (the power pass and the accumulation)
`library` names the library measured: a variant built with -DSPECINV_WPE_SLICES=1, 2 or 4 (build_lib(extra_flags=..., out=...),
selected with SPECINV_LIB) gives the figures of fewer frame slices.  Nothing is required of the ratio; the tool writes down what
comes out.
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

TAPS, DELAY, N_ITER, EPS, LOAD = 10, 3, 3, 1e-10, 1e-10
PEAK_FMA = 39.3e12
TINY = 2.2250738585072014e-308


def wpe_torch(X, taps=TAPS, delay=DELAY, n_iter=N_ITER, eps=EPS, diag_load=LOAD):
    """Y (B, C, F, T) complex128: the module's definition in torch ops"""
    X = X.to(torch.complex128)
    B, Cn, F, T = X.shape
    D = Cn * taps
    Xp = X.new_zeros((B, Cn, F, T + delay + taps - 1))
    Xp[..., delay + taps - 1:] = X
    xs = Xp[..., :T + taps - 1].unfold(-1, taps, 1).flip(-1)                  # (B, C, F, T, K): X[t - delay - k]
    xs = xs.permute(0, 2, 1, 4, 3).reshape(B, F, D, T)
    Xf = X.permute(0, 2, 1, 3)                                                 # (B, F, C, T)
    Y = Xf
    eye = torch.eye(D, dtype=torch.complex128, device=X.device)
    for _ in range(n_iter):
        q = (Y.real ** 2 + Y.imag ** 2).mean(2)
        lam = torch.maximum(q, eps * q.amax(-1, keepdim=True)).clamp(min=TINY)
        xw = xs / lam[:, :, None, :]
        R = torch.einsum("bfdt,bfet->bfde", xw, xs.conj())
        P = torch.einsum("bfdt,bfct->bfdc", xw, Xf.conj())
        tr = torch.diagonal(R, dim1=-2, dim2=-1).real.sum(-1)
        R = R + (diag_load * tr / D + TINY)[..., None, None] * eye
        G = torch.linalg.solve(R, P)
        Y = Xf - torch.einsum("bfdc,bfdt->bfct", G.conj(), xs)
    return Y.permute(0, 2, 1, 3)


def fmas(B, Cn, F, T, taps=TAPS, n_iter=N_ITER):
    D = Cn * taps
    return B * F * n_iter * 4 * T * (D * (D + 1) // 2 + 2 * D * Cn)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=200.0, help="ms of work per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wpe_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    gen = torch.Generator(device=dev).manual_seed(0)
    res = {"tool": "tools/bench_wpe.py", "device": torch.cuda.get_device_name(0), "library": os.path.basename(_lib.LIB_PATH),
           "config": dict(taps=TAPS, delay=DELAY, n_iter=N_ITER, dtype="complex64", window_ms=a.window, repeats=a.repeats,
                          peak_fp64_fma_per_s=PEAK_FMA), "cases": {}}
    for (B, Cn, F, T) in ((16, 1, 257, 512), (4, 4, 257, 512)):
        # noise smoothed along the frames (pole 0.8), so that there is something to predict
        e = torch.randn((B, Cn, F, T, 2), device=dev, generator=gen)
        z = torch.empty_like(e)
        acc = torch.zeros_like(e[..., 0, :])
        for t in range(T):
            acc = 0.8 * acc + e[..., t, :]
            z[..., t, :] = acc
        x = torch.view_as_complex(z.contiguous())
        D = Cn * TAPS

        def launcher(xx, n_iter, filt=None):
            nT = xx.shape[-1]
            out = torch.empty_like(xx)
            lam = torch.empty((B, F, nT), dtype=torch.float64, device=dev)

            def launch():
                _lib.check(lib.specinv_wpe(xx.data_ptr(), None, None if filt is None else filt.data_ptr(), out.data_ptr(), None,
                                           None if filt is not None else lam.data_ptr(), None, B, Cn, F, nT, TAPS, DELAY, n_iter, 0,
                                           EPS, LOAD, _lib.F32, 0, sp))
            return launch, out

        r, split = {}, {}
        for nT in (T, T // 2):
            xx = x[..., :nT].contiguous()
            filt = si.wpe(xx, TAPS, DELAY, N_ITER, return_filter=True)[1].contiguous()
            full = timed(launcher(xx, N_ITER)[0], a.window, a.repeats)
            pf = timed(launcher(xx, 0)[0], a.window, a.repeats)
            fo = timed(launcher(xx, 0, filt)[0], a.window, a.repeats)
            split[nT] = dict(launch_ms=full, power_filter_ms=pf, filter_ms=fo, iteration_ms=(full - pf) / N_ITER)
        r["launch_ms"] = split[T]["launch_ms"]
        r["call_ms"] = timed(lambda: si.wpe(x, TAPS, DELAY, N_ITER), a.window, a.repeats)
        solve = 2 * split[T // 2]["iteration_ms"] - split[T]["iteration_ms"]
        r["split"] = dict(filter_ms=split[T]["filter_ms"], power_filter_ms=split[T]["power_filter_ms"],
                          iteration_ms=split[T]["iteration_ms"], iteration_ms_half_T=split[T // 2]["iteration_ms"],
                          solve_ms_fit=solve, frames_ms_fit=split[T]["iteration_ms"] - solve)
        Yt = wpe_torch(x)                                                          # (also `timed`'s kind of warm-up, at full size)
        r["torch_ms"] = timed(lambda: wpe_torch(x), a.window, a.repeats)
        r["torch_over_launch"] = r["torch_ms"] / r["launch_ms"]
        r["torch_over_call"] = r["torch_ms"] / r["call_ms"]
        launch, out = launcher(x, N_ITER)
        launch()
        torch.cuda.synchronize()
        r["agreement"] = {"rel_l2": float(torch.linalg.vector_norm(out.to(torch.complex128) - Yt) / torch.linalg.vector_norm(Yt))}
        rate = fmas(B, Cn, F, T) / (r["launch_ms"] * 1e-3)
        r["fp64_fma_rate"] = {"fma_per_s": rate, "share_of_peak": rate / PEAK_FMA}
        del Yt

        def rounded(v):
            return {k: rounded(w) for k, w in v.items()} if isinstance(v, dict) else (float(f"{v:.5g}") if isinstance(v, float) else v)
        res["cases"][f"B {B} C {Cn} F {F} T {T} (D {D})"] = rounded(r)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
