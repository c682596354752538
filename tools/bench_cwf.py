#!/usr/bin/env python3
"""consistent_wiener: the time of a call and of an iteration, the share of the four transforms in it against the new
element-wise kernels, and the same definition in torch ops on the same GPU.  One JSON line, also written to profiles/cwf_bench.json.

    python tools/bench_cwf.py [--reps N] [--repeats M] [--out PATH]

B 16, 1024 / 256 Hann, 512 frames, float32, 30 iterations, chirps in noise with the target's power known and a flat noise variance.
  call_ms          si.consistent_wiener with n_iter = 30: events around `reps` calls, the median of `repeats` such windows
  setup_ms         ... with n_iter = 0: the two setup kernels, one round of the four transforms, the first residual, N = X - S
  iter_ms          (call_ms - setup_ms) / 30
  transforms_ms    Plan.istft, .stft, .stft_adjoint, .istft_adjoint on the same plan, one after the other: what an iteration spends
                   in the library's transforms (each with the transpose to and from (B, F, T))
  kernels_ms       iter_ms - transforms_ms: k_cwf_u, k_cwf_q, k_cwf_update, k_cwf_dir
  kernels_bytes    what those four read and write per iteration: 17.5 complex arrays (u: 3, q: 4.5, update: 6.5, dir: 3.5; Lam, real,
                   counts one half), and kernels_gbps = kernels_bytes / kernels_ms
  torch_ms         the definition in torch ops (torch.stft / torch.istft, autograd for G', per-item sums kept on the device), 30
                   iterations, and torch_iter_ms likewise from a 0-iteration run
  distance         relative L2 distance between the two results
The speed is reported, not judged.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import spectrogram_inversion_amd as si
from _cwf_oracle import chirps_in_noise
from spectrogram_inversion_amd.plan import args_helper, get_plan


def timed(fn, reps, repeats):
    """ms per call: events around `reps` calls, the median of `repeats` windows, after a warm-up window"""
    out = []
    for r in range(repeats + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        if r:
            out.append(a.elapsed_time(b) / reps)
    return statistics.median(out)


def torch_form(X, vs, vn, gamma, n_iter, floor, n_fft, hop, window):
    """the module's definition, batched, in torch ops; alpha and beta stay on the device"""
    kw = dict(hop_length=hop, window=window)

    def G(Z):
        return torch.stft(torch.istft(Z, n_fft, **kw), n_fft, return_complex=True, **kw)

    def Gt(U):
        Z = torch.zeros_like(U, requires_grad=True)
        return torch.autograd.grad(G(Z), Z, grad_outputs=U)[0]

    def dot(a, b):
        return (torch.view_as_real(a).double() * torch.view_as_real(b).double()).sum((1, 2, 3))

    def col(s):
        return s.to(vs.dtype)[:, None, None]

    m = floor * (vs.double() + vn.double()).amax((1, 2))
    vs, vn = torch.maximum(vs, col(m)), torch.maximum(vn, col(m))
    lam = 1 / vs + 1 / vn
    g = gamma / (vs.double() * vn.double() / (vs.double() + vn.double())).mean((1, 2))
    M = lam + col(g * (1 - hop / n_fft))

    def A(P):
        u = P - G(P)
        return lam * P + col(g) * (u - Gt(u))

    S = vs / (vs + vn) * X
    r = X / vn - A(S)
    p = r / M
    rz = dot(r, p)
    for _ in range(n_iter):
        q = A(p)
        alpha = rz / dot(p, q)
        S = S + col(alpha) * p
        r = r - col(alpha) * q
        z = r / M
        rz_new = dot(r, z)
        p = z + col(rz_new / rz) * p
        rz = rz_new
    return S, X - S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cwf_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, n_fft, hop, T, n_iter, gamma = 16, 1024, 256, 512, 30, 1.0
    w = torch.hann_window(n_fft)
    kw = dict(hop_length=hop, window=w)
    sig = [chirps_in_noise((T - 1) * hop, b, noise=0.85) for b in range(B)]
    St = torch.stft(torch.stack([s for s, _ in sig]).float(), n_fft, return_complex=True, **kw)
    Nt = torch.stft(torch.stack([n for _, n in sig]).float(), n_fft, return_complex=True, **kw)
    X = (St + Nt).to(dev).contiguous()
    vs = (St.abs() ** 2).to(dev).contiguous()
    vn = (Nt.abs() ** 2).mean((1, 2), keepdim=True).expand(St.shape).to(dev).contiguous()
    F = n_fft // 2 + 1
    assert X.shape == (B, F, T)

    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "repeats": a.repeats, "B": B, "n_fft": n_fft, "hop": hop,
           "frames": T, "dtype": "float32", "n_iter": n_iter, "gamma": gamma}
    res["call_ms"] = round(timed(lambda: si.consistent_wiener(X, vs, vn, gamma=gamma, n_iter=n_iter, **kw), a.reps, a.repeats), 3)
    res["setup_ms"] = round(timed(lambda: si.consistent_wiener(X, vs, vn, gamma=gamma, n_iter=0, **kw), a.reps, a.repeats), 3)
    res["iter_ms"] = round((res["call_ms"] - res["setup_ms"]) / n_iter, 4)

    plan = get_plan(args_helper(X, **kw), B, T, torch.float32, dev)
    x = plan.istft(X)

    def transforms():
        y = plan.istft(X)
        plan.stft(y)
        y = plan.stft_adjoint(X, plan.length)
        plan.istft_adjoint(y)

    res["transforms_ms"] = round(timed(transforms, 10 * a.reps, a.repeats), 4)
    for name, fn in (("istft", lambda: plan.istft(X)), ("stft", lambda: plan.stft(x)),
                     ("stft_adjoint", lambda: plan.stft_adjoint(X, plan.length)), ("istft_adjoint", lambda: plan.istft_adjoint(x))):
        res[name + "_ms"] = round(timed(fn, 10 * a.reps, a.repeats), 4)
    res["kernels_ms"] = round(res["iter_ms"] - res["transforms_ms"], 4)
    res["transforms_share"] = round(res["transforms_ms"] / res["iter_ms"], 3)
    res["kernels_bytes"] = int(17.5 * 8 * B * F * T)
    res["kernels_gbps"] = round(res["kernels_bytes"] / (res["kernels_ms"] * 1e-3) / 1e9, 1)

    wd = w.to(dev)
    res["torch_ms"] = round(timed(lambda: torch_form(X, vs, vn, gamma, n_iter, 1e-8, n_fft, hop, wd), 1, 3), 3)
    res["torch_setup_ms"] = round(timed(lambda: torch_form(X, vs, vn, gamma, 0, 1e-8, n_fft, hop, wd), 1, 3), 3)
    res["torch_iter_ms"] = round((res["torch_ms"] - res["torch_setup_ms"]) / n_iter, 4)
    res["speedup"] = round(res["torch_ms"] / res["call_ms"], 2)
    S, _, info = si.consistent_wiener(X, vs, vn, gamma=gamma, n_iter=n_iter, return_info=True, **kw)
    St_, _ = torch_form(X, vs, vn, gamma, n_iter, 1e-8, n_fft, hop, wd)
    res["distance"] = float((S - St_).norm() / St_.norm())
    res["residual_max"] = float(info["residual"].max())
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
