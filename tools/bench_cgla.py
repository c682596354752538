#!/usr/bin/env python3
"""constrained_griffin_lim's iteration at BASELINE C2's geometry (B 64, n_fft 2048, hop 512, T 1024, float32, alpha 0.99), beside
the unconstrained AGLA iteration in the same process: one JSON line, also written to profiles/cgla_bench.json.

    python tools/bench_cgla.py [--iters N] [--reps N] [--no-trace] [--out PATH]
    python tools/bench_cgla.py --step-only [--gamma G]      (constrained iterations alone: the process a kernel trace wraps)

<tag>.free_ms_per_iter    one unconstrained iteration (projection launch + k_agla_step), gamma = 1 (fgla) and gamma = 0.7 (general)
<tag>.spec_ms_per_iter    ... with the low quarter band known (projection launch + k_agla_step, no sample mask)
<tag>.both_ms_per_iter    ... and two thirds of the samples known (the mask read too); over_free: its ratio to the first
<tag>.kernel_trace        k_agla_step with both constraints - unless --no-trace - in a rocprofv3 kernel trace of a child process: its
                          median, bytes = 5 (gamma = 1) or 7 transfers of 4 bytes per sample plus the mask byte and the read of the
                          chunk tails, and their rate against the 8 TB/s peak
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch

from bench_agla import ALPHA, B, BETA, GAMMAS, HOP, N_FFT, PEAK_BPS, T, TRACE_LIMIT_S, TraceFailed, problem, timed
from spectrogram_inversion_amd import constrained as cg


def constraints(plan, start, g):
    """The low quarter band of a second random spectrogram known, and the two outer thirds of the samples of a random signal"""
    F, L = start.shape[1], plan.length
    K = torch.polar(start.abs(), 6.2831853 * torch.rand(start.shape, device=start.device, generator=g))
    M = torch.zeros((1, F, 1), dtype=torch.bool, device=start.device)
    M[:, : F // 4] = True
    xk = 0.1 * torch.randn((B, L), device=start.device, generator=g)
    W = torch.zeros((1, L), dtype=torch.bool, device=start.device)
    W[:, : L // 3] = True
    W[:, 2 * L // 3:] = True
    return K, M.expand(start.shape), xk, W.expand(B, L)


def begin(plan, start, con, mode, gamma):
    K, M, xk, W = con
    if mode == "free":
        plan.agla_init(start, None, ALPHA, BETA, gamma)
    else:
        cg._begin(plan, start, K, M, *((xk, W) if mode == "both" else (None, None)), ALPHA, BETA, gamma)


def step_bytes(plan, gamma):
    """What k_agla_step must move with both constraints: x and t read and written, offset read (d read and written too with
    gamma != 1), a mask byte, the chunk tails read"""
    geo = plan.launch_geometry
    tails = B * (geo["chunks"] - 1) * (N_FFT // HOP - 1) * HOP if geo["kernel"].startswith("k_fused") and geo["chunks"] > 1 else 0
    return ((5 if gamma == 1.0 else 7) * B * plan.length + tails) * 4 + B * plan.length


def trace_step(gamma, iters):
    """Median duration of k_agla_step in a kernel trace of a child process running constrained iterations alone (None: no
    profiler).  The child runs under `timeout -k 10`; any exit status but 0 raises TraceFailed and the caller stops there."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None
    out = tempfile.mkdtemp(prefix="cgla_trace_")
    try:
        cmd = ["timeout", "-k", "10", str(TRACE_LIMIT_S), exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--",
               sys.executable, os.path.abspath(__file__), "--step-only", "--gamma", str(gamma), "--iters", str(iters), "--reps", "2"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise TraceFailed(f"traced child (gamma = {gamma}) exited with status {r.returncode}: {(r.stderr or r.stdout)[-400:]}")
        files = sorted(glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True))
        if not files:
            return {"error": "the profiler wrote no kernel trace: " + (r.stderr or r.stdout)[-400:]}
        per = {}
        with open(files[-1], newline="") as fh:
            for row in csv.DictReader(fh):
                name = row["Kernel_Name"]
                if "k_agla_step" in name or "k_fused4" in name:
                    per.setdefault(name.split("(")[0].replace("void specinv::", "").replace("fast::", ""), []).append(
                        (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        res = {}
        for name, d in per.items():
            if "k_agla_step" in name:
                d = d[1:]        # the first launch after the one agla_init of --step-only has no history: no t or d to read
            res[name] = {"calls": len(d), "median_us": round(statistics.median(d), 2), "min_us": round(min(d), 2),
                         "max_us": round(max(d), 2)}
        return res
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gamma", type=float, default=1.0)
    ap.add_argument("--step-only", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cgla_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    plan, start, g = problem(dev)
    con = constraints(plan, start, g)
    if a.step_only:
        begin(plan, start, con, "both", a.gamma)
        for _ in range(a.reps):
            plan.agla_iterate(a.iters)
        torch.cuda.synchronize()
        print(json.dumps({"iterations": a.reps * a.iters, "gamma": a.gamma, "kernel": plan.launch_geometry}))
        return
    device_name = torch.cuda.get_device_name(dev)
    res = {"config": dict(B=B, n_fft=N_FFT, hop=HOP, T=T, L=plan.length, dtype="float32", alpha=ALPHA, beta=BETA, iters=a.iters,
                          reps=a.reps, known_bins="the low quarter band", known_samples="the two outer thirds")}
    ms, nbytes = {}, {}
    for gamma in GAMMAS:
        for mode in ("free", "spec", "both"):
            begin(plan, start, con, mode, gamma)
            ms[gamma, mode] = timed(lambda: plan.agla_iterate(a.iters), a.reps) / a.iters
        nbytes[gamma] = step_bytes(plan, gamma)
    res["kernel"] = plan.launch_geometry
    del plan, start, con                         # the timing is done: the traced children get the device to themselves
    torch.cuda.synchronize()
    failed = None
    for gamma in GAMMAS:
        entry = {"gamma": gamma, "step_bytes": nbytes[gamma]}
        for mode in ("free", "spec", "both"):
            entry[mode + "_ms_per_iter"] = round(ms[gamma, mode], 4)
        entry["spec_over_free"] = round(ms[gamma, "spec"] / ms[gamma, "free"], 3)
        entry["both_over_free"] = round(ms[gamma, "both"] / ms[gamma, "free"], 3)
        if not a.no_trace and failed is None:
            try:
                tr = trace_step(gamma, 20)
            except TraceFailed as e:             # record it, start no further trace (nor anything else on the GPU), exit non-zero
                tr, failed = {"error": str(e)}, str(e)
            entry["kernel_trace"] = tr
            for name, st in (tr or {}).items():
                if "k_agla_step" in name and "median_us" in st:
                    st["TBps"] = round(nbytes[gamma] / (st["median_us"] * 1e-6) / 1e12, 2)
                    st["fraction_of_8TBps_peak"] = round(nbytes[gamma] / (st["median_us"] * 1e-6) / PEAK_BPS, 3)
        res["fgla" if gamma == 1.0 else "general"] = entry
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"tool": "tools/bench_cgla.py", "device": device_name, "bench": res}, fh, indent=1)
        fh.write("\n")
    if failed is not None:
        sys.exit(f"bench_cgla: {failed}")


if __name__ == "__main__":
    main()
