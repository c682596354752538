#!/usr/bin/env python3
"""Accelerated Griffin-Lim at BASELINE C2's geometry (B 64, n_fft 2048, hop 512, T 1024, float32), gamma = 1 (Fast Griffin-Lim) and
gamma != 1: one JSON line, also written to profiles/agla_bench.json.

    python tools/bench_agla.py [--iters N] [--reps N] [--no-trace] [--out PATH]
    python tools/bench_agla.py --step-only [--gamma G]      (AGLA iterations alone: the process a kernel trace wraps)

agla_*_ms_per_iter            one iteration (projection launch + k_agla_step) on a warm plan, gamma = 1 and gamma = 0.7
gla_ms_per_iter               one griffin_lim(alpha=0) iteration on the same items, in the same process (its signal-form kernel)
gla_plain_state_ms_per_iter   ... on the kernel AGLA's projection runs (keep_state's routing)
misi_ms_per_iter              one MISI iteration, the 64 items as 16 mixtures of 4 sources
step_*                        k_agla_step alone: the difference to the plain-state projection, and - unless --no-trace - its median
                              in a rocprofv3 kernel trace of a child process; bytes = 4 (gamma = 1) or 6 transfers of 4 bytes per
                              sample plus the read of the chunk tails, and their rate against the 8 TB/s peak
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
import torch

from spectrogram_inversion_amd.plan import Plan, args_helper

PEAK_BPS = 8.0e12
B, T, N_FFT, HOP = 64, 1024, 2048, 512
GAMMAS = (1.0, 0.7)
ALPHA, BETA = 0.99, 1.2


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def problem(dev):
    F = N_FFT // 2 + 1
    g = torch.Generator(device=dev).manual_seed(0)
    mag = torch.rand((B, F, T), device=dev, generator=g) + 0.05
    start = torch.polar(mag, 6.2831853 * torch.rand((B, F, T), device=dev, generator=g))
    plan = Plan(args_helper(start, hop_length=HOP, window=torch.hann_window(N_FFT)), B, T, torch.float32, dev)
    return plan, start, g


def step_bytes(plan, gamma):
    """What k_agla_step must move: x and t read and written (d too with gamma != 1), the chunk tails read"""
    geo = plan.launch_geometry
    tails = B * (geo["chunks"] - 1) * (N_FFT // HOP - 1) * HOP if geo["kernel"].startswith("k_fused") and geo["chunks"] > 1 else 0
    return ((4 if gamma == 1.0 else 6) * B * plan.length + tails) * 4


TRACE_LIMIT_S = 240


class TraceFailed(RuntimeError):
    """The traced child ended badly (a fault, an abort, its time limit): nothing more is started on the GPU after it"""


def trace_step(gamma, iters):
    """Median duration of k_agla_step in a kernel trace of a child process running AGLA iterations alone (None: no profiler).
    The child runs under `timeout -k 10`, which ends the profiler and the program below it alike; any exit status but 0 raises
    TraceFailed and the caller stops there."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None
    out = tempfile.mkdtemp(prefix="agla_trace_")
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
                # the first launch after an agla_init copies y to t, no extrapolation; --step-only calls agla_init exactly once,
                # so it is the first row of the trace and the only one to drop
                d = d[1:]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "agla_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    plan, start, g = problem(dev)
    if a.step_only:
        plan.agla_init(start, None, ALPHA, BETA, a.gamma)
        for _ in range(a.reps):
            plan.agla_iterate(a.iters)
        torch.cuda.synchronize()
        print(json.dumps({"iterations": a.reps * a.iters, "gamma": a.gamma, "kernel": plan.launch_geometry}))
        return
    device_name = torch.cuda.get_device_name(dev)
    res = {"config": dict(B=B, n_fft=N_FFT, hop=HOP, T=T, L=plan.length, dtype="float32", alpha=ALPHA, beta=BETA, iters=a.iters,
                          reps=a.reps)}
    agla_ms, geo = {}, {}
    for gamma in GAMMAS:
        plan.agla_init(start, None, ALPHA, BETA, gamma)
        agla_ms[gamma] = timed(lambda: plan.agla_iterate(a.iters), a.reps) / a.iters
        geo[gamma] = plan.launch_geometry
    plan.gla_init(start, None, 0.0)
    geo_gla = plan.launch_geometry
    gla_ms = timed(lambda: plan.iterate(a.iters), a.reps) / a.iters
    plan.keep_state(True)                        # the projection on the kernel AGLA runs it on
    plan.gla_init(start, None, 0.0)
    geo_plain = plan.launch_geometry
    plain_ms = timed(lambda: plan.iterate(a.iters), a.reps) / a.iters
    plan.keep_state(False)
    mix = 0.1 * torch.randn((B // 4, plan.length), device=dev, generator=g)
    plan.misi_init(start, None, mix, 4)
    misi_ms = timed(lambda: plan.misi_iterate(a.iters), a.reps) / a.iters
    res.update(gla_ms_per_iter=round(gla_ms, 4), gla_plain_state_ms_per_iter=round(plain_ms, 4), misi_ms_per_iter=round(misi_ms, 4),
               kernels=dict(agla=geo[1.0], griffin_lim=geo_gla, griffin_lim_plain_state=geo_plain))
    plan.agla_init(start, None, ALPHA, BETA, 1.0)          # (for step_bytes: the geometry of the kernel AGLA runs)
    step_bytes_of = {gamma: step_bytes(plan, gamma) for gamma in GAMMAS}
    del plan, start, mix                         # the timing is done: the traced children get the device to themselves
    torch.cuda.synchronize()
    failed = None
    for gamma in GAMMAS:
        tag = "fgla" if gamma == 1.0 else "general"
        nbytes = step_bytes_of[gamma]
        step_ms = agla_ms[gamma] - plain_ms
        entry = {"gamma": gamma, "ms_per_iter": round(agla_ms[gamma], 4), "over_gla": round(agla_ms[gamma] / gla_ms, 3),
                 "over_gla_plain_state": round(agla_ms[gamma] / plain_ms, 3), "step_bytes": nbytes,
                 "step_ms_by_difference": round(step_ms, 4)}
        if not a.no_trace and failed is None:
            try:
                tr = trace_step(gamma, 20)
            except TraceFailed as e:             # record it, start no further trace (nor anything else on the GPU), exit non-zero
                tr, failed = {"error": str(e)}, str(e)
            entry["kernel_trace"] = tr
            for name, st in (tr or {}).items():
                if "k_agla_step" in name and "median_us" in st:
                    st["TBps"] = round(nbytes / (st["median_us"] * 1e-6) / 1e12, 2)
                    st["fraction_of_8TBps_peak"] = round(nbytes / (st["median_us"] * 1e-6) / PEAK_BPS, 3)
        res["agla_" + tag] = entry
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"tool": "tools/bench_agla.py", "device": device_name, "bench": res}, fh, indent=1)
        fh.write("\n")
    if failed is not None:
        sys.exit(f"bench_agla: {failed}")


if __name__ == "__main__":
    main()
