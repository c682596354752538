#!/usr/bin/env python3
"""MISI at BASELINE C2's geometry (n_fft 2048, hop 512, T 1024, float32; its 64 items as B 16 mixtures of K 4 sources): one JSON line.

    python tools/bench_misi.py [--iters N] [--reps N] [--mix-only]      (--mix-only: the coupling launches alone, for a profiler)

misi_ms_per_iter   one MISI iteration (projection launch + coupling launch) on a warm plan
gla_ms_per_iter    one griffin_lim(alpha=0) iteration on the same 64 items, in the same run
mix_ms             k_misi_mix alone: the difference of the two, and timed on its own through the plan's first coupling step
bytes              what the coupling launch must move, (2 K + 1) * 4 bytes per mixture sample, and the rate against the 8 TB/s peak
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from spectrogram_inversion_amd.plan import Plan, args_helper

PEAK_BPS = 8.0e12


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mix-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, K, T, n_fft, hop = 16, 4, 1024, 2048, 512
    F = n_fft // 2 + 1
    g = torch.Generator(device=dev).manual_seed(0)
    mag = torch.rand((B * K, F, T), device=dev, generator=g) + 0.05
    start = torch.polar(mag, 6.2831853 * torch.rand((B * K, F, T), device=dev, generator=g))
    args = args_helper(start, hop_length=hop, window=torch.hann_window(n_fft))
    plan = Plan(args, B * K, T, torch.float32, dev)
    L = plan.length
    mix = 0.1 * torch.randn((B, L), device=dev, generator=g)

    plan.misi_init(start, None, mix, K)
    geo_misi = plan.launch_geometry
    if a.mix_only:
        # (every misi_init ends with one coupling launch; the projection launches of an iteration come with it otherwise)
        for _ in range(a.reps):
            plan.misi_iterate(a.iters)
        torch.cuda.synchronize()
        print(json.dumps({"iterations": a.reps * a.iters, "kernel": geo_misi}))
        return
    misi_ms = timed(lambda: plan.misi_iterate(a.iters), a.reps) / a.iters
    plan.gla_init(start, None, 0.0)
    geo_gla = plan.launch_geometry
    gla_ms = timed(lambda: plan.iterate(a.iters), a.reps) / a.iters
    # the projection on the kernels MISI runs it on (the signal as xb + chunk tails: keep_state's routing)
    plan.keep_state(True)
    plan.gla_init(start, None, 0.0)
    geo_plain = plan.launch_geometry
    plain_ms = timed(lambda: plan.iterate(a.iters), a.reps) / a.iters
    plan.keep_state(False)
    mix_ms = misi_ms - plain_ms
    nbytes = (2 * K + 1) * 4 * B * L
    print(json.dumps({
        "config": dict(B=B, K=K, n_fft=n_fft, hop=hop, T=T, L=L, dtype="float32", iters=a.iters, reps=a.reps),
        "misi_ms_per_iter": round(misi_ms, 4),
        "gla_ms_per_iter": round(gla_ms, 4),
        "gla_plain_state_ms_per_iter": round(plain_ms, 4),
        "misi_over_gla": round(misi_ms / gla_ms, 3),
        "mix_ms": round(mix_ms, 4),
        "mix_bytes": nbytes,
        "mix_GBps": round(nbytes / (mix_ms * 1e-3) / 1e9, 1) if mix_ms > 0 else None,
        "mix_fraction_of_peak": round(nbytes / (mix_ms * 1e-3) / PEAK_BPS, 3) if mix_ms > 0 else None,
        "kernels": dict(misi=geo_misi, griffin_lim=geo_gla, griffin_lim_plain_state=geo_plain),
    }))


if __name__ == "__main__":
    main()
