#!/usr/bin/env python3
"""phase_vocoder (k_phase_vocoder) at B 16, n_fft 1024, hop 256, 512 input frames, rates 0.8 and 1.25, float32,
against the same definition written as torch ops on the same GPU: one JSON line, also written to profiles/pvoc_bench.json.

    python tools/bench_pvoc.py [--reps N] [--repeats M] [--out PATH]

per rate:
launch_ms             Plan.phase_vocoder on a warm plan: events around `reps` calls, the median of `repeats` such windows
call_ms               si.phase_vocoder, the public function (argument checks, plan cache, the output's allocation), likewise
torch_f64_ms          the definition as torch ops: float32 angles, everything after them in float64 (what the kernel computes)
torch_f32_ms          ... as a plain float32 op chain (what the usual torch implementations do; 1e-3 of the result is lost)
min_bytes             the spectrogram read once and the result written once; GBps = min_bytes / launch_ms
err_*                 max |P - P_ref| / max |P_ref| against the definition in float64 torch ops on the input's bits
`accuracy` holds the same three errors as relative L2 at the four shapes of DESIGN 3.19's table.  No gate: the figures go into DESIGN.
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import spectrogram_inversion_amd as si
from spectrogram_inversion_amd.plan import args_helper, get_plan


def pvoc_torch(spec, rate, n_fft, hop, angle=torch.float32, work=torch.float64):
    """DESIGN 3.19 in torch ops on the tensor's device: the angles in `angle`, everything after them in `work`."""
    n_out = si.stretched_frames(spec.shape[-1], rate)
    t = torch.arange(n_out, dtype=torch.float64, device=spec.device) * rate
    fl = torch.floor(t)
    i = fl.to(torch.int64)
    a = (t - fl).to(work)
    sp = torch.cat([spec, spec.new_zeros(spec.shape[:-1] + (2,))], -1)
    s0, s1 = sp[..., i], sp[..., i + 1]
    th0 = torch.atan2(s0.imag.to(angle), s0.real.to(angle)).to(work)
    th1 = torch.atan2(s1.imag.to(angle), s1.real.to(angle)).to(work)
    cw = torch.complex128 if work == torch.float64 else torch.complex64
    m = a * s1.to(cw).abs() + (1 - a) * s0.to(cw).abs()
    k = torch.arange(spec.shape[-2], dtype=torch.float64, device=spec.device)
    adv = (2 * math.pi * torch.where(k <= n_fft // 2, k, k - n_fft) * hop / n_fft)[:, None].to(work)
    two_pi = torch.tensor(2 * math.pi, dtype=work, device=spec.device)
    d = th1 - th0 - adv
    d = d - two_pi * torch.round(d / two_pi) + adv
    phi = torch.cumsum(torch.cat([th0[..., :1], d[..., :-1]], -1), -1)
    return torch.polar(m, phi)


def window_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def timed(fn, reps, repeats):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    return statistics.median(window_ms(fn, reps) for _ in range(repeats))


def signal(batch, n, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64, device=dev)
    chirp = torch.sin(2 * math.pi * (0.02 * t + 0.5 * (0.3 / n) * t * t))
    return (chirp + 0.3 * torch.randn((batch, n), device=dev, dtype=torch.float64, generator=gen)).float()


def errors(spec, rate, n_fft, hop, kw, norm):
    ref = pvoc_torch(spec, rate, n_fft, hop, angle=torch.float64)
    out = {"kernel": si.phase_vocoder(spec, rate, **kw),
           "torch_f32_angles": pvoc_torch(spec, rate, n_fft, hop),
           "torch_f32_chain": pvoc_torch(spec, rate, n_fft, hop, work=torch.float32)}
    return {k: float(norm(v.to(torch.complex128) - ref) / norm(ref)) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pvoc_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, T, n_fft, hop = 16, 512, 1024, 256
    kw = dict(hop_length=hop, window=torch.hann_window(n_fft))
    spec = si.stft(signal(B, (T - 1) * hop, dev, 0), n_fft, **kw)
    assert spec.shape == (B, n_fft // 2 + 1, T) and spec.dtype == torch.complex64
    res = {"tool": "tools/bench_pvoc.py", "device": torch.cuda.get_device_name(0),
           "config": dict(B=B, n_fft=n_fft, hop=hop, T=T, dtype="float32", reps=a.reps, repeats=a.repeats), "rates": {}}
    maxabs = lambda v: v.abs().max()                                                       # noqa: E731
    for rate in (0.8, 1.25):
        n_out = si.stretched_frames(T, rate)
        plan = get_plan(args_helper(spec, **kw), B, n_out, torch.float32, dev)
        r = {"T_out": n_out,
             "launch_ms": timed(lambda: plan.phase_vocoder(spec, rate), a.reps, a.repeats),
             "call_ms": timed(lambda: si.phase_vocoder(spec, rate, **kw), a.reps, a.repeats),
             "torch_f64_ms": timed(lambda: pvoc_torch(spec, rate, n_fft, hop), max(1, a.reps // 10), a.repeats),
             "torch_f32_ms": timed(lambda: pvoc_torch(spec, rate, n_fft, hop, work=torch.float32), max(1, a.reps // 10), a.repeats)}
        r["min_bytes"] = 8 * B * spec.shape[1] * (T + n_out)
        r["GBps"] = r["min_bytes"] / (r["launch_ms"] * 1e-3) / 1e9
        r["torch_f64_over_launch"] = r["torch_f64_ms"] / r["launch_ms"]
        r["torch_f32_over_launch"] = r["torch_f32_ms"] / r["launch_ms"]
        r.update({"err_" + k: v for k, v in errors(spec, rate, n_fft, hop, kw, maxabs).items()})
        res["rates"][str(rate)] = {k: (round(v, 5) if isinstance(v, float) and v > 1e-3 else v) for k, v in r.items()}
    res["accuracy"] = []
    for nf, hp, rate, frames in ((512, 128, 0.8, 301), (512, 128, 1.25, 301), (2048, 512, 1.5, 258), (128, 32, 0.5, 1101)):
        kwa = dict(hop_length=hp, window=torch.hann_window(nf))
        s = si.stft(signal(2, (frames - 1) * hp, dev, nf), nf, **kwa)
        row = dict(n_fft=nf, hop=hp, rate=rate, T=frames, T_out=si.stretched_frames(frames, rate))
        row.update({"rel_l2_" + k: v for k, v in errors(s, rate, nf, hp, kwa, torch.linalg.norm).items()})
        res["accuracy"].append(row)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
