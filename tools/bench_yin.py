#!/usr/bin/env python3
"""yin (k_yin) at B 16, L 163 584, frames of 2048 every 512 and of 1024 every 256, against the same definition written as
torch ops on the same GPU in the same run, and the accuracy figures tests/test_gpu_yin.py refers to.  One JSON line, also written
to profiles/yin_bench.json.

    python tools/bench_yin.py [--window MS] [--repeats M] [--out PATH]

per shape:
launch_ms             specinv_yin on preallocated outputs (period, aperiodicity, tau): events around as many calls as fill `window` ms
                      (200: enough work that the clock and the scheduler do not show), the median of `repeats` such windows
launch_cmnd_ms        the same with the (B, T, W + 1) array of d' written as well
call_ms               si.yin, the public function (argument checks, the outputs' allocation, f0 and voiced from period and d')
torch_ms              the definition as torch ops: unfold, two rfft and an irfft in float32, two cumsum and the normalisation in
                      float64 over the (B, T, W + 1) array, the first-below-threshold search, the descent and the arg-min as masked
                      arg-max / arg-min, a gather and the parabola
frames_per_s          B T / launch_ms
agreement             lags that differ between the two (their float32 correlations differ in the last bits) and the largest relative
                      difference in period where the lags agree
accuracy              per frame length, on the test's four signals (hop N / 4 and 100, centred and not): the largest error in d'
                      against the float64 oracle of `cmnd_f32` on the CPU (the yardstick) and of the kernel
No speed is promised and nothing is asserted about it: the tool writes down what comes out.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import _yin_oracle as oracle
import spectrogram_inversion_amd as si
from spectrogram_inversion_amd import _lib


def yin_torch(x, n, hop, tau_min, tau_max, threshold):
    """The module's definition in torch ops, centred frames: (period float32, aperiodicity float32, tau int64), each (B, T)"""
    w = n // 2
    t = 1 + x.shape[-1] // hop
    f = torch.nn.functional.pad(x, (w, n)).unfold(-1, n, hop)[:, :t]
    r = torch.fft.irfft(torch.fft.rfft(f[..., :w], n).conj() * torch.fft.rfft(f, n), n)[..., :w + 1]
    p = torch.nn.functional.pad(torch.cumsum(f.double() ** 2, -1), (1, 0))
    e = p[..., w:n + 1] - p[..., :w + 1]
    d = e[..., :1] + e - 2.0 * r.double()
    d[..., 0] = 0
    c = torch.cumsum(d, -1)
    lag = torch.arange(w + 1, device=x.device, dtype=torch.float64)
    dp = torch.where(c > 0, d * lag / c, torch.ones_like(d)).float()
    dp[..., 0] = 1
    rng, nxt = dp[..., tau_min:tau_max + 1], dp[..., tau_min + 1:tau_max + 2]
    below = rng.double() < threshold
    first = below.to(torch.uint8).argmax(-1, keepdim=True)
    stop = ~(nxt < rng)
    stop[..., -1] = True
    idx = torch.arange(rng.shape[-1], device=x.device)
    rest = (stop & (idx >= first)).to(torch.uint8).argmax(-1)
    tau = torch.where(below.any(-1), rest, rng.argmin(-1)) + tau_min
    a, b, cc = (dp.gather(-1, (tau + k).unsqueeze(-1)).squeeze(-1).double() for k in (-1, 0, 1))
    q, num = a - 2 * b + cc, a - cc
    s = torch.where((q > 0) & (num.abs() < q), num / (2 * q), torch.zeros_like(q))
    return (tau.double() + s).float(), b.float(), tau


def window_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def timed(fn, window, repeats):
    """ms per call: events around as many calls as fill `window` ms (sized by a pilot of 10), the median of `repeats` such windows"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    reps = max(10, min(50000, int(window / max(window_ms(fn, 10), 1e-4))))
    return statistics.median(window_ms(fn, reps) for _ in range(repeats))


def accuracy(dev):
    out = {}
    for n in (256, 512, 1024, 2048):
        x = oracle.signals(n)
        yard = kern = 0.0
        for hop in (n // 4, 100):
            for center in (True, False):
                got = si.yin_cmnd(torch.tensor(x).to(dev), n, hop, center).double().cpu().numpy()
                for item in range(4):
                    ref = oracle.cmnd(x[item], n, hop, center)
                    yard = max(yard, float(np.abs(oracle.cmnd_f32(x[item], n, hop, center) - ref).max()))
                    kern = max(kern, float(np.abs(got[item] - ref).max()))
        out[str(n)] = {"float32_restatement_max_err": yard, "kernel_max_err": kern, "ratio": round(kern / yard, 3)}
    return out


def voice(batch, length, sr, dev):
    """harmonic items of different pitch with vibrato and some noise: most frames voiced"""
    t = torch.arange(length, device=dev, dtype=torch.float64) / sr
    f0 = torch.linspace(90.0, 400.0, batch, device=dev, dtype=torch.float64)[:, None]
    ph = 2 * np.pi * torch.cumsum(f0 * 2.0 ** (0.05 * torch.sin(2 * np.pi * 1.5 * t)) / sr, -1)
    x = sum(torch.sin(h * ph) / h for h in range(1, 6))
    return (x + 0.02 * torch.randn(x.shape, device=dev, dtype=torch.float64, generator=torch.Generator(device=dev).manual_seed(0))).float()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=200.0, help="ms of work per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yin_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, L, sr, fmax, thr = 16, 163584, 16000, 1000.0, 0.1
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev)
    res = {"tool": "tools/bench_yin.py", "device": torch.cuda.get_device_name(0), "library": os.path.basename(_lib.LIB_PATH),
           "config": dict(B=B, L=L, sample_rate=sr, fmax=fmax, threshold=thr, window_ms=a.window, repeats=a.repeats), "shapes": {}}
    x = voice(B, L, sr, dev)
    for n, hop in ((2048, 512), (1024, 256)):
        fmin = max(60.0, sr / (n // 2 - 1))
        tau_min, tau_max = oracle.lag_range(sr, fmin, fmax)
        t = si.yin_frames(L, n, hop)
        period, aper = torch.empty((B, t), device=dev), torch.empty((B, t), device=dev)
        tau = torch.empty((B, t), dtype=torch.int32, device=dev)
        cmnd = torch.empty((B, t, n // 2 + 1), device=dev)

        def launch(with_cmnd=False):
            _lib.check(lib.specinv_yin(x.data_ptr(), period.data_ptr(), aper.data_ptr(), tau.data_ptr(),
                                       cmnd.data_ptr() if with_cmnd else None, B, L, n, hop, 1, tau_min, tau_max, thr, _lib.F32, 0,
                                       C.c_void_p(stream.cuda_stream)))

        r = {"T": t, "fmin": round(fmin, 3), "tau_min": tau_min, "tau_max": tau_max,
             "launch_ms": timed(launch, a.window, a.repeats),
             "launch_cmnd_ms": timed(lambda: launch(True), a.window, a.repeats),
             "call_ms": timed(lambda: si.yin(x, sr, fmin, fmax, n, hop, thr), a.window, a.repeats),
             "torch_ms": timed(lambda: yin_torch(x, n, hop, tau_min, tau_max, thr), a.window, a.repeats)}
        r["frames_per_s"] = round(B * t / (r["launch_ms"] * 1e-3))
        r["torch_over_launch"] = r["torch_ms"] / r["launch_ms"]
        launch()
        want_period, want_aper, want_tau = yin_torch(x, n, hop, tau_min, tau_max, thr)
        same = want_tau == tau
        r["voiced_share"] = float((aper.double() < thr).double().mean())
        r["agreement"] = {"lags_that_differ": int((~same).sum()), "of": B * t,
                          "period_max_rel_diff": float((period[same] / want_period[same] - 1).abs().max()),
                          "aperiodicity_max_diff": float((aper[same] - want_aper[same]).abs().max())}
        res["shapes"][f"{n} / {hop}"] = {k: (round(v, 5) if isinstance(v, float) else v) for k, v in r.items()}
    res["accuracy"] = accuracy(dev)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
