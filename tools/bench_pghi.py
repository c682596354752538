#!/usr/bin/env python3
"""rtpghi: the time of one call, and what its phase is worth as a start.  One JSON line, also written to
profiles/pghi_bench.json.

    python tools/bench_pghi.py [--reps N] [--repeats M] [--out PATH]

timing      B 16, T 512, float32, F 513 (1024 / 256) and 1025 (2048 / 512), magnitudes of seeded noise.  Per entry:
  launch_ms       specinv_pghi on preallocated outputs: events around `reps` calls, the median of `repeats` such windows
  call_ms         si.rtpghi, the public function (argument checks, the allocations), likewise
  us_per_frame    launch_ms per frame of one item: the 16 items run side by side, one workgroup each
  phase_init_ms   si.phase_init on the same magnitudes, the start the package had (a different, cheaper estimate)
  cpu_heap_s      the NumPy heap of tests/_pghi_oracle.py on ONE item on the host: a CPU figure, the only other implementation there is
  parents_equal   the kernel's parents on that item against the NumPy definition's (must be true)
  heap_agreement  the fraction of that item's bins on which the heap chose the same parent: float32 magnitudes of 5e5 bins hold equal
                  values, and among equals the heap's order is its own
inconsistency   || |stft(y)| - s || / || s || at 512 / 128, Hann, 64 frames, float64, with the package's own stft / istft /
  accelerated_griffin_lim: y after 0, 5 and 30 iterations from rtpghi, from phase_init and from zero phase, on five chirping
  partials, on white noise and on clicks plus a tone.
Exit status 1 if the parents differ; the speed is reported, not judged.
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import spectrogram_inversion_amd as si
from _pghi_oracle import HANN_GAMMA, definition, heap
from spectrogram_inversion_amd import _lib


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


def timing(F, T, B, reps, repeats, dev):
    n_fft, hop = 2 * (F - 1), (F - 1) // 2
    g = torch.Generator().manual_seed(F)
    x = torch.randn(B, (T - 1) * hop, generator=g)
    w = torch.hann_window(n_fft)
    mag = torch.stft(x, n_fft, hop_length=hop, window=w, return_complex=True).abs().to(dev).contiguous()
    assert mag.shape == (B, F, T)
    lib = _lib.load()
    out = torch.empty(mag.shape, dtype=torch.complex64, device=dev)
    stream = torch.cuda.current_stream()
    gamma = HANN_GAMMA * n_fft ** 2

    def launch():
        _lib.check(lib.specinv_pghi(mag.data_ptr(), out.data_ptr(), None, None, B, F, T, n_fft, hop, gamma, 1e-6, _lib.F32,
                                    stream.device.index, C.c_void_p(stream.cuda_stream)))

    res = {"F": F, "T": T, "B": B, "n_fft": n_fft, "hop": hop, "dtype": "float32"}
    res["launch_ms"] = round(timed(launch, reps, repeats), 4)
    res["call_ms"] = round(timed(lambda: si.rtpghi(mag, hop_length=hop, window=w), reps, repeats), 4)
    res["us_per_frame"] = round(1e3 * res["launch_ms"] / T, 3)
    res["phase_init_ms"] = round(timed(lambda: si.phase_init(mag, hop_length=hop, window=w), reps, repeats), 4)
    _, parents = si.rtpghi(mag[:1], return_parents=True, hop_length=hop, window=w)
    item = mag[0].double().cpu().numpy()
    t0 = time.perf_counter()
    _, want = heap(item, n_fft, hop, gamma)
    res["cpu_heap_s"] = round(time.perf_counter() - t0, 2)
    got = parents[0].cpu().numpy()
    res["parents_equal"] = bool(np.array_equal(got, definition(item, n_fft, hop, gamma)[1]))
    res["heap_agreement"] = round(float((got == want).mean()), 6)
    return res


def signals(n):
    t = np.arange(n) / n
    rng = np.random.default_rng(0)
    chirps = sum(np.sin(2 * np.pi * n * (0.01 * k * t + 0.01 * k * t * t) + k) / k for k in range(1, 6))
    clicks = 0.5 * np.sin(2 * np.pi * 0.07 * np.arange(n))
    clicks[n // 8::n // 6] += 4.0
    return {"five chirping partials": chirps, "white noise": rng.standard_normal(n), "clicks plus a tone": clicks}


def inconsistency(dev):
    n_fft, hop, T = 512, 128, 64
    w = torch.hann_window(n_fft, dtype=torch.float64)
    kw = dict(hop_length=hop, window=w)
    table = {}
    for name, x in signals((T - 1) * hop).items():
        mag = si.stft(torch.from_numpy(x).to(dev), n_fft, **kw).abs()
        assert mag.shape == (n_fft // 2 + 1, T)
        starts = {"rtpghi": si.rtpghi(mag, **kw), "phase_init": si.phase_init(mag, **kw), "zero phase": mag.to(torch.complex128)}
        row = {}
        for sname, start in starts.items():
            for it in (0, 5, 30):
                y = si.istft(start, **kw) if it == 0 else si.accelerated_griffin_lim(start, max_iter=it, tol=0, verbose=False, **kw)
                s = si.stft(y, n_fft, **kw).abs()
                row[f"{sname}, {it} iterations"] = round(float(torch.linalg.norm(s - mag) / torch.linalg.norm(mag)), 4)
        table[name] = row
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pghi_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "repeats": a.repeats,
           "timing": [timing(F, 512, 16, a.reps, a.repeats, dev) for F in (513, 1025)],
           "inconsistency": inconsistency(dev)}
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    ok = all(t["parents_equal"] for t in res["timing"])
    sys.exit(0 if ok and all(math.isfinite(t["launch_ms"]) for t in res["timing"]) else 1)


if __name__ == "__main__":
    main()
