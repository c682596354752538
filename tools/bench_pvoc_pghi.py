#!/usr/bin/env python3
"""phase_lock="pghi" (DESIGN 3.26): the time of one call beside the other two modes, and what its phase is worth as a start.  One
JSON line, also written to profiles/pvoc_pghi_bench.json.

    python tools/bench_pvoc_pghi.py [--reps N] [--repeats M] [--out PATH] [--skip-buys]

timing      B 16, 512 -> 640 frames (rate 0.8) of the chirp + 0.3 noise, 1024 / 256 and 2048 / 512, float32 and float64.  Per entry:
  launch_ms       specinv_pvoc_pghi on preallocated outputs: events around `reps` calls, the median of `repeats` such windows
  call_ms         si.phase_vocoder(..., phase_lock="pghi"), the public function (argument checks, the allocation), likewise
  us_per_frame    launch_ms per output frame of one item: the 16 items run side by side, one workgroup each
  unlocked_ms, identity_ms   si.phase_vocoder with phase_lock=None and "identity" on the same input, in the same run
  cpu_oracle_s    the NumPy definition of tests/_pvoc_pghi_oracle.py on ONE item on the host: a CPU figure
  parents_equal   the kernel's parents on that item against the NumPy definition's (must be true)
buys        || |stft(y)| - |P| || / || |P| || of y = time_stretch(x, rate, max_iter=n, tol=0), default method, 1024 / 256, 300 frames,
  float32, after 0 / 5 / 10 / 30 iterations from the three modes, on the harmonic signal and on the chirp + 0.3 noise at rates 0.5
  and 0.8 (P the mode's own vocoder output: the magnitudes agree between the modes to a rounding).
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
from _pvoc_pghi_oracle import pghi_ref, signal
from spectrogram_inversion_amd import _lib

RATE = 0.8


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


def timing(n_fft, hop, dtype, T, B, reps, repeats, dev):
    F = n_fft // 2 + 1
    x = torch.stack([signal("chirp", (T - 1) * hop, seed=n_fft + b) for b in range(B)])
    w64 = torch.hann_window(n_fft, dtype=torch.float64)
    cd = torch.complex64 if dtype == torch.float32 else torch.complex128
    s = torch.stft(x, n_fft, hop_length=hop, window=w64, return_complex=True).to(cd).to(dev).contiguous()
    assert s.shape == (B, F, T)
    n_out = si.stretched_frames(T, RATE)
    kw = dict(hop_length=hop, window=torch.hann_window(n_fft, dtype=dtype))
    lib = _lib.load()
    out = torch.empty((B, F, n_out), dtype=cd, device=dev)
    stream = torch.cuda.current_stream()
    code = _lib.F32 if dtype == torch.float32 else _lib.F64

    def launch():
        _lib.check(lib.specinv_pvoc_pghi(s.data_ptr(), out.data_ptr(), None, B, F, T, n_out, n_fft, hop, RATE, 1e-6, code,
                                         stream.device.index, C.c_void_p(stream.cuda_stream)))

    res = {"n_fft": n_fft, "hop": hop, "F": F, "T_in": T, "T_out": n_out, "B": B, "rate": RATE,
           "dtype": "float32" if dtype == torch.float32 else "float64", "bins_per_lane": (-(-F // 256)) | 1}
    res["launch_ms"] = round(timed(launch, reps, repeats), 4)
    res["call_ms"] = round(timed(lambda: si.phase_vocoder(s, RATE, phase_lock="pghi", **kw), reps, repeats), 4)
    res["us_per_frame"] = round(1e3 * res["launch_ms"] / n_out, 3)
    res["unlocked_ms"] = round(timed(lambda: si.phase_vocoder(s, RATE, **kw), reps, repeats), 4)
    res["identity_ms"] = round(timed(lambda: si.phase_vocoder(s, RATE, phase_lock="identity", **kw), reps, repeats), 4)
    _, parents = si.phase_vocoder(s[:1], RATE, phase_lock="pghi", return_parents=True, **kw)
    item = s[0].cpu()
    t0 = time.perf_counter()
    want = pghi_ref(item, RATE, n_fft, hop)[2]
    res["cpu_oracle_s"] = round(time.perf_counter() - t0, 2)
    res["parents_equal"] = bool(np.array_equal(parents[0].cpu().numpy(), want))
    return res


def buys(dev):
    n_fft, hop, T = 1024, 256, 300
    kw = dict(hop_length=hop, window=torch.hann_window(n_fft))
    table = {}
    for name in ("harmonic", "chirp"):
        x = signal(name, (T - 1) * hop).to(torch.float32).to(dev)
        for rate in (0.5, 0.8):
            row = {}
            for lock in (None, "identity", "pghi"):
                target = si.phase_vocoder(si.stft(x, n_fft, **kw), rate, phase_lock=lock, **kw).abs().double()
                for it in (0, 5, 10, 30):
                    y = si.time_stretch(x, rate, n_fft, max_iter=it, phase_lock=lock, tol=0, verbose=False, **kw)
                    got = si.stft(y, n_fft, **kw).abs().double()
                    row[f"{lock}, {it} iterations"] = round(float(torch.linalg.norm(got - target) / torch.linalg.norm(target)), 4)
            table[f"{name}, rate {rate}"] = row
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--skip-buys", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pvoc_pghi_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "repeats": a.repeats,
           "timing": [timing(n, h, d, 512, 16, a.reps, a.repeats, dev)
                      for n, h in ((1024, 256), (2048, 512)) for d in (torch.float32, torch.float64)]}
    if not a.skip_buys:
        res["buys"] = buys(dev)
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    ok = all(t["parents_equal"] for t in res["timing"])
    sys.exit(0 if ok and all(math.isfinite(t["launch_ms"]) for t in res["timing"]) else 1)


if __name__ == "__main__":
    main()
