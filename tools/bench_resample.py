#!/usr/bin/env python3
"""resample (k_resample) at B 16, L 163584 (what time_stretch returns for 1024 / 256 and 640 frames), float32, ratios
27781:22050, 2:1 and 1:2, against torchaudio's algorithm written as torch ops on the same GPU and against a device copy of the
same bytes: one JSON line, also written to profiles/resample_bench.json.

    python tools/bench_resample.py [--reps N] [--repeats M] [--out PATH]

per ratio:
launch_ms             specinv_resample into a preallocated result: events around `reps` calls, the median of `repeats` such windows
call_ms               si.resample, the public function (argument checks, the result's allocation), likewise
bank_prebuilt_ms      the filter bank + conv1d restatement in float32 with the bank made beforehand (torchaudio.transforms.Resample)
bank_built_ms         ... with the bank made in float64 and rounded inside the timed call (torchaudio.functional.resample)
bank_elements         the bank's size: n filters of 2 ceil(W o / base) + o taps
copy_ms               a device-to-device copy that reads and writes min_bytes = (L + L_out) * 4 * B bytes in all: the floor
err_kernel, err_bank_f32   max |y - y_ref| / max |y_ref|, y_ref the restatement in float64 on the input's bits
A restatement that runs out of device memory is recorded as the exception's text.  No gate: the figures go into
DESIGN 3.20.
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import spectrogram_inversion_amd as si
from spectrogram_inversion_amd import _lib


def bank(o, n, dtype, dev, width=6, rolloff=0.99):
    """torchaudio's _get_sinc_resample_kernel for the reduced ratio o : n: (n, 1, 2 w + o), made in float64, rounded to `dtype`"""
    base = min(o, n) * rolloff
    w = math.ceil(width * o / base)
    idx = torch.arange(-w, w + o, dtype=torch.float64, device=dev)[None, None] / o
    t = torch.arange(0, -n, -1, dtype=torch.float64, device=dev)[:, None, None] / n + idx
    t = (t * base).clamp_(-width, width)
    win = torch.cos(t * (math.pi / width / 2)) ** 2
    t = t * math.pi
    k = torch.where(t == 0, torch.ones((), dtype=torch.float64, device=dev), t.sin() / t) * win * (base / o)
    return k.to(dtype)


def apply_bank(x, kernel, o, n):
    w = (kernel.shape[-1] - o) // 2
    xp = torch.nn.functional.pad(x.to(kernel.dtype)[:, None], (w, w + o))
    y = torch.nn.functional.conv1d(xp, kernel, stride=o).transpose(1, 2).reshape(x.shape[0], -1)
    return y[..., :-((-n * x.shape[-1]) // o)]


def window_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def timed(fn, reps, repeats, budget_ms=4000.0):
    """median over `repeats` windows of `reps` calls after a warm-up; `reps` shrinks so that a window stays within the budget"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    one = window_ms(fn, 1)
    reps = max(1, min(reps, int(budget_ms / repeats / max(one, 1e-3))))
    return statistics.median(window_ms(fn, reps) for _ in range(repeats)), reps


def attempt(fn):
    try:
        return fn()
    except torch.cuda.OutOfMemoryError as e:                     # (recorded, not hidden: see the docstring)
        return f"failed: {type(e).__name__}: {str(e)[:200]}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, L = 16, 163584
    x = torch.randn((B, L), device=dev, dtype=torch.float32, generator=torch.Generator(device=dev).manual_seed(0))
    lib = _lib.load()
    res = {"tool": "tools/bench_resample.py", "device": torch.cuda.get_device_name(0),
           "config": dict(B=B, L=L, dtype="float32", lowpass_filter_width=6, rolloff=0.99, reps=a.reps, repeats=a.repeats), "ratios": {}}
    for orig, new in ((27781, 22050), (2, 1), (1, 2)):
        g = math.gcd(orig, new)
        o, n = orig // g, new // g
        n_out = -((-n * L) // o)
        out = torch.empty((B, n_out), device=dev, dtype=torch.float32)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def launch():
            _lib.check(lib.specinv_resample(x.data_ptr(), out.data_ptr(), B, L, n_out, o, n, 6, 0.99, _lib.F32, 0, stream))

        r = {"L_out": n_out, "taps": 2 * math.ceil(6 * o / (min(o, n) * 0.99)) + 1}
        r["launch_ms"], r["launch_reps"] = timed(launch, a.reps, a.repeats)
        print(f"{orig}:{new}: launch {r['launch_ms']:.4f} ms", file=sys.stderr, flush=True)
        r["call_ms"], _ = timed(lambda: si.resample(x, orig, new), a.reps, a.repeats)
        r["min_bytes"] = 4 * B * (L + n_out)
        src = torch.empty(r["min_bytes"] // 8, device=dev, dtype=torch.float32)
        dst = torch.empty_like(src)
        r["copy_ms"], _ = timed(lambda: dst.copy_(src), a.reps, a.repeats)
        r["launch_over_copy"] = r["launch_ms"] / r["copy_ms"]
        r["bank_elements"] = n * (2 * math.ceil(6 * o / (min(o, n) * 0.99)) + o)
        y = si.resample(x, orig, new)
        ref = attempt(lambda: apply_bank(x, bank(o, n, torch.float64, dev), o, n))
        if isinstance(ref, str):
            r["reference_f64"] = ref
        else:
            scale = float(ref.abs().max())
            r["err_kernel"] = float((y.double() - ref).abs().max()) / scale
        print(f"{orig}:{new}: float64 restatement done", file=sys.stderr, flush=True)
        k32 = attempt(lambda: bank(o, n, torch.float32, dev))
        if isinstance(k32, str):
            r["bank_prebuilt_ms"] = r["bank_built_ms"] = k32
        else:
            y32 = attempt(lambda: apply_bank(x, k32, o, n))
            if isinstance(y32, str):
                r["bank_prebuilt_ms"] = r["bank_built_ms"] = y32
            else:
                if not isinstance(ref, str):
                    r["err_bank_f32"] = float((y32.double() - ref).abs().max()) / scale
                del y32
                r["bank_prebuilt_ms"], r["bank_prebuilt_reps"] = timed(lambda: apply_bank(x, k32, o, n), a.reps, a.repeats)
                r["bank_built_ms"], r["bank_built_reps"] = timed(lambda: apply_bank(x, bank(o, n, torch.float32, dev), o, n),
                                                                 a.reps, a.repeats)
                r["bank_prebuilt_over_launch"] = r["bank_prebuilt_ms"] / r["launch_ms"]
                r["bank_built_over_launch"] = r["bank_built_ms"] / r["launch_ms"]
        del ref, k32
        torch.cuda.empty_cache()
        res["ratios"][f"{orig}:{new}"] = {k: (round(v, 5) if isinstance(v, float) and v > 1e-3 else v) for k, v in r.items()}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
