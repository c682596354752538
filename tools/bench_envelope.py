#!/usr/bin/env python3
"""spectral_envelope (k_spectral_envelope) on a complex64 spectrogram at B 16, T 512, F 513 and 1025, n_iter 0 and 16, in
both layouts, against the same definition written as torch ops on the same GPU in the same run; pitch_shift with and without
preserve_formants; and the accuracy and property figures tests/test_gpu_envelope.py refers to.  One JSON line, also written to
profiles/envelope_bench.json.

    python tools/bench_envelope.py [--window MS] [--repeats M] [--out PATH]

per size, n_iter and layout:
launch_ms             specinv_spectral_envelope on a preallocated output and amin: events around as many calls as fill `window` ms (200:
                      enough work that the clock and the scheduler do not show), the median of `repeats` such windows
call_ms               si.spectral_envelope, the public function (argument checks, the item maxima, the output's allocation)
torch_ms              the definition as float32 torch ops: abs, log, then n_iter + 1 times irfft, a multiply, rfft and maximum over
                      the (B, T, F) array
min_bytes             the spectrogram read once (8 B per bin) and the envelope written once (4 B per bin); GBps = min_bytes / launch_ms
accuracy              per n_fft, on the parity test's input (B 3, two tiles plus one frame, complex64, order n_fft / 16): the largest
                      error in V against the float64 oracle of the float32 torch chain on the CPU (the yardstick) and of the kernel
pitch_shift           L 8192 at 16 kHz, 512 / 128, max_iter 8, +4 and -4 semitones on the synthetic voice: ms per call without and
                      with preserve_formants, and the envelope distance to the input in dB for both
The one condition: at n_iter 16 the fused launch is not slower than the torch form (exit status 1 otherwise).
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

import spectrogram_inversion_amd as si
from _envelope_oracle import envelope_distance_db, log_envelope, voice
from spectrogram_inversion_amd import _lib


def envelope_torch(spec_btf, order, n_iter, floor=1e-6):
    """The definition in float32 torch ops on a frame-major (B, T, F) array: V"""
    mag = spec_btf.abs()
    amin = mag.amax(dim=(1, 2), keepdim=True) * floor
    a0 = torch.log(torch.maximum(mag, amin))
    n_fft = 2 * (spec_btf.shape[-1] - 1)
    q = torch.arange(n_fft, device=spec_btf.device)
    lift = (torch.minimum(q, n_fft - q) <= order).to(torch.float32)
    v = torch.fft.rfft(torch.fft.irfft(a0, n_fft) * lift, n_fft).real
    for _ in range(n_iter):
        v = torch.fft.rfft(torch.fft.irfft(torch.maximum(a0, v), n_fft) * lift, n_fft).real
    return v


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


def rounded(d):
    return {n: (round(v, 5) if isinstance(v, float) and n != "max_diff_to_torch" else v) for n, v in d.items()}


def accuracy(dev):
    from test_gpu_envelope import TILE, _chain32, _spectrogram
    out = {}
    for n_fft in (256, 512, 1024, 2048):
        S = _spectrogram(n_fft, 3, 2 * TILE[n_fft] + 1, True, seed=n_fft)
        row = {}
        for n_iter in (0, 16):
            ref = log_envelope(S.numpy(), n_fft // 16, n_iter)
            chain = float(np.abs(_chain32(S, n_fft // 16, n_iter).double().numpy() - ref).max())
            got = si.spectral_envelope(S.to(dev), n_fft // 16, n_iter, log=True).double().cpu().numpy()
            kern = float(np.abs(got - ref).max())
            row[f"n_iter {n_iter}"] = {"v_min": round(float(ref.min()), 2), "v_max": round(float(ref.max()), 2),
                                       "float32_chain_max_err": chain, "kernel_max_err": kern, "ratio": round(kern / chain, 3)}
        out[str(n_fft)] = row
    return out


def pitch(dev, window, repeats):
    sr, length = 16000, 8192
    x = torch.from_numpy(voice(150.0, 1.0, length, sr)).float().to(dev)
    kw = dict(n_fft=512, hop_length=128, window=torch.hann_window(512), max_iter=8, verbose=False)
    out = {"config": dict(L=length, sample_rate=sr, n_fft=512, hop_length=128, max_iter=8, order=si.default_envelope_order(sr),
                          formant_iter=16)}
    x64 = x.double().cpu().numpy()
    for steps in (4, -4):
        r = 2.0 ** (steps / 12)
        plain = si.pitch_shift(x, sr, steps, **kw)
        kept = si.pitch_shift(x, sr, steps, preserve_formants=True, **kw)
        row = {"plain_ms": timed(lambda: si.pitch_shift(x, sr, steps, **kw), window, repeats),
               "preserve_formants_ms": timed(lambda: si.pitch_shift(x, sr, steps, preserve_formants=True, **kw), window, repeats),
               "distance_plain_db": envelope_distance_db(plain.double().cpu().numpy(), x64, 512, 128, 27, r),
               "distance_preserved_db": envelope_distance_db(kept.double().cpu().numpy(), x64, 512, 128, 27, r)}
        row["distance_ratio"] = row["distance_preserved_db"] / row["distance_plain_db"]
        out[f"{steps:+d}"] = rounded(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=200.0, help="ms of work per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "envelope_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, T = 16, 512
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev)
    res = {"tool": "tools/bench_envelope.py", "device": torch.cuda.get_device_name(0), "library": os.path.basename(_lib.LIB_PATH),
           "config": dict(B=B, T=T, dtype="complex64", floor=1e-6, window_ms=a.window, repeats=a.repeats), "sizes": {}}
    ok = True
    gen = torch.Generator(device=dev).manual_seed(0)
    for F in (513, 1025):
        order = (F - 1) // 8                                                     # n_fft / 16
        spec = torch.complex(torch.randn((B, F, T), device=dev, generator=gen), torch.randn((B, F, T), device=dev, generator=gen))
        spec_t = spec.transpose(1, 2).contiguous()
        amin = (spec.abs().amax(dim=(1, 2)) * 1e-6).contiguous()
        out = torch.empty((B, F, T), dtype=torch.float32, device=dev)
        out_t = torch.empty((B, T, F), dtype=torch.float32, device=dev)
        for n_iter in (0, 16):
            ref = envelope_torch(spec_t, order, n_iter)
            torch_ms = timed(lambda: envelope_torch(spec_t, order, n_iter), a.window, a.repeats)
            for frame_major in (False, True):
                src, dst = (spec_t, out_t) if frame_major else (spec, out)

                def launch():
                    _lib.check(lib.specinv_spectral_envelope(src.data_ptr(), dst.data_ptr(), amin.data_ptr(), B, F, T, order, n_iter, 1, 1,
                                                             int(frame_major), _lib.F32, 0, C.c_void_p(stream.cuda_stream)))

                r = {"launch_ms": timed(launch, a.window, a.repeats),
                     "call_ms": timed(lambda: si.spectral_envelope(src, order, n_iter, log=True, frame_major=frame_major), a.window,
                                      a.repeats),
                     "torch_ms": torch_ms}
                r["min_bytes"] = B * F * T * 12
                r["GBps"] = r["min_bytes"] / (r["launch_ms"] * 1e-3) / 1e9
                r["torch_over_launch"] = r["torch_ms"] / r["launch_ms"]
                launch()
                got = dst if frame_major else dst.transpose(1, 2)
                r["max_diff_to_torch"] = float((got - ref).abs().max())
                ok = ok and (n_iter != 16 or r["launch_ms"] <= r["torch_ms"])
                res["sizes"][f"F {F} n_iter {n_iter} {'(B, T, F)' if frame_major else '(B, F, T)'}"] = rounded(r)
            del ref
    res["accuracy"] = accuracy(dev)
    res["pitch_shift"] = pitch(dev, a.window, a.repeats)
    res["fused_not_slower_at_16"] = ok
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
