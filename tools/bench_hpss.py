#!/usr/bin/env python3
"""hpss (k_hpss) on a complex64 spectrogram at B 16, F 513, T 512 for the sizes (31, 31) and (127, 127), components and
medians only, against the same definition written as torch ops on the same GPU in the same run: one JSON line, also written to
profiles/hpss_bench.json.

    python tools/bench_hpss.py [--reps N] [--repeats M] [--out PATH]

per size and mode:
launch_ms             specinv_hpss on preallocated outputs: events around `reps` calls, the median of `repeats` such windows
call_ms               si.hpss / si.hpss_medians, the public function (argument checks, the outputs' allocation), likewise
torch_ms              the definition as torch ops in float64: index_select through the reflection map, unfold, median(-1), then the
                      mask arithmetic (a (B, F, T, k) float64 view per axis: 4.3 GB materialised by median at k = 127)
torch_f32_ms          the same on the float32 magnitude (what a plain torch port would do; the masks lose float32 roundings)
min_bytes             what the kernel has to move: the spectrogram read once (8 B per bin) and both outputs written once (2 x 8 B for
                      the components - 24 B per bin - and 2 x 4 B for the medians); GBps = min_bytes / launch_ms
equal                 the kernel's output against the torch form's: medians bit for bit, components within 2^-23 per part
The one condition: at (31, 31) the fused launch is not slower than the torch form (exit status 1 otherwise).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import spectrogram_inversion_amd as si
from spectrogram_inversion_amd import _lib


def refl_map(n, k, dev):
    i = torch.arange(-(k // 2), n + k // 2, device=dev)
    j = torch.remainder(i, 2 * n)
    return torch.where(j < n, j, 2 * n - 1 - j)


def medians_torch(a, k_h, k_p):
    F, T = a.shape[-2:]
    harm = a.index_select(-1, refl_map(T, k_h, a.device)).unfold(-1, k_h, 1).median(-1).values
    perc = a.index_select(-2, refl_map(F, k_p, a.device)).unfold(-2, k_p, 1).median(-1).values
    return harm, perc


def soft_torch(x, r, power, split, tiny):
    z = torch.maximum(x, r)
    small = z < tiny
    z = torch.where(small, torch.ones_like(z), z)
    a, b = x / z, r / z
    if power == 2:
        a, b = a * a, b * b
    elif power != 1:
        a, b = a ** power, b ** power
    return torch.where(small, torch.full_like(a, 0.5 if split else 0.0), a / torch.where(small, torch.ones_like(a), a + b))


def hpss_torch(spec, k_h, k_p, mode, work=torch.float64):
    """DESIGN 3.22 in torch ops on the tensor's device, power 2 and margin 1, everything after the magnitude in `work`"""
    if work == torch.float64:
        a = torch.sqrt(spec.real.double() ** 2 + spec.imag.double() ** 2)
    else:
        a = spec.abs()
    harm, perc = medians_torch(a, k_h, k_p)
    if mode == "medians":
        return harm.float(), perc.float()
    tiny = torch.finfo(torch.float32).tiny
    mh, mp = soft_torch(harm, perc, 2, True, tiny), soft_torch(perc, harm, 2, True, tiny)
    if work == torch.float64:
        wide = spec.to(torch.complex128)
        return (wide * mh).to(spec.dtype), (wide * mp).to(spec.dtype)
    return spec * mh, spec * mp


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hpss_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, F, T = 16, 513, 512
    gen = torch.Generator(device=dev).manual_seed(0)
    spec = torch.complex(torch.randn((B, F, T), device=dev, generator=gen), torch.randn((B, F, T), device=dev, generator=gen))
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev)
    res = {"tool": "tools/bench_hpss.py", "device": torch.cuda.get_device_name(0), "library": os.path.basename(_lib.LIB_PATH),
           "config": dict(B=B, F=F, T=T, dtype="complex64", power=2.0, margin=1.0, reps=a.reps, repeats=a.repeats), "sizes": {}}
    ok = True
    for k in (31, 127):
        for mode in ("components", "medians"):
            code = _lib.HPSS_COMPONENTS if mode == "components" else _lib.HPSS_MEDIANS
            out_a = torch.empty((B, F, T), dtype=torch.complex64 if mode == "components" else torch.float32, device=dev)
            out_b = torch.empty_like(out_a)

            def launch():
                _lib.check(lib.specinv_hpss(spec.data_ptr(), out_a.data_ptr(), out_b.data_ptr(), B, F, T, k, k, 2.0, 1.0, 1.0, code, 1,
                                            _lib.F32, 0, C.c_void_p(stream.cuda_stream)))

            call = (lambda: si.hpss(spec, k)) if mode == "components" else (lambda: si.hpss_medians(spec, k))
            slow, few = max(1, a.reps // 25), min(3, a.repeats)            # (the torch forms take tens of milliseconds and more)
            r = {"launch_ms": timed(launch, a.reps, a.repeats), "call_ms": timed(call, a.reps, a.repeats),
                 "torch_ms": timed(lambda: hpss_torch(spec, k, k, mode), slow, few),
                 "torch_f32_ms": timed(lambda: hpss_torch(spec, k, k, mode, torch.float32), slow, few)}
            r["min_bytes"] = B * F * T * (24 if mode == "components" else 16)
            r["GBps"] = r["min_bytes"] / (r["launch_ms"] * 1e-3) / 1e9
            r["torch_over_launch"] = r["torch_ms"] / r["launch_ms"]
            r["torch_f32_over_launch"] = r["torch_f32_ms"] / r["launch_ms"]
            launch()
            ref = hpss_torch(spec, k, k, mode)
            if mode == "medians":
                r["equal"] = bool(torch.equal(out_a, ref[0]) and torch.equal(out_b, ref[1]))
            else:
                r["equal"] = all(bool(((torch.view_as_real(o).double() - torch.view_as_real(w).double()).abs()
                                       <= 2.0 ** -23 * torch.view_as_real(w).double().abs()).all())
                                 for o, w in zip((out_a, out_b), ref))
            ok = ok and r["equal"] and (k != 31 or r["launch_ms"] <= r["torch_ms"])
            res["sizes"][f"{k},{k} {mode}"] = {n: (round(v, 5) if isinstance(v, float) else v) for n, v in r.items()}
            del ref
    res["fused_not_slower_at_31"] = ok
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
