#!/usr/bin/env python3
"""wsola, ola and time_stretch_hpss at B 16, L 163 584 (7.4 s at 22.05 kHz) in float32, the kernels against the same
definition written as torch ops on the same GPU in the same run: one JSON line, also written to profiles/wsola_bench.json.

    python tools/bench_wsola.py [--reps N] [--repeats M] [--out PATH]

wsola      1024 / 512 / tolerance 512 at rate 0.8;   ola   256 / 128 at rate 0.8.   Per entry:
launch_ms        specinv_wsola on preallocated outputs: events around `reps` calls, the median of `repeats` such windows
call_ms          si.wsola / si.ola, the public function (argument checks, the centres, the allocations), likewise
ola_only_ms      (wsola) the same launch at tolerance 0: k_wsola_ola and a memset;  lags_ms = launch_ms - ola_only_ms is k_wsola_lags
torch_lags_ms    the lag chain in torch ops, float64: per frame a gather of p, a grouped conv1d over the search region and an arg-max
                 under the tie rule, the lags kept on the device (no read-back between frames); torch_f32 the same in float32 (its lags may differ)
torch_ola_ms     the overlap-add in torch ops, float64: a gather of the frames, the window, index_add_ of numerator and window sum
lags_equal       the torch chain's lags against the kernel's (float64 chain: must be true)
y_close          the kernel's output against the torch overlap-add on the same lags, within 2^-22 |y| + 2^-40
fma              products of the chain, B (M - 1) N (2 D + 1); GFMA_per_s over lags_ms (float64 fmas, 16 workgroups on 16 of the
                 chip's compute units: one per item)
time_stretch_hpss against time_stretch (phase_lock='identity') at 1024 / 256, both at their default 32 iterations: call_ms each.
Exit status 1 if the lags differ or an output is not close; the speed is reported, not judged.
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
from spectrogram_inversion_amd import _lib, tsm


def padded(x, pad, dtype):
    return torch.nn.functional.pad(x.to(dtype), (pad, pad))


def corr_conv1d(region, p):
    return torch.nn.functional.conv1d(region[None], p[:, None, :], groups=p.shape[0])[0]


def corr_unfold(region, p):
    """where the convolution library has no float64 grouped conv1d: the same sums as a batched matrix-vector product"""
    return torch.einsum("bdn,bn->bd", region.unfold(1, p.shape[1], 1), p)


CORR = [corr_conv1d]


def lags_torch(xp, pad, a, N, Hs, D):
    """the lag chain on xp (B, pad + L + pad), centres a (a list of ints): (B, M) int64 on the device"""
    B = xp.shape[0]
    n = torch.arange(N, device=xp.device)
    lags = [torch.zeros(B, dtype=torch.int64, device=xp.device)]
    d = torch.arange(-D, D + 1, device=xp.device)
    prefer = -(2 * d.abs() + (d > 0))                                                 # among equals: the smallest |d|, then the negative
    for m in range(len(a) - 1):
        start = a[m] + lags[m] - N // 2 + Hs + pad                                   # (B,)
        p = xp.gather(1, start[:, None] + n[None, :])                                 # (B, N)
        lo = a[m + 1] - N // 2 - D + pad
        region = xp[:, lo:lo + N + 2 * D]                                             # (B, N + 2 D)
        c = CORR[0](region, p)                                                        # (B, 2 D + 1): a correlation
        tied = c == c.max(dim=1, keepdim=True).values                                 # (silent frames past the input's end tie)
        lags.append(d[torch.where(tied, prefer, prefer.min() - 1).argmax(dim=1)])
    return torch.stack(lags, dim=1)


def ola_torch(xp, pad, a, lags, w, N, Hs, n_out):
    B, M = lags.shape
    n = torch.arange(N, device=xp.device)
    u = torch.as_tensor(a, device=xp.device)[None, :] + lags - N // 2 + pad           # (B, M)
    frames = xp.gather(1, (u[:, :, None] + n[None, None, :]).reshape(B, -1)).reshape(B, M, N) * w
    where = (torch.arange(M, device=xp.device)[:, None] * Hs + n[None, :]).reshape(-1)
    acc = torch.zeros((B, (M - 1) * Hs + N), dtype=xp.dtype, device=xp.device).index_add_(1, where, frames.reshape(B, -1))
    ow = torch.zeros((M - 1) * Hs + N, dtype=xp.dtype, device=xp.device).index_add_(0, where, w.repeat(M))
    ow = torch.where(ow >= 1e-3, ow, torch.ones_like(ow))
    return (acc / ow)[:, N // 2:N // 2 + n_out]


def window_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def timed(fn, reps, repeats):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    return statistics.median(window_ms(fn, reps) for _ in range(repeats))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wsola_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, L, rate = 16, 163584, 0.8
    gen = torch.Generator(device=dev).manual_seed(0)
    t = torch.arange(L, device=dev, dtype=torch.float64)
    f = 0.02 + 1.4 * torch.rand((B, 3, 1), device=dev, generator=gen, dtype=torch.float64)
    x = ((torch.sin(f * t) * torch.tensor([1.0, 0.5, 0.25], device=dev, dtype=torch.float64)[None, :, None]).sum(1)
         + 0.1 * torch.randn((B, L), device=dev, generator=gen, dtype=torch.float64)).float()
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev)
    res = {"tool": "tools/bench_wsola.py", "device": torch.cuda.get_device_name(0), "library": os.path.basename(_lib.LIB_PATH),
           "config": dict(B=B, L=L, rate=rate, dtype="float32", reps=a.reps, repeats=a.repeats)}
    ok = True
    try:
        corr_conv1d(torch.zeros((2, 24), dtype=torch.float64, device=dev), torch.zeros((2, 8), dtype=torch.float64, device=dev))
        torch.cuda.synchronize()
    except RuntimeError:
        CORR[0] = corr_unfold
    res["config"]["torch_correlation"] = CORR[0].__name__
    n_out = -(-L * 5 // 4)
    assert n_out == tsm.math.ceil(L / rate)
    for name, N, Hs, D in (("wsola", 1024, 512, 512), ("ola", 256, 128, 0)):
        M = tsm.wsola_frames(n_out, N, Hs)
        centres_np = tsm.wsola_centres(M, Hs, rate)
        centres = torch.from_numpy(centres_np).to(dev)
        w = torch.hann_window(N).to(dev)
        y = torch.empty((B, n_out), device=dev)
        lags = torch.empty((B, M), dtype=torch.int32, device=dev)

        def launch(tol=D):
            _lib.check(lib.specinv_wsola(x.data_ptr(), centres.data_ptr(), w.data_ptr(), lags.data_ptr(), y.data_ptr(), B, L, n_out, M,
                                         N, Hs, tol, _lib.F32, 0, C.c_void_p(stream.cuda_stream)))

        call = (lambda: si.wsola(x, rate, N, Hs, D)) if D else (lambda: si.ola(x, rate, N, Hs))
        r = {"frame": N, "hop": Hs, "tolerance": D, "n_out": n_out, "n_frames": M,
             "launch_ms": timed(launch, a.reps, a.repeats), "call_ms": timed(call, a.reps, a.repeats)}
        pad = 2 * N + 2 * D + Hs
        xp64, w64 = padded(x, pad, torch.float64), w.double()
        alist = [int(v) for v in centres_np]
        few = min(3, a.repeats)
        if D:
            r["ola_only_ms"] = timed(lambda: launch(0), a.reps, a.repeats)
            r["lags_ms"] = r["launch_ms"] - r["ola_only_ms"]
            r["torch_lags_ms"] = timed(lambda: lags_torch(xp64, pad, alist, N, Hs, D), 1, few)
            xp32 = padded(x, pad, torch.float32)
            r["torch_f32_lags_ms"] = timed(lambda: lags_torch(xp32, pad, alist, N, Hs, D), 1, few)
            r["fma"] = B * (M - 1) * N * (2 * D + 1)
            r["GFMA_per_s"] = r["fma"] / (r["lags_ms"] * 1e-3) / 1e9
            r["torch_over_lags"] = r["torch_lags_ms"] / r["lags_ms"]
            r["torch_f32_over_lags"] = r["torch_f32_lags_ms"] / r["lags_ms"]
            launch()
            want = lags_torch(xp64, pad, alist, N, Hs, D)
            r["lags_equal"] = bool(torch.equal(want, lags.long()))
            r["lags_f32_equal"] = bool(torch.equal(lags_torch(xp32, pad, alist, N, Hs, D), lags.long()))
            r["lags_nonzero"] = int((lags != 0).sum())
            ok = ok and r["lags_equal"]
        launch()
        l64 = lags.long()
        r["torch_ola_ms"] = timed(lambda: ola_torch(xp64, pad, alist, l64, w64, N, Hs, n_out), max(1, a.reps // 4), few)
        r["torch_over_ola"] = r["torch_ola_ms"] / (r["ola_only_ms"] if D else r["launch_ms"])
        ref = ola_torch(xp64, pad, alist, l64, w64, N, Hs, n_out)
        r["y_close"] = bool(((y.double() - ref).abs() <= 2.0 ** -22 * ref.abs() + 2.0 ** -40).all())
        ok = ok and r["y_close"]
        res[name] = {k: (round(v, 5) if isinstance(v, float) else v) for k, v in r.items()}
        del xp64, ref
    kw = dict(n_fft=1024, hop_length=256, window=torch.hann_window(1024).to(dev))
    few = min(3, a.repeats)
    ts = timed(lambda: si.time_stretch(x, rate, phase_lock="identity", **kw), 2, few)
    th = timed(lambda: si.time_stretch_hpss(x, rate, **kw), 2, few)
    y_h = si.time_stretch_hpss(x, rate, **kw)
    res["time_stretch_hpss"] = {"n_fft": 1024, "hop": 256, "max_iter": 32, "time_stretch_ms": round(ts, 4),
                                "time_stretch_hpss_ms": round(th, 4), "ratio": round(th / ts, 4),
                                "same_length": bool(y_h.shape == si.time_stretch(x, rate, phase_lock="identity", **kw).shape),
                                "finite": bool(torch.isfinite(y_h).all())}
    ok = ok and res["time_stretch_hpss"]["same_length"] and res["time_stretch_hpss"]["finite"]
    res["ok"] = ok
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
