#!/usr/bin/env python3
"""phase_vocoder(phase_lock="identity") (k_pvoc_lock_scan + k_pvoc_lock_apply) beside the unlocked launch and beside
the same locked definition written as torch ops on the same GPU, and what locking is worth against the iteration count: one JSON
line, also written to profiles/pvoc_lock_bench.json.

    python tools/bench_pvoc_lock.py [--reps N] [--repeats M] [--out PATH] [--no-table]

`timing`, per shape (B 16, 512 input frames of the chirp + 0.3 noise at rate 0.8 -> 640; 1024 / 256 and 2048 / 512; both dtypes):
locked_ms             Plan.phase_vocoder(phase_lock="identity") on a warm plan: events around `reps` calls, median of `repeats` windows
unlocked_ms           Plan.phase_vocoder on the same plan in the same run, likewise
call_ms               si.phase_vocoder(phase_lock="identity"), the public function
torch_ms              the locked definition as torch ops (neighbour comparisons, cummax / cummin for the peak below and above, a gather)
apply_waves, band     the waves of k_pvoc_lock_apply and the bins each takes (kPvocLockBand)
err_kernel, err_torch max |P - P_ref| / max |P_ref| against the torch form with float64 angles on the input's bits
`inconsistency`: || |STFT(y)| - |P| || / || |P| || of y = time_stretch(x, rate, max_iter=n, tol=0) for n = 0, 5, 10, 30, both starts,
on the harmonic signal (eight harmonics, 1 % vibrato, 1 % noise) and the chirp + 0.3 noise at 1024 / 256, 300 frames, float32.
No gate: the figures go into DESIGN 3.21.
"""
import argparse
import json
import math
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import spectrogram_inversion_amd as si
from spectrogram_inversion_amd.plan import args_helper, get_plan


def band_height():
    text = open(os.path.join(ROOT, "spectrogram_inversion_amd", "csrc", "kernels_pvoc_lock.h")).read()
    return int(re.search(r"kPvocLockBand = (\d+)", text).group(1))


def lock_torch(spec, rate, n_fft, hop, angle=torch.float32):
    """DESIGN 3.21 in torch ops on the tensor's device: the angles in `angle`, everything after them in float64."""
    n_freq = spec.shape[-2]
    onesided = n_freq != n_fft
    dev = spec.device
    n_out = si.stretched_frames(spec.shape[-1], rate)
    t = torch.arange(n_out, dtype=torch.float64, device=dev) * rate
    fl = torch.floor(t)
    i = fl.to(torch.int64)
    a = t - fl
    sp = torch.cat([spec, spec.new_zeros(spec.shape[:-1] + (2,))], -1)
    s0, s1 = sp[..., i], sp[..., i + 1]
    th0 = torch.atan2(s0.imag.to(angle), s0.real.to(angle)).double()
    th1 = torch.atan2(s1.imag.to(angle), s1.real.to(angle)).double()
    m = a * s1.to(torch.complex128).abs() + (1 - a) * s0.to(torch.complex128).abs()
    k = torch.arange(n_freq, dtype=torch.int64, device=dev)
    adv = (2 * math.pi * torch.where(k <= n_fft // 2, k, k - n_fft).double() * hop / n_fft)[:, None]
    d = th1 - th0 - adv
    d = d - 2 * math.pi * torch.round(d / (2 * math.pi)) + adv
    phi = torch.cumsum(torch.cat([th0[..., :1], d[..., :-1]], -1), -1)
    # peaks
    re, im = s0.real.double(), s0.imag.double()
    q = re * re + im * im
    peak = torch.ones_like(q, dtype=torch.bool)
    for step in (-2, -1, 1, 2):
        if onesided:
            drop = (k + step < 0) | (k + step >= n_freq)
            idx = (k + step).clamp(0, n_freq - 1)
        else:
            drop = (2 * k + step) % n_fft == 0
            idx = (k + step) % n_fft
        peak &= (q > q[..., idx, :]) | drop[:, None]
    # the peak at or below and the peak at or above every bin, over three turns of a two-sided spectrum
    turns = 1 if onesided else 3
    kk = torch.arange(turns * n_freq, dtype=torch.int64, device=dev) - (0 if onesided else n_freq)
    pk = peak if onesided else torch.cat([peak] * 3, -2)
    far = 4 * n_freq
    below = torch.cummax(torch.where(pk, kk[:, None], -far), -2).values
    above = torch.cummin(torch.where(pk, kk[:, None], far).flip(-2), -2).values.flip(-2)
    if not onesided:
        below, above = below[..., n_freq:2 * n_freq, :], above[..., n_freq:2 * n_freq, :]
    kc = k[:, None]
    dl, dh = kc - below, above - kc
    pl, ph = below % n_freq, above % n_freq
    al = pl if onesided else torch.where(pl > n_freq // 2, n_freq - pl, pl)
    ah = ph if onesided else torch.where(ph > n_freq // 2, n_freq - ph, ph)
    take_lo = (dl < dh) | ((dl == dh) & ((al < ah) | ((al == ah) & (pl <= ph))))
    has = (below > -far) | (above < far)
    owner = torch.where(take_lo & (below > -far) | (above >= far), pl, ph)
    psi = torch.where(has, torch.gather(phi - th0, -2, owner) + th0, phi)
    return torch.polar(m, psi)


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


def chirp(batch, n, dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64, device=dev)
    tone = torch.sin(2 * math.pi * (0.02 * t + 0.5 * (0.3 / n) * t * t))
    return tone + 0.3 * torch.randn((batch, n), device=dev, dtype=torch.float64, generator=gen)


def harmonic(batch, n, dev, seed, f0=0.031):
    gen = torch.Generator(device=dev).manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64, device=dev)
    inst = 2 * math.pi * f0 * (t + 0.01 / (2 * math.pi * 0.0004) * torch.sin(2 * math.pi * 0.0004 * t))
    x = sum(torch.sin(h * inst + 0.7 * h) / h for h in range(1, 9))
    return x + 0.01 * torch.randn((batch, n), device=dev, dtype=torch.float64, generator=gen)


def rounded(r):
    return {k: (round(v, 5) if isinstance(v, float) and v > 1e-3 else v) for k, v in r.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--no-table", action="store_true", help="skip the inconsistency table")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pvoc_lock_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, T, rate = 16, 512, 0.8
    band = band_height()
    res = {"tool": "tools/bench_pvoc_lock.py", "device": torch.cuda.get_device_name(0),
           "config": dict(B=B, T=T, rate=rate, reps=a.reps, repeats=a.repeats, band=band), "timing": []}
    maxabs = lambda v: float(v.abs().max())                                                # noqa: E731
    for n_fft, hop in ((1024, 256), (2048, 512)):
        for dtype in (torch.float32, torch.float64):
            kw = dict(hop_length=hop, window=torch.hann_window(n_fft, dtype=dtype))
            spec = si.stft(chirp(B, (T - 1) * hop, dev, 0).to(dtype), n_fft, **kw)          # tools/bench_pvoc.py's signal
            n_out = si.stretched_frames(T, rate)
            plan = get_plan(args_helper(spec, **kw), B, n_out, dtype, dev)
            r = dict(n_fft=n_fft, hop=hop, dtype=str(dtype).split(".")[1], T_out=n_out,
                     locked_ms=timed(lambda: plan.phase_vocoder(spec, rate, "identity"), a.reps, a.repeats),
                     unlocked_ms=timed(lambda: plan.phase_vocoder(spec, rate), a.reps, a.repeats),
                     call_ms=timed(lambda: si.phase_vocoder(spec, rate, phase_lock="identity", **kw), a.reps, a.repeats),
                     torch_ms=timed(lambda: lock_torch(spec, rate, n_fft, hop, angle=dtype), max(1, a.reps // 20), a.repeats))
            r["locked_over_unlocked"] = r["locked_ms"] / r["unlocked_ms"]
            r["torch_over_locked"] = r["torch_ms"] / r["locked_ms"]
            r["apply_waves"] = B * ((n_out + 63) // 64) * ((spec.shape[1] + band - 1) // band)
            r["band"] = band
            ref = lock_torch(spec, rate, n_fft, hop, angle=torch.float64)
            r["err_kernel"] = maxabs(si.phase_vocoder(spec, rate, phase_lock="identity", **kw).to(torch.complex128) - ref) / maxabs(ref)
            r["err_torch"] = maxabs(lock_torch(spec, rate, n_fft, hop, angle=dtype) - ref) / maxabs(ref)
            res["timing"].append(rounded(r))
            del ref
    res["inconsistency"] = []
    if not a.no_table:
        n_fft, hop, frames = 1024, 256, 300
        kw = dict(hop_length=hop, window=torch.hann_window(n_fft))
        rel = lambda x, y: float(torch.linalg.norm((x - y).double()) / torch.linalg.norm(y.double()))   # noqa: E731
        for name, make in (("harmonic", harmonic), ("chirp_noise", chirp)):
            x = make(1, (frames - 1) * hop, dev, 9).float()
            for rt in (0.5, 0.8):
                row = dict(signal=name, n_fft=n_fft, hop=hop, rate=rt)
                for lock in (None, "identity"):
                    target = si.phase_vocoder(si.stft(x, n_fft, **kw), rt, phase_lock=lock, **kw).abs()
                    for it in (0, 5, 10, 30):
                        y = si.time_stretch(x, rt, n_fft, max_iter=it, phase_lock=lock, verbose=False, tol=0, **kw)
                        row[f"{'locked' if lock else 'unlocked'}_{it}"] = round(rel(si.stft(y, n_fft, **kw).abs(), target), 4)
                res["inconsistency"].append(row)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
