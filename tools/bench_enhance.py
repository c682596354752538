#!/usr/bin/env python3
"""spectral_gain (k_enhance) at B 16, F 513, T 512, complex64, both layouts and both rules, against the same
definition written as torch ops (float64, one step per frame) on the same GPU in the same run.  One JSON line, also written to
profiles/enhance_bench.json.

    python tools/bench_enhance.py [--window MS] [--repeats M] [--out PATH]

per layout and rule:
launch_ms     specinv_enhance on preallocated outputs (G, xi, sigma2 and the state): events around as many calls as fill `window`
              ms, the median of `repeats` such windows (tools/bench_yin.py's `timed`)
call_ms       si.spectral_gain(..., return_snr=True, return_noise=True, return_state=True), the public function
torch_ms      the definition in torch ops, E1 by the device's scheme (series and Chebyshev table); the median of three runs
agreement     the largest relative difference of G and sigma2 between the two
`library` names the library measured: a variant built with -DSPECINV_ENHANCE_BINS=16 or 32 (build_lib(extra_flags=..., out=...),
selected with SPECINV_LIB) gives the figures of the narrower bin groups.  Nothing is required of the ratio; the tool writes down
what comes out.
"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch

import spectrogram_inversion_amd as si
from bench_yin import timed
from spectrogram_inversion_amd import _lib

EULER = 0.57721566490153286061


def e1_tables(dev):
    text = open(os.path.join(ROOT, "spectrogram_inversion_amd", "csrc", "enhance_e1_table.h")).read()

    def array(name):
        body = re.search(name + r"(?:\[\w+(?: \+ 1)?\])+ = \{(.*?)\};", text, re.S).group(1)
        return torch.tensor([float(x) for x in re.findall(r"-?\d[\d.]*(?:e[-+]?\d+)?", body)], dtype=torch.float64, device=dev)

    mid = array("kE1Mid")
    return array("kE1SeriesCoef"), mid, array("kE1Scale"), array("kE1Cheb").reshape(len(mid), -1)


def e1_torch(v, tables):
    series, mid, scale, cheb = tables
    x = v.clamp(max=1.0)
    s = torch.full_like(x, float(series[-1]))
    for k in range(len(series) - 2, -1, -1):
        s = s * x + series[k]
    low = (s * x - torch.log(x)) - EULER
    y = v.clamp(min=1.0, max=700.0)
    j = (torch.frexp(y)[1] - 1).clamp(max=len(mid) - 1).long()
    rv = 1.0 / y
    t = (2.0 * rv - mid[j]) * scale[j]
    tab = cheb[j]
    b1, b2 = torch.zeros_like(y), torch.zeros_like(y)
    for k in range(tab.shape[-1] - 1, 0, -1):
        b1, b2 = tab[..., k] + (2.0 * t * b1 - b2), b1
    high = torch.exp(-y) * rv * (tab[..., 0] + (t * b1 - b2))
    return torch.where(v <= 1.0, low, torch.where(v <= 700.0, high, torch.zeros_like(v)))


def enhance_torch(spec, rule, frame_major, tables, alpha=0.98, xi_min_db=-25.0, gain_floor_db=-20.0, init_frames=5, a_pow=0.8,
                  a_spp=0.9, prior_snr_db=15.0):
    """(G, sigma2) in float64, in spec's layout: the module's definition, one step of element-wise ops per frame"""
    t_dim = 1 if frame_major else 2
    n_frames = spec.shape[t_dim]
    xi1 = 10.0 ** (prior_snr_db / 10.0)
    c, xi_min, g_min = xi1 / (1.0 + xi1), 10.0 ** (xi_min_db / 10.0), 10.0 ** (gain_floor_db / 20.0)
    re, im = spec.real.double(), spec.imag.double()
    P = re * re + im * im
    G_out, sig_out = torch.empty_like(P), torch.empty_like(P)
    n0 = min(init_frames, n_frames)
    sig = P.narrow(t_dim, 0, n0).sum(t_dim) / n0
    pbar = torch.zeros_like(sig)
    a2 = None
    for l in range(n_frames):
        Pl = P.select(t_dim, l)
        gp = (Pl / sig.clamp(min=1e-300)).clamp(max=1e300)
        p = 1.0 / (1.0 + (1.0 + xi1) * torch.exp(-(gp * c)))
        pbar = a_spp * pbar + (1.0 - a_spp) * p
        p = torch.where(pbar > 0.99, p.clamp(max=0.99), p)
        sig = a_pow * sig + (1.0 - a_pow) * ((1.0 - p) * Pl + p * sig)
        den = sig.clamp(min=1e-300)
        g = (Pl / den).clamp(max=1e300)
        r = torch.ones_like(g) if a2 is None else (a2 / den).clamp(max=1e300)
        xi = (alpha * r + (1.0 - alpha) * (g - 1.0).clamp(min=0.0)).clamp(min=xi_min)
        w = xi / (1.0 + xi)
        G = w if rule == "wiener" else w * torch.exp(0.5 * e1_torch((w * g).clamp(min=1e-12), tables))
        G = G.clamp(min=g_min, max=1.0)
        a2 = (G * G) * Pl
        G_out.select(t_dim, l).copy_(G)
        sig_out.select(t_dim, l).copy_(sig)
    return G_out, sig_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=200.0, help="ms of work per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "enhance_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, F, T = 16, 513, 512
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    gen = torch.Generator(device=dev).manual_seed(0)
    # noise whose level differs from bin to bin, and bursts 20 dB above it in a third of the frames
    z = torch.randn((B, F, T, 2), device=dev, generator=gen) * (10.0 ** (2.0 * torch.rand((B, F, 1, 1), device=dev, generator=gen) - 1.0))
    burst = (torch.rand((B, 1, T // 16, 1), device=dev, generator=gen) < 0.33).repeat_interleave(16, dim=2)
    z = torch.where(burst & (torch.rand((B, F, 1, 1), device=dev, generator=gen) < 0.5), 10.0 * z, z)
    x_bm = torch.view_as_complex(z.contiguous())
    tables = e1_tables(dev)
    res = {"tool": "tools/bench_enhance.py", "device": torch.cuda.get_device_name(0), "library": os.path.basename(_lib.LIB_PATH),
           "config": dict(B=B, F=F, T=T, dtype="complex64", window_ms=a.window, repeats=a.repeats), "cases": {}}
    xi1, xi_min, g_min = 10.0 ** 1.5, 10.0 ** -2.5, 10.0 ** -1.0
    for frame_major in (False, True):
        x = x_bm.transpose(1, 2).contiguous() if frame_major else x_bm
        G, xi, sig = (torch.empty(x.shape, device=dev) for _ in range(3))
        state = torch.empty((B, F, 3), dtype=torch.float64, device=dev)
        for rule in ("wiener", "lsa"):
            def launch():
                _lib.check(lib.specinv_enhance(x.data_ptr(), None, None, sig.data_ptr(), None, G.data_ptr(), xi.data_ptr(), None,
                                               state.data_ptr(), B, F, T, 5, _lib.ENHANCE_TRACK, _lib.ENHANCE_RULES[rule], 0.8, 0.9,
                                               xi1, 0.98, xi_min, g_min, 1, int(frame_major), _lib.F32, 0, sp))

            def call():
                return si.spectral_gain(x, rule=rule, return_snr=True, return_noise=True, return_state=True, frame_major=frame_major)

            r = {"launch_ms": timed(launch, a.window, a.repeats), "call_ms": timed(call, a.window, a.repeats)}
            enhance_torch(x[:, :32] if frame_major else x[:, :, :32], rule, frame_major, tables)        # warm-up
            runs = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                Gt, st = enhance_torch(x, rule, frame_major, tables)
                torch.cuda.synchronize()
                runs.append((time.perf_counter() - t0) * 1e3)
            r["torch_ms"] = statistics.median(runs)
            r["torch_over_launch"] = r["torch_ms"] / r["launch_ms"]
            r["torch_over_call"] = r["torch_ms"] / r["call_ms"]
            launch()
            torch.cuda.synchronize()
            r["agreement"] = {"gain_max_rel_diff": float((G.double() / Gt - 1.0).abs().max()),
                              "noise_max_rel_diff": float((sig.double() / st - 1.0).abs().max())}
            res["cases"][f"{'frame' if frame_major else 'bin'}-major {rule}"] = {k: (round(v, 5) if isinstance(v, float) else v)
                                                                                 for k, v in r.items()}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
