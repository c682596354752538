#!/usr/bin/env python3
"""gla_projection, forward and backward, at B 16, n_fft 1024, hop 256, 512 frames, in float32 and float64, the backward pass on the
fused kernel (k_wave_proj_adjoint) and on the staged path (SPECINV_PROJ_ADJ_FUSED=0: proj_adjoint_stages, what MISI's and AGLA's
sweeps run): one JSON line, also written to profiles/projection_bench.json.

    python tools/bench_projection.py [--reps N] [--out PATH]

per dtype:
forward_ms            gla_projection without grad on a warm plan (stft_internal, k_project, istft_internal)
backward_ms           torch.autograd.grad through the layer, per path
adjoint_call_ms       specinv_project_adjoint alone, events around `reps` calls, per path: the fused kernel + the overlap-add and
                      fold launches, or the division, two transforms, k_misi_proj_adjoint, the inverse transform and the fold
staged_over_fused     adjoint_call_ms staged / fused
grad_rel_l2           fused against staged, x and mag
bytes_per_frame       the reals DESIGN 3.16 counts per frame, times the element size
The kernel's own time is in a kernel trace of this script (k_wave_proj_adjoint's row).  No gate: the figures go into DESIGN 3.16.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import spectrogram_inversion_amd as si
from spectrogram_inversion_amd.plan import Plan, args_helper


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def one_dtype(dtype, B, T, n_fft, hop, reps, dev):
    F = n_fft // 2 + 1
    kw = dict(hop_length=hop, window=torch.hann_window(n_fft, dtype=dtype))
    gen = torch.Generator(device=dev).manual_seed(0)
    args = args_helper(torch.empty((F, 1), dtype=dtype), **kw)
    L = args.signal_length(T)
    x = torch.randn((B, L), device=dev, dtype=dtype, generator=gen)
    other = torch.randn((B, L), device=dev, dtype=dtype, generator=gen)
    mag = si.stft(other, n_fft=n_fft, **kw).abs() * (0.5 + torch.rand((B, F, T), device=dev, dtype=dtype, generator=gen))
    mag_fm = mag.transpose(1, 2).contiguous()
    w = torch.randn((B, L), device=dev, dtype=dtype, generator=gen)
    with torch.no_grad():
        forward_ms = timed(lambda: si.gla_projection(x, mag_fm, frame_major=True, **kw), reps)
    res = {"forward_ms": round(forward_ms, 4)}
    grads = {}
    for path, knob in (("fused", "1"), ("staged", "0")):
        os.environ["SPECINV_PROJ_ADJ_FUSED"] = knob
        si.plan.clear_plan_cache()                                    # (the knob is read when a plan is created)
        plan = Plan(args, B, T, dtype, dev)
        assert plan.project_adjoint_kind == path, plan.project_adjoint_kind
        xs, ms = x.clone().requires_grad_(True), mag_fm.clone().requires_grad_(True)
        loss = (si.gla_projection(xs, ms, frame_major=True, **kw) * w).sum()
        res[f"backward_ms_{path}"] = round(timed(lambda: torch.autograd.grad(loss, (xs, ms), retain_graph=True), reps), 4)
        res[f"adjoint_call_ms_{path}"] = round(timed(lambda: plan.project_adjoint(x, mag_fm, w), reps), 4)
        grads[path] = plan.project_adjoint(x, mag_fm, w)
    del os.environ["SPECINV_PROJ_ADJ_FUSED"]
    si.plan.clear_plan_cache()
    res["staged_over_fused"] = round(res["adjoint_call_ms_staged"] / res["adjoint_call_ms_fused"], 3)
    res["grad_rel_l2_fused_vs_staged"] = [float((a - b).norm() / b.norm()) for a, b in zip(grads["fused"], grads["staged"])]
    size = torch.empty((), dtype=dtype).element_size()
    reals = 2 * hop + 2 * F + n_fft
    res["bytes_per_frame"] = {"fused": reals * size, "staged": (reals + 6 * 2 * F) * size}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "projection_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, T, n_fft, hop = 16, 512, 1024, 256
    res = {"config": dict(B=B, n_fft=n_fft, hop=hop, T=T, reps=a.reps)}
    for dtype in (torch.float32, torch.float64):
        res[str(dtype).split(".")[1]] = one_dtype(dtype, B, T, n_fft, hop, a.reps, dev)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
