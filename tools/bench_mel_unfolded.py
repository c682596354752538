#!/usr/bin/env python3
"""mel_to_stft_unfolded, forward + backward, at B 16, 1024 frames, n_fft 2048, 80 bands, 100 iterations, float32 (the geometry of
tests/test_gpu_mel.py::test_bench_size_sample): one JSON line, also written to profiles/mel_unfolded_bench.json.

    python tools/bench_mel_unfolded.py [--reps N] [--out PATH]

forward_launch_ms    specinv_mel_nnls alone (k_mel_nnls) on a warm plan
adjoint_launch_ms    specinv_mel_nnls_adjoint alone (k_mel_nnls_adjoint: the iteration recomputed, then swept back)
forward_ms           mel_to_stft_unfolded under grad (the launch plus the layer's host work)
backward_ms          its backward pass
inference_ms         mel_to_stft on the same input
No gate: the figures go into DESIGN 3.15.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import spectrogram_inversion_amd as si
from spectrogram_inversion_amd import _lib
from spectrogram_inversion_amd.mel import mel_filterbank
from spectrogram_inversion_amd.plan import args_helper, get_plan


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mel_unfolded_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, T, n_fft, n_mels, n_iter = 16, 1024, 2048, 80, 100
    F = n_fft // 2 + 1
    M = mel_filterbank(22050, n_fft, n_mels)
    gen = torch.Generator(device=dev).manual_seed(0)
    mag = torch.rand((B, F, T), device=dev, generator=gen) ** 2
    mel = torch.from_numpy(M).to(dev) @ mag
    w = torch.randn((B, F, T), device=dev, generator=gen)

    inference_ms = timed(lambda: si.mel_to_stft(mel, M, n_iter=n_iter), a.reps)
    y = mel.clone().requires_grad_(True)
    forward_ms = timed(lambda: si.mel_to_stft_unfolded(y, M, n_iter=n_iter), a.reps)
    out = si.mel_to_stft_unfolded(y, M, n_iter=n_iter)
    backward_ms = timed(lambda: torch.autograd.grad(out, y, w, retain_graph=True), a.reps)
    grad = torch.autograd.grad(out, y, w)[0]

    # the two launches alone, on the plan the calls above left set up
    plan = get_plan(args_helper(torch.empty(1, F, 1)), B, T, torch.float32, dev)
    plan._sync_stream()
    o, gm = torch.empty_like(mag), torch.empty_like(mel)
    fwd = lambda: _lib.check(plan.lib.specinv_mel_nnls(plan._h, mel.data_ptr(), n_iter, 1.0, o.data_ptr()))                      # noqa: E731
    adj = lambda: _lib.check(plan.lib.specinv_mel_nnls_adjoint(plan._h, mel.data_ptr(), n_iter, 1.0, w.data_ptr(), gm.data_ptr()))  # noqa: E731
    forward_launch_ms = timed(fwd, a.reps)
    adjoint_launch_ms = timed(adj, a.reps)
    most = C.c_int()
    _lib.check(plan.lib.specinv_mel_nnls_adjoint_max_iter(plan._h, C.byref(most)))
    res = {
        "bench": "mel_unfolded",
        "device": torch.cuda.get_device_name(0),
        "shape": {"B": B, "T": T, "n_fft": n_fft, "n_mels": n_mels, "n_iter": n_iter, "dtype": "float32"},
        "reps": a.reps,
        "forward_launch_ms": round(forward_launch_ms, 4),
        "adjoint_launch_ms": round(adjoint_launch_ms, 4),
        "adjoint_over_forward": round(adjoint_launch_ms / forward_launch_ms, 3),
        "inference_ms": round(inference_ms, 4),
        "forward_ms": round(forward_ms, 4),
        "backward_ms": round(backward_ms, 4),
        "frame_iterations_per_s_forward": round(B * T * n_iter / forward_launch_ms * 1e3),
        "frame_iterations_per_s_adjoint": round(B * T * n_iter / adjoint_launch_ms * 1e3),
        "adjoint_max_iter": most.value,
        "launch_equals_layer": bool(torch.equal(gm, grad)),
        "saved_bytes": mel.numel() * 4,
    }
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
