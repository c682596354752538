#!/usr/bin/env python3
"""misi_unfolded, forward + backward, at B 16 mixtures of K 2 sources, n_fft 1024, hop 256, 512 frames, float32, 5 iterations:
one JSON line, also written to profiles/misi_unfolded_bench.json.

    python tools/bench_misi_unfolded.py [--reps N] [--out PATH]

forward_ms           the recorded forward pass (misi_init, 5 x (wave, misi_iterate(1)), wave) on a warm plan
inference_ms         misi(max_iter=5, tol=0) on the same inputs: what the recording costs is the difference
backward_ms          the backward sweep: 5 x specinv_misi_step_adjoint, the coupling adjoint, istft_adjoint, the chain to the inputs
blocks_backward_ms   the same sweep assembled from the blocks that were there before: istft_adjoint, gla_update_adjoint at lr = 0,
                     stft_adjoint, the coupling adjoint and the envelope's place in torch ops, on recorded signals (the spectrum is
                     recomputed with plan.stft, so both sweeps do the same transforms)
saved_bytes          what the graph holds between forward and backward: 5 signals of B K L reals (recorded spectra: B K F T complex)
No gate: the figures go into DESIGN 3.13.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import spectrogram_inversion_amd as si
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


def blocks_backward(plan, K, waves, mag, g_y):
    """The sweep of misi_unfolded's backward from the adjoint blocks of autograd.py; returns (g of x_0's pre-coupling signal as
    the cotangent of C0, gmag, gmix)."""
    n_mix, L = plan.batch // K, plan.length
    g = g_y
    gmix = torch.zeros((n_mix, L), dtype=g.dtype, device=g.device)
    gm = torch.zeros_like(mag)
    for x_prev in reversed(waves):
        c = g.reshape(n_mix, K, L).mean(1)
        gmix += c
        gq = plan.istft_adjoint((g.reshape(n_mix, K, L) - c[:, None]).reshape(plan.batch, L))
        gr, _ = plan.gla_update_adjoint(gq, None, plan.stft(x_prev), mag, 0.0, gm)
        g = plan.stft_adjoint(gr, L)
    c = g.reshape(n_mix, K, L).mean(1)
    gmix += c
    return plan.istft_adjoint((g.reshape(n_mix, K, L) - c[:, None]).reshape(plan.batch, L)), gm, gmix


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "misi_unfolded_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, K, T, n_fft, hop, n_iter = 16, 2, 512, 1024, 256, 5
    F = n_fft // 2 + 1
    kw = dict(hop_length=hop, window=torch.hann_window(n_fft))
    gen = torch.Generator(device=dev).manual_seed(0)
    mag = torch.rand((B, K, F, T), device=dev, generator=gen) + 0.05
    plan = get_plan(args_helper(mag.reshape(B * K, F, T), **kw), B * K, T, torch.float32, dev)
    L = plan.length
    mix = 0.1 * torch.randn((B, L), device=dev, generator=gen)
    w = torch.randn((B, K, L), device=dev, generator=gen)

    inference_ms = timed(lambda: si.misi(mag, mix, max_iter=n_iter, tol=0, verbose=False, **kw), a.reps)
    s, m = mag.clone().requires_grad_(True), mix.clone().requires_grad_(True)
    forward_ms = timed(lambda: si.misi_unfolded(s, m, n_iter, **kw), a.reps)
    loss = (si.misi_unfolded(s, m, n_iter, **kw) * w).sum()
    backward_ms = timed(lambda: torch.autograd.grad(loss, (s, m), retain_graph=True), a.reps)
    geo = plan.launch_geometry

    # the same iterates, recorded by hand, through the blocks
    start = torch.polar(mag.reshape(B * K, F, T), torch.angle(plan.stft(mix.repeat_interleave(K, dim=0))))
    plan.misi_init(start, mag.reshape(B * K, F, T), mix, K)
    waves = []
    for _ in range(n_iter):
        waves.append(plan.wave())
        plan.misi_iterate(1)
    mag3, g_y = mag.reshape(B * K, F, T).contiguous(), w.reshape(B * K, L).contiguous()
    blocks_ms = timed(lambda: blocks_backward(plan, K, waves, mag3, g_y), a.reps)
    # (the two sweeps agree: the fused one is checked against the blocks in tests/test_gpu_misi_unfolded.py)
    gs, gmx = torch.autograd.grad(loss, (s, m))
    gc, gm, gmix = blocks_backward(plan, K, waves, mag3, g_y)
    u = start / mag3
    agree = float(((gm + (gc.real * u.real + gc.imag * u.imag)).reshape(B, K, F, T) - gs).norm() / gs.norm())

    res = {
        "config": dict(B=B, K=K, n_fft=n_fft, hop=hop, T=T, L=L, dtype="float32", n_iter=n_iter, reps=a.reps),
        "inference_ms": round(inference_ms, 4),
        "forward_ms": round(forward_ms, 4),
        "backward_ms": round(backward_ms, 4),
        "forward_backward_ms": round(forward_ms + backward_ms, 4),
        "blocks_backward_ms": round(blocks_ms, 4),
        "blocks_over_fused_backward": round(blocks_ms / backward_ms, 3),
        "grad_specs_rel_l2_fused_vs_blocks": agree,
        "saved_bytes": n_iter * B * K * L * 4,
        "saved_bytes_as_spectra": n_iter * B * K * F * T * 8,
        "kernel": geo,
    }
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
