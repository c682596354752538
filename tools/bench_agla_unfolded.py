#!/usr/bin/env python3
"""agla_unfolded, forward + backward, at B 16, n_fft 1024, hop 256, 512 frames, float32, 5 iterations, with a general schedule
(gamma != 1: three sequences) and in the Fast Griffin-Lim form (every gamma = 1): one JSON line, also written to
profiles/agla_unfolded_bench.json.

    python tools/bench_agla_unfolded.py [--reps N] [--out PATH]

per form:
forward_ms           the recorded forward pass (agla_init_sched, 5 x (wave, agla_iterate(1)), wave) on a warm plan
inference_ms         accelerated_griffin_lim(max_iter=5, tol=0) on the same inputs: what the recording costs is the difference
backward_ms          the backward sweep: 4 x specinv_agla_step_adjoint, specinv_agla_first_adjoint, istft_adjoint, phase_init_adjoint
blocks_backward_ms   the same sweep assembled from the blocks that were there before: the extrapolation's adjoint, the recomputation
                     of c_{n-1} and the three inner products in torch ops, istft_adjoint, gla_update_adjoint at lr = 0, stft_adjoint
step_kernel_ms       specinv_agla_extrap_adjoint alone (k_agla_step_adjoint + the finishing launch) and the bytes / s it achieves at
                     10 (general) or 8 (every gamma = 1) transfers of 4 bytes per sample
No gate: the figures go into DESIGN 3.14.
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


def blocks_backward(plan, t, sched, mag, g_y, env):
    """agla_unfolded's sweep from the adjoint blocks of autograd.py and torch ops; t[0] = c_0, t[n] = t_n.  Returns (cotangent of
    C0, gmag, the (n_iter, 3) parameter gradients)."""
    al, be, ga = sched
    n_iter, L = len(al), plan.length
    general = any(g != 1.0 for g in ga)
    a, gc, gd = g_y, torch.zeros_like(g_y), torch.zeros_like(g_y)
    gm = torch.zeros_like(mag)
    dots = torch.zeros((n_iter, 3), dtype=torch.float64, device=g_y.device)
    for n in range(n_iter, 1, -1):
        delta = t[n] - t[n - 1]
        s = a + (1 + al[n - 1]) * gc
        if general:
            s = s + (1 + be[n - 1]) * gd
        back = t[n - 1] - t[n - 2] if n > 2 else None
        c_prev = t[n - 1] + al[n - 2] * back if n > 2 else t[n - 1]
        d_prev = t[n - 1] + be[n - 2] * back if n > 2 else t[n - 1]
        dots[n - 1, 0] = (gc.double() * delta.double()).sum()
        if general:
            dots[n - 1, 1] = (gd.double() * delta.double()).sum()
        dots[n - 1, 2] = (s.double() * (t[n] - d_prev).double()).sum() / ga[n - 1]
        a = -al[n - 1] * gc
        if general:
            a = a - be[n - 1] * gd
            gd = (1 - ga[n - 1]) * s
        gq = plan.istft_adjoint(ga[n - 1] * s)
        gr, _ = plan.gla_update_adjoint(gq, None, plan.stft(c_prev), mag, 0.0, gm)
        gc = plan.stft_adjoint(gr, L)
    gq = plan.istft_adjoint(a + gc + gd)
    gr, _ = plan.gla_update_adjoint(gq, None, plan.stft(t[0]), mag, 0.0, gm)
    return plan.istft_adjoint(plan.stft_adjoint(gr, L)), gm, dots


def one_form(plan, mag, w, sched, kw, reps):
    dev = mag.device
    n_iter = len(sched[0])
    B, L = plan.batch, plan.length
    consts = dict(alpha=sched[0][0], beta=sched[1][0], gamma=sched[2][0])
    inference_ms = timed(lambda: si.accelerated_griffin_lim(mag, max_iter=n_iter, tol=0, verbose=False, **consts, **kw), reps)
    s = mag.clone().requires_grad_(True)
    par = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in sched]
    forward_ms = timed(lambda: si.agla_unfolded(s, n_iter, *par, **kw), reps)
    loss = (si.agla_unfolded(s, n_iter, *par, **kw) * w).sum()
    backward_ms = timed(lambda: torch.autograd.grad(loss, (s, *par), retain_graph=True), reps)
    geo = plan.launch_geometry

    # the same iterates, recorded by hand, through the blocks
    plan.agla_init_sched(None, mag, *sched)
    t = []
    for _ in range(n_iter):
        t.append(plan.wave())
        plan.agla_iterate(1)
    t.append(plan.wave())
    env = plan.envelope()
    blocks_ms = timed(lambda: blocks_backward(plan, t, sched, mag, w, env), reps)
    grads = torch.autograd.grad(loss, (s, *par))
    g_c0, gm, dots = blocks_backward(plan, t, sched, mag, w, env)
    plan.phase_init_adjoint(mag, g_c0.contiguous(), gm)
    agree = float((gm - grads[0]).norm() / grads[0].norm())
    agree_par = float((dots.cpu().T - torch.stack(grads[1:])).norm() / torch.stack(grads[1:]).norm())

    # the step kernel alone
    general = any(g != 1.0 for g in sched[2])
    a, gc, c_prev = w.clone(), torch.randn_like(w), torch.empty_like(w)
    gd = torch.randn_like(w) if general else None
    dots1 = torch.zeros(3, dtype=torch.float64, device=dev)
    coef = (sched[0][2], sched[1][2], sched[2][2], sched[0][1], sched[1][1])
    step_ms = timed(lambda: plan.agla_extrap_adjoint(t[3], t[2], t[1], coef, a, gc, gd, c_prev, dots1), reps)
    moved = (10 if general else 8) * B * L * 4
    return {
        "schedule": sched,
        "inference_ms": round(inference_ms, 4),
        "forward_ms": round(forward_ms, 4),
        "backward_ms": round(backward_ms, 4),
        "forward_backward_ms": round(forward_ms + backward_ms, 4),
        "blocks_backward_ms": round(blocks_ms, 4),
        "blocks_over_fused_backward": round(blocks_ms / backward_ms, 3),
        "grad_spec_rel_l2_fused_vs_blocks": agree,
        "grad_params_rel_l2_fused_vs_blocks": agree_par,
        "step_kernel_ms": round(step_ms, 4),
        "step_kernel_bytes": moved,
        "step_kernel_gb_per_s": round(moved / step_ms / 1e6, 1),
        "saved_bytes": (n_iter + 1) * B * L * 4,
        "saved_bytes_as_spectra": n_iter * B * (plan.n_freq * plan.n_frames) * 8,
        "kernel": geo,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "agla_unfolded_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, T, n_fft, hop, n_iter = 16, 512, 1024, 256, 5
    F = n_fft // 2 + 1
    kw = dict(hop_length=hop, window=torch.hann_window(n_fft))
    gen = torch.Generator(device=dev).manual_seed(0)
    mag = torch.rand((B, F, T), device=dev, generator=gen) + 0.05
    plan = get_plan(args_helper(mag, **kw), B, T, torch.float32, dev)
    w = torch.randn((B, plan.length), device=dev, generator=gen)
    forms = {"general": ([0.5] * n_iter, [1.2] * n_iter, [0.7] * n_iter), "fgla": ([0.99] * n_iter, [0.99] * n_iter, [1.0] * n_iter)}
    res = {"config": dict(B=B, n_fft=n_fft, hop=hop, T=T, L=plan.length, dtype="float32", n_iter=n_iter, reps=a.reps)}
    for name, sched in forms.items():
        res[name] = one_form(plan, mag, w, sched, kw, a.reps)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
