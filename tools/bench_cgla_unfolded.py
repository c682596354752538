#!/usr/bin/env python3
"""constrained_unfolded, forward + backward, at B 16, n_fft 1024, hop 256, 512 frames, float32, 5 iterations, known bins and known
samples both, a complex start, with a general schedule (gamma != 1: three sequences) and in the Fast Griffin-Lim form (every
gamma = 1): one JSON line, also written to profiles/cgla_unfolded_bench.json.

    python tools/bench_cgla_unfolded.py [--reps N] [--out PATH]

per form:
forward_ms            the recorded forward pass (_begin, 5 x (wave, agla_iterate(1)), wave) on a warm plan
inference_ms          constrained_griffin_lim(max_iter=5, tol=0) on the same inputs: what the recording costs is the difference
backward_ms           the backward sweep: 4 x specinv_cgla_step_adjoint, specinv_cgla_first_adjoint, two istft_adjoint and the
                      split of the cotangents between spec, known_spec and known_wave in torch ops
composed_*_ms         the baseline: the same layer composed from si.gla_projection, si.istft, torch.where and element-wise torch
                      ops under autograd on the device, forward and backward
step_kernel_ms        specinv_cgla_extrap_adjoint alone (k_agla_step_adjoint + the finishing launch) and the bytes / s it achieves at
                      12 (general) or 10 (every gamma = 1) transfers of 4 bytes plus one mask byte per sample
No gate: the figures go into DESIGN 3.18.
"""
import argparse
import json
import math
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


def composed(s, K, M, xk, W, par, kw):
    """The layer from the library's layers and torch ops: what a user writes without constrained_unfolded"""
    al, be, ga = par
    n_iter = al.numel()
    m_free = torch.where(M, torch.zeros_like(s.real), s.abs())
    c = si.istft(torch.where(M, K, s), **kw)
    k = si.istft(torch.where(M, K, torch.zeros_like(K)), **kw)
    t = d = None
    for n in range(1, n_iter + 1):
        u = si.gla_projection(c, m_free, **kw) + k
        if n == 1:
            t = c = d = torch.where(W, xk, u)
        else:
            tn = torch.where(W, xk, (1.0 - ga[n - 1]) * d + ga[n - 1] * u)
            c = tn + al[n - 1] * (tn - t)
            d = tn + be[n - 1] * (tn - t)
            t = tn
    return t


def one_form(plan, case, sched, kw, reps):
    spec, K, M, xk, W, w = case
    dev = spec.device
    n_iter = len(sched[0])
    B, L = plan.batch, plan.length
    consts = dict(alpha=sched[0][0], beta=sched[1][0], gamma=sched[2][0])
    inference_ms = timed(lambda: si.constrained_griffin_lim(spec, K, M, xk, W, max_iter=n_iter, tol=0, verbose=False, **consts, **kw),
                         reps)
    leaves = [t.clone().requires_grad_(True) for t in (spec, K, xk)]
    par = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in sched]

    def layer():
        return si.constrained_unfolded(leaves[0], leaves[1], M, leaves[2], W, n_iter, *par, **kw)

    forward_ms = timed(layer, reps)
    loss = (layer() * w).sum()
    backward_ms = timed(lambda: torch.autograd.grad(loss, (*leaves, *par), retain_graph=True), reps)
    grads = torch.autograd.grad(loss, (*leaves, *par))

    # the baseline: parameters as float32 device tensors, so that no element-wise op is promoted or crosses to the host
    dpar = [torch.tensor(v, dtype=torch.float32, device=dev, requires_grad=True) for v in sched]

    def base():
        return composed(leaves[0], leaves[1], M, leaves[2], W, dpar, kw)

    composed_forward_ms = timed(base, reps)
    bloss = (base() * w).sum()
    composed_backward_ms = timed(lambda: torch.autograd.grad(bloss, (*leaves, *dpar), retain_graph=True), reps)
    bgrads = torch.autograd.grad(bloss, (*leaves, *dpar))
    agree = {name: float((g - b).norm() / b.norm())
             for name, g, b in zip(("spec", "known_spec", "known_wave"), grads[:3], bgrads[:3])}
    gp, bp = torch.stack(grads[3:])[:, 1:], torch.stack([b.double().cpu() for b in bgrads[3:]])[:, 1:]
    agree["params"] = float((gp - bp).norm() / bp.norm())

    # the step kernel alone
    general = any(g != 1.0 for g in sched[2])
    t = [torch.randn_like(w) for _ in range(3)]
    a, gc, goff, c_prev = w.clone(), torch.randn_like(w), torch.zeros_like(w), torch.empty_like(w)
    gd = torch.randn_like(w) if general else None
    dots1 = torch.zeros(3, dtype=torch.float64, device=dev)
    coef = (sched[0][2], sched[1][2], sched[2][2], sched[0][1], sched[1][1])
    w8 = W.to(torch.uint8)
    step_ms = timed(lambda: plan.cgla_extrap_adjoint(t[0], t[1], t[2], coef, w8, a, gc, gd, goff, c_prev, dots1), reps)
    moved = ((12 if general else 10) * 4 + 1) * B * L
    fused, base_ms = forward_ms + backward_ms, composed_forward_ms + composed_backward_ms
    return {
        "schedule": sched,
        "inference_ms": round(inference_ms, 4),
        "forward_ms": round(forward_ms, 4),
        "backward_ms": round(backward_ms, 4),
        "forward_backward_ms": round(fused, 4),
        "composed_forward_ms": round(composed_forward_ms, 4),
        "composed_backward_ms": round(composed_backward_ms, 4),
        "composed_forward_backward_ms": round(base_ms, 4),
        "composed_over_layer": round(base_ms / fused, 3),
        "grad_rel_l2_layer_vs_composed": agree,
        "step_kernel_ms": round(step_ms, 4),
        "step_kernel_bytes": moved,
        "step_kernel_gb_per_s": round(moved / step_ms / 1e6, 1),
        "saved_bytes": (n_iter + 1) * B * L * 4,
        "kernel": plan.launch_geometry,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cgla_unfolded_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, T, n_fft, hop, n_iter = 16, 512, 1024, 256, 5
    F = n_fft // 2 + 1
    kw = dict(hop_length=hop, window=torch.hann_window(n_fft))
    gen = torch.Generator(device=dev).manual_seed(0)
    spec = torch.polar(torch.rand((B, F, T), device=dev, generator=gen) + 0.05,
                       (torch.rand((B, F, T), device=dev, generator=gen) * 2 - 1) * math.pi)
    plan = get_plan(args_helper(spec, **kw), B, T, torch.float32, dev)
    L = plan.length
    w = torch.randn((B, L), device=dev, generator=gen)
    # bandwidth extension and a gap: the bins below F / 4 and the first third of the samples are known, those of a noise signal
    xk = torch.randn((B, L), device=dev, generator=gen) * 0.05
    K = si.stft(xk, n_fft, **kw)
    M = torch.zeros((B, F, T), dtype=torch.bool, device=dev)
    M[:, : F // 4] = True
    W = torch.zeros((B, L), dtype=torch.bool, device=dev)
    W[:, : L // 3] = True
    forms = {"general": ([0.5] * n_iter, [1.2] * n_iter, [0.7] * n_iter), "fgla": ([0.99] * n_iter, [0.99] * n_iter, [1.0] * n_iter)}
    res = {"config": dict(B=B, n_fft=n_fft, hop=hop, T=T, L=L, dtype="float32", n_iter=n_iter, reps=a.reps,
                          known_bins=float(M.float().mean()), known_samples=float(W.float().mean()))}
    for name, sched in forms.items():
        res[name] = one_form(plan, (spec, K, M, xk, W, w), sched, kw, a.reps)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
