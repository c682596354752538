#!/usr/bin/env python3
"""pyin (k_pyin_obs, k_pyin_viterbi) at B 16, L 163 584 at 16 kHz, frames of 2048 every 512 and of 1024 every 256,
fmin 65, fmax 2093, defaults otherwise, against the decode written as torch ops on the same GPU in the same run.  One JSON line,
also written to profiles/pyin_bench.json.

    python tools/bench_pyin.py [--window MS] [--repeats M] [--out PATH]

per shape:
yin_cmnd_ms           launch 1, specinv_yin writing d' (B, T, W + 1), on preallocated outputs: events around as many calls as fill
                      `window` ms, the median of `repeats` such windows (tools/bench_yin.py's `timed`)
obs_ms                launch 2, specinv_pyin_obs
viterbi_ms            launch 3, specinv_pyin_viterbi, the walk back included
call_ms               si.pyin, the public function (argument checks, allocation of d', observations, pointers and outputs, f0)
decode_us_per_frame   viterbi_ms / T: an item is one workgroup, so the B items run side by side
ticks                 from the kernel's own 100 MHz wall clock (the variant with ticks_out), the median over the items: microseconds
                      per frame of the forward pass, microseconds per frame of the walk back, and the walk's share of the item
torch_decode_ms       the same model as torch ops: log(A + tiny) as a dense (2P, 2P) float64 matrix, per frame one (B, 2P, 2P) add
                      and one max over the predecessors, then the walk back as T gathers - fed the kernel's observations.  The
                      observation stage has no torch form here: a whole pyin in torch ops costs at least this.
agreement             of the two decodes: frames whose voiced flag differs, voiced frames whose state differs, and the largest
                      relative difference of the two paths' scores under the dense model (unvoiced bins tie and are not compared)
The only requirement fixed in advance is call_ms <= torch_decode_ms; the tool writes down what comes out and exits 1 otherwise.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch

import spectrogram_inversion_amd as si
from bench_yin import timed, voice
from spectrogram_inversion_amd import _lib, pitch

TINY = 2.2250738585072014e-308


def dense_model(n_bins, half, switch, dev):
    """(log A (2P, 2P), log init (2P,)) in float64"""
    j = torch.arange(n_bins, device=dev)
    k = (j[None] - j[:, None]).abs()
    tri = torch.where(k <= half, 1.0 - k.double() / (half + 1.0), torch.zeros((), dtype=torch.float64, device=dev))
    a = tri / tri.sum(-1, keepdim=True)
    sw = torch.tensor([[1.0 - switch, switch], [switch, 1.0 - switch]], dtype=torch.float64, device=dev)
    init = torch.cat([torch.zeros(n_bins, dtype=torch.float64, device=dev),
                      torch.full((n_bins,), 1.0 / n_bins, dtype=torch.float64, device=dev)])
    return torch.log(torch.kron(sw, a) + TINY), torch.log(init + TINY)


def log_emission(obs, vprob):
    n_bins = obs.shape[-1]
    unv = ((1.0 - vprob.double()) / n_bins)[..., None].expand(-1, -1, n_bins)
    return torch.log(torch.cat([obs.double(), unv], -1) + TINY)


def viterbi_torch(obs, vprob, log_a, log_init):
    """int64 states (B, T): the dense log-space decode, one (B, 2P, 2P) add and max per frame"""
    log_b = log_emission(obs, vprob)
    batch, n_frames, n_states = log_b.shape
    delta = log_init + log_b[:, 0]
    ptr = torch.empty((batch, n_frames, n_states), dtype=torch.int64, device=obs.device)
    for t in range(1, n_frames):
        best, ptr[:, t] = (delta[:, :, None] + log_a).max(dim=1)
        delta = best + log_b[:, t]
    states = torch.empty((batch, n_frames), dtype=torch.int64, device=obs.device)
    states[:, -1] = delta.argmax(-1)
    for t in range(n_frames - 1, 0, -1):
        states[:, t - 1] = ptr[:, t].gather(-1, states[:, t:t + 1]).squeeze(-1)
    return states


def path_scores(states, obs, vprob, log_a, log_init):
    log_b = log_emission(obs, vprob)
    s = states.long()
    return (log_init[s[:, 0]] + log_b.gather(-1, s[..., None]).squeeze(-1).sum(-1) + log_a[s[:, :-1], s[:, 1:]].sum(-1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=200.0, help="ms of work per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pyin_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, L, sr, fmin, fmax, switch = 16, 163584, 16000, 65.0, 2093.0, 0.01
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev)
    sp = C.c_void_p(stream.cuda_stream)
    n_bins, bps = si.pyin_bins(fmin, fmax), 10
    res = {"tool": "tools/bench_pyin.py", "device": torch.cuda.get_device_name(0), "library": os.path.basename(_lib.LIB_PATH),
           "config": dict(B=B, L=L, sample_rate=sr, fmin=fmin, fmax=fmax, P=n_bins, n_thresholds=100, resolution=0.1,
                          window_ms=a.window, repeats=a.repeats), "shapes": {}}
    x = voice(B, L, sr, dev)
    x[B - 1] = 0.3 * torch.randn(L, device=dev, generator=torch.Generator(device=dev).manual_seed(1))      # one unvoiced item
    x[B - 2, L // 3:L // 2] = 0                                                                             # and one with a pause
    ok = True
    for n, hop in ((2048, 512), (1024, 256)):
        tau_min, tau_max = pitch._lag_range(sr, fmin, fmax, n)
        half = pitch._transition_half(sr, hop, bps, 35.92)
        t = si.yin_frames(L, n, hop)
        n_ranks = (tau_max - tau_min) // 2 + 1
        period, aper = torch.empty((B, t), device=dev), torch.empty((B, t), device=dev)
        cmnd = torch.empty((B, t, n // 2 + 1), device=dev)
        obs, vprob = torch.empty((B, t, n_bins), device=dev), torch.empty((B, t), device=dev)
        backptr = torch.empty((B, t, 2 * n_bins), dtype=torch.int16, device=dev)
        states = torch.empty((B, t), dtype=torch.int32, device=dev)
        ticks = torch.zeros((B, 3), dtype=torch.int64, device=dev)
        tab_obs = pitch._obs_tables(pitch._integer_prior(100, 2, 18), 2.0, n_ranks, dev)
        tab_dec = pitch._decode_tables(n_bins, half, dev)

        def launch_yin():
            _lib.check(lib.specinv_yin(x.data_ptr(), period.data_ptr(), aper.data_ptr(), None, cmnd.data_ptr(), B, L, n, hop, 1, 1,
                                       n // 2 - 1, 0.1, _lib.F32, 0, sp))

        def launch_obs():
            _lib.check(lib.specinv_pyin_obs(cmnd.data_ptr(), tab_obs.data_ptr(), obs.data_ptr(), vprob.data_ptr(), B * t, n, tau_min,
                                            tau_max, 100, n_ranks, n_bins, bps, float(sr), fmin, 0.01, _lib.F32, 0, sp))

        def launch_vit(with_ticks=False):
            _lib.check(lib.specinv_pyin_viterbi(obs.data_ptr(), vprob.data_ptr(), tab_dec.data_ptr(), backptr.data_ptr(),
                                                states.data_ptr(), ticks.data_ptr() if with_ticks else None, B, t, n_bins, half,
                                                switch, _lib.F32, 0, sp))

        launch_yin()
        launch_obs()
        log_a, log_init = dense_model(n_bins, half, switch, dev)
        r = {"T": t, "tau_min": tau_min, "tau_max": tau_max, "half_width": half,
             "yin_cmnd_ms": timed(launch_yin, a.window, a.repeats),
             "obs_ms": timed(launch_obs, a.window, a.repeats),
             "viterbi_ms": timed(launch_vit, a.window, a.repeats),
             "call_ms": timed(lambda: si.pyin(x, sr, fmin, fmax, n, hop), a.window, a.repeats),
             "torch_decode_ms": timed(lambda: viterbi_torch(obs, vprob, log_a, log_init), a.window, max(3, a.repeats // 2))}
        r["launches_ms"] = r["yin_cmnd_ms"] + r["obs_ms"] + r["viterbi_ms"]
        r["decode_us_per_frame"] = r["viterbi_ms"] * 1e3 / t
        r["torch_over_call"] = r["torch_decode_ms"] / r["call_ms"]
        r["torch_over_viterbi"] = r["torch_decode_ms"] / r["viterbi_ms"]
        launch_vit(True)
        torch.cuda.synchronize()
        tk = ticks.double().cpu()
        fwd, walk = (tk[:, 1] - tk[:, 0]) / 100.0, (tk[:, 2] - tk[:, 1]) / 100.0                  # microseconds at 100 MHz
        r["ticks"] = {"forward_us_per_frame": statistics.median((fwd / t).tolist()),
                      "walk_us_per_frame": statistics.median((walk / t).tolist()),
                      "walk_share": statistics.median((walk / (fwd + walk)).tolist())}
        want = viterbi_torch(obs, vprob, log_a, log_init)
        got = states.long()
        voiced = want < n_bins
        s_got, s_want = path_scores(got, obs, vprob, log_a, log_init), path_scores(want, obs, vprob, log_a, log_init)
        f0, flag, prob = si.pyin(x, sr, fmin, fmax, n, hop)
        r["voiced_share"] = float(flag.double().mean())
        r["agreement"] = {"flags_that_differ": int(((got < n_bins) != voiced).sum()),
                          "voiced_states_that_differ": int((got[voiced] != want[voiced]).sum()), "of": B * t,
                          "score_max_rel_diff": float(((s_got - s_want) / s_want).abs().max())}
        ok = ok and r["call_ms"] <= r["torch_decode_ms"]
        res["shapes"][f"{n} / {hop}"] = {k: (round(v, 5) if isinstance(v, float) else v) for k, v in r.items()}
    res["pyin_not_slower_than_torch_decode"] = ok
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
