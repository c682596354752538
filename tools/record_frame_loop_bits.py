#!/usr/bin/env python3
"""Records what the signal-form Griffin-Lim kernels (kernels_fast_td.h) compute, for tests/test_gpu_frame_loop_bits.py.

    python tools/record_frame_loop_bits.py <commit the library was built from> [out.npz]

Run it ONCE, on the build whose bits are to be kept (the parent of a change that must not move them), on an MI355X.  Per case of
CASES the fixture holds the SHA-256 of the float32 waveform and of the evaluation rows (iteration, metric, loss as float64), the
first 64 samples of item 0, the frame count the case ran at and the launch geometry; `meta` names the commit.  The test imports
CASES and run_case from here, so that both sides run the same inputs; it never regenerates the fixture.

A case needs the `_td` kernel and at least two chunks per item (chunk seams are crossed): the recorder raises the frame count by 8
until the plan says so and stores the count it ended at."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "frame_loop_bits.npz")
ITERATIONS, EVA_ITER, BATCH = 24, 5, 3

# name: n_fft, hop, frames, alpha, pad_mode, SPECINV_CU_BUDGET (None: not set), seed
CASES = {
    "2048_512": (2048, 512, 40, 0.3, "reflect", None, 11),
    "2048_512_alpha0": (2048, 512, 40, 0.0, "reflect", None, 12),
    "1024_256": (1024, 256, 40, 0.3, "reflect", None, 13),
    "2048_1024": (2048, 1024, 40, 0.3, "reflect", None, 14),
    "2048_256": (2048, 256, 40, 0.3, "reflect", None, 15),
    "512_128": (512, 128, 40, 0.3, "reflect", None, 16),
    "2048_512_constant": (2048, 512, 40, 0.3, "constant", None, 17),
    "2048_512_replicate": (2048, 512, 40, 0.3, "replicate", None, 18),
    "2048_512_circular": (2048, 512, 40, 0.3, "circular", None, 19),
    # a chip of one compute unit: 2 chunks of 24 frames where the whole chip gets 6 of 8
    "2048_512_cu_budget": (2048, 512, 48, 0.3, "reflect", 255, 20),
}


def hann(n):
    return (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n) / n)).astype(np.float32)


def make_plan(n_fft, hop, frames, pad_mode, budget, device):
    from spectrogram_inversion_amd.plan import Plan, args_helper
    a = args_helper(torch.empty(1, n_fft // 2 + 1, 1), hop_length=hop, window=torch.from_numpy(hann(n_fft)), pad_mode=pad_mode)
    # small problems normally go to the one-frame-per-wave kernel: SPECINV_SMALL_FRAMES=0 puts them on the chunk-walking ones
    env = {"SPECINV_SMALL_FRAMES": "0", "SPECINV_CU_BUDGET": None if budget is None else str(budget)}
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        return Plan(a, BATCH, frames, torch.float32, device)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def run_case(name, frames=None, keep_state=False, device=None):
    """-> (waveform (B, L) float32, evaluation rows (n, 3) float64, launch geometry) of case `name` at `frames` frames"""
    n_fft, hop, frames0, alpha, pad_mode, budget, seed = CASES[name]
    frames = frames0 if frames is None else int(frames)
    device = torch.device("cuda", 0) if device is None else device
    mag = np.random.default_rng(seed).random((BATCH, n_fft // 2 + 1, frames), dtype=np.float32)
    p = make_plan(n_fft, hop, frames, pad_mode, budget, device)
    p.keep_state(keep_state)
    p.gla_init(None, torch.from_numpy(mag).to(device), alpha)
    geo = p.launch_geometry
    done, evals = p.run(ITERATIONS, EVA_ITER, 0.0, "sc")
    assert done == ITERATIONS and len(evals) == ITERATIONS // EVA_ITER, (done, evals)
    wave = p.wave().cpu().numpy()
    return np.ascontiguousarray(wave), np.array(evals, dtype=np.float64).reshape(-1, 3), geo


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def seams_crossed(geo):
    return geo["kernel"].endswith("_td") and geo["chunks"] >= 2


def main():
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    rec = {}
    cases = {}
    for name, (n_fft, hop, frames, alpha, pad_mode, budget, seed) in CASES.items():
        while True:
            wave, evals, geo = run_case(name, frames)
            if seams_crossed(geo):
                break
            frames += 8
            assert frames <= 200, (name, geo)
        assert np.isfinite(wave).all() and np.isfinite(evals).all(), name
        again, evals2, _ = run_case(name, frames)           # (the recorded bits are the build's, not one run's)
        assert np.array_equal(wave, again) and np.array_equal(evals, evals2), name
        if budget is not None:
            plain = make_plan(n_fft, hop, frames, pad_mode, None, torch.device("cuda", 0))
            plain.gla_init(None, torch.zeros(BATCH, n_fft // 2 + 1, frames, device="cuda") + 1.0, alpha)
            assert plain.launch_geometry["chunks"] != geo["chunks"], (name, geo, plain.launch_geometry)
        equals_spectral = False
        if alpha == 0.0:
            # no momentum: the signal-form kernel and the one that iterates on the spectrum compute the same waveform
            spectral, _, sgeo = run_case(name, frames, keep_state=True)
            assert not sgeo["kernel"].endswith("_td"), sgeo
            equals_spectral = bool(np.array_equal(wave, spectral))
        cases[name] = {"frames": frames, "kernel": geo["kernel"], "chunks": geo["chunks"], "waves": geo["waves"],
                       "wave_sha256": digest(wave), "evals_sha256": digest(evals), "equals_spectral_kernel": equals_spectral}
        rec[name + "__head"] = wave[0, :64].copy()
        rec[name + "__evals"] = evals
        print(name, cases[name], flush=True)
    meta = {"commit": commit, "iterations": ITERATIONS, "eva_iter": EVA_ITER, "batch": BATCH, "cases": cases}
    rec["meta"] = np.array(json.dumps(meta, sort_keys=True))
    os.makedirs(os.path.dirname(out), exist_ok=True)
    np.savez(out, **rec)
    print("wrote", out)


if __name__ == "__main__":
    main()
