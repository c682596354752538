#!/usr/bin/env python3
"""Records what a Griffin-Lim run computes around its frame loop, for tests/test_gpu_step_fixed_costs.py: the waveform right after
`gla_init` (the fused initial ISTFT, k_fused_istft), the waveform after 24 iterations and the evaluation rows.

    python tools/record_step_fixed_costs.py <commit the library was built from> [out.json]

Run it ONCE, on the build whose bits are to be kept, on an MI355X.  The entries take their inputs from the cases of
tools/record_frame_loop_bits.py (same seeds, same plans) and add the shapes its fixture lacks:

  * every `2048_512*` case, `1024_256` and `2048_1024` (another overlap) at the frame counts of tests/golden/frame_loop_bits.npz;
  * `2048_512@chunks_of_4`: 16 frames in chunks of exactly NB + 1 = 4 (SPECINV_FAST_CHUNK=4), the shortest a chunk can be: the
    initial ISTFT requests every frame one frame ahead and must ask for nothing past a chunk's last one.  Only the initial waveform
    is recorded (the iteration kernels ask for longer chunks);
  * `2048_512@one_item` and `1024_256@one_item`: a batch of one, whose waves do not fill the last workgroup - the waves that return
    early must still have passed the workgroup's barrier.

The test imports ENTRIES and run_entry from here; it never regenerates the fixture."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import record_frame_loop_bits as rec          # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "step_fixed_costs.json")
ITERATIONS, EVA_ITER = rec.ITERATIONS, rec.EVA_ITER

# name: case of record_frame_loop_bits.CASES, batch, frames (None: the frame-loop fixture's), SPECINV_FAST_CHUNK (None: not set),
# iterate after the initial waveform?
ENTRIES = {
    "2048_512": ("2048_512", 3, None, None, True),
    "2048_512_alpha0": ("2048_512_alpha0", 3, None, None, True),
    "2048_512_constant": ("2048_512_constant", 3, None, None, True),
    "2048_512_replicate": ("2048_512_replicate", 3, None, None, True),
    "2048_512_circular": ("2048_512_circular", 3, None, None, True),
    "2048_512_cu_budget": ("2048_512_cu_budget", 3, None, None, True),
    "1024_256": ("1024_256", 3, None, None, True),
    "2048_1024": ("2048_1024", 3, None, None, True),
    "2048_512@chunks_of_4": ("2048_512", 3, 16, 4, False),
    "2048_512@one_item": ("2048_512", 1, 44, None, True),
    "1024_256@one_item": ("1024_256", 1, 44, None, True),
}


def frames_of(name):
    case, _, frames, _, _ = ENTRIES[name]
    if frames is not None:
        return frames
    meta = json.loads(str(np.load(rec.FIXTURE, allow_pickle=False)["meta"]))
    return int(meta["cases"][case]["frames"])


def make_plan(name, batch=None, device=None):
    """-> (plan, magnitudes (batch, F, frames) on the device, alpha) of entry `name` (batch: another batch size, same seed)"""
    from spectrogram_inversion_amd.plan import Plan, args_helper
    case, batch0, _, fast_chunk, _ = ENTRIES[name]
    n_fft, hop, _, alpha, pad_mode, budget, seed = rec.CASES[case]
    batch = batch0 if batch is None else int(batch)
    frames = frames_of(name)
    device = torch.device("cuda", 0) if device is None else device
    a = args_helper(torch.empty(1, n_fft // 2 + 1, 1), hop_length=hop, window=torch.from_numpy(rec.hann(n_fft)), pad_mode=pad_mode)
    env = {"SPECINV_SMALL_FRAMES": "0", "SPECINV_CU_BUDGET": None if budget is None else str(budget),
           "SPECINV_FAST_CHUNK": None if fast_chunk is None else str(fast_chunk)}
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        plan = Plan(a, batch, frames, torch.float32, device)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    mag = np.random.default_rng(seed).random((batch, n_fft // 2 + 1, frames), dtype=np.float32)
    return plan, torch.from_numpy(mag).to(device), alpha


def run_entry(name):
    """-> (initial waveform, waveform after the iterations or None, evaluation rows (n, 3) float64 or None, launch geometry)"""
    p, mag, alpha = make_plan(name)
    p.gla_init(None, mag, alpha)
    geo = p.launch_geometry
    wave0 = np.ascontiguousarray(p.wave().cpu().numpy())
    if not ENTRIES[name][4]:
        return wave0, None, None, geo
    done, evals = p.run(ITERATIONS, EVA_ITER, 0.0, "sc")
    assert done == ITERATIONS and len(evals) == ITERATIONS // EVA_ITER, (done, evals)
    wave = np.ascontiguousarray(p.wave().cpu().numpy())
    return wave0, wave, np.array(evals, dtype=np.float64).reshape(-1, 3), geo


def main():
    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
    entries = {}
    for name in ENTRIES:
        wave0, wave, evals, geo = run_entry(name)
        again0, again, evals2, _ = run_entry(name)          # (the recorded bits are the build's, not one run's)
        assert np.isfinite(wave0).all() and np.array_equal(wave0, again0), name
        assert geo["chunks"] >= 2 and geo["kernel"].endswith("_td"), (name, geo)
        e = {"frames": frames_of(name), "batch": int(wave0.shape[0]), "kernel": geo["kernel"], "chunks": geo["chunks"],
             "waves": geo["waves"], "waves_per_workgroup": geo["waves_per_workgroup"], "initial_wave_sha256": rec.digest(wave0)}
        if wave is not None:
            assert np.isfinite(wave).all() and np.array_equal(wave, again) and np.array_equal(evals, evals2), name
            e["wave_sha256"] = rec.digest(wave)
            e["evals_sha256"] = rec.digest(evals)
        if name.endswith("@one_item"):
            assert geo["waves"] % geo["waves_per_workgroup"] != 0, (name, geo)
        if name.endswith("@chunks_of_4"):
            assert e["frames"] == 4 * geo["chunks"], (name, geo)
        entries[name] = e
        print(name, e, flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        json.dump({"commit": commit, "iterations": ITERATIONS, "eva_iter": EVA_ITER, "entries": entries}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
