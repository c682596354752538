"""The inputs of the enhancement tests, in NumPy and seeded: the spectrograms every GPU test of k_enhance runs on (so that
tests/test_enhance_host.py can check, without a GPU, that the definition's one branch cannot flip on any of them), and the
16 kHz signals of the host tests with a plain 512 / 128 periodic-Hann STFT."""
import functools

import numpy as np

import _enhance_oracle as eo

TILE = 32                       # enhance._TILE_FRAMES (tests/test_enhance_host.py asserts that it is)
F_SET = (1, 63, 65, 257)
B_SET = (1, 3)
KINDS = ("complex64", "float32", "complex128")


def t_set(tile=TILE):
    return (1, 3, tile - 1, tile, tile + 1, 2 * tile + 5)


def make_spec(B, F, T, kind, seed=0):
    """(B, F, T): complex Gaussian noise whose level differs from bin to bin, and in every chain one burst 20 dB above it with a
    random start and length - short ones, and ones long enough for Pbar to cross 0.99."""
    rng = np.random.default_rng([seed, B, F, T])
    level = 10.0 ** rng.uniform(-1.0, 1.0, size=(B, F, 1))
    z = (rng.standard_normal((B, F, T)) + 1j * rng.standard_normal((B, F, T))) * np.sqrt(0.5)
    start = rng.integers(0, T, size=(B, F, 1))
    length = rng.integers(0, T + 1, size=(B, F, 1))
    t = np.arange(T)[None, None, :]
    burst = (t >= start) & (t < start + length)
    z = z * level * np.where(burst, 10.0, 1.0)
    if kind == "complex64":
        return z.astype(np.complex64)
    if kind == "complex128":
        return z
    if kind == "float32":
        return np.abs(z).astype(np.float32)
    raise ValueError(kind)


def grid_shapes(tile=TILE):
    return [(B, F, T) for T in t_set(tile) for F in F_SET for B in B_SET]


@functools.lru_cache(maxsize=None)
def grid_oracle(T, kind, rule, tile=TILE):
    """the oracle over every chain of the grid's shapes with T frames at once (the chains are independent): {(B, F): dict}"""
    specs = {(B, F): make_spec(B, F, T, kind) for F in F_SET for B in B_SET}
    P = np.concatenate([eo.power(s).reshape(-1, T) for s in specs.values()], axis=0)
    res = eo.enhance(P, rule=rule)
    out, row = {}, 0
    for (B, F) in specs:
        n = B * F
        out[(B, F)] = {k: (v[row:row + n].reshape((B, F) + v.shape[1:])) for k, v in res.items()}
        row += n
    return out


# the other GPU tests' inputs: name -> (B, F, T, kind, seed)
NAMED = {
    "chunks": (3, 65, 2 * TILE + 5, "complex64", 11),
    "layout": (3, 63, TILE + 1, "complex64", 12),
    "strided": (2, 65, 2 * TILE + 5, "complex64", 13),
    "batch": (1, 63, TILE + 1, "complex64", 14),
    "nullable": (3, 65, TILE + 1, "complex64", 15),
    "halves": (2, 63, TILE + 1, "complex64", 16),
    "looped": (1, 4096 * 64 + 5, 2, "float32", 17),
}


def named(name):
    B, F, T, kind, seed = NAMED[name]
    return make_spec(B, F, T, kind, seed)


def every_gpu_input(tile=TILE):
    """(label, spectrogram) over everything a GPU test feeds the tracker"""
    for kind in KINDS:
        for (B, F, T) in grid_shapes(tile):
            yield f"grid {kind} {(B, F, T)}", make_spec(B, F, T, kind)
    for name in NAMED:
        yield name, named(name)


# ---- the host tests' signals

SR, N_FFT, HOP = 16000, 512, 128


def stft(x):
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)
    n = 1 + (len(x) - N_FFT) // HOP
    idx = np.arange(N_FFT)[None, :] + HOP * np.arange(n)[:, None]
    return np.fft.rfft(x[idx] * w, axis=1).T            # (F, T)


def white(n, seed, level=1.0):
    return level * np.random.default_rng(seed).standard_normal(n)


def voice(n, seed):
    """eleven amplitude-modulated chirping harmonics with pauses"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    f0 = 140.0 + 40.0 * np.sin(2.0 * np.pi * 0.7 * t) + 15.0 * t
    phase = 2.0 * np.pi * np.cumsum(f0) / SR
    x = np.zeros(n)
    for h in range(1, 12):
        x += (1.0 / h) * (1.0 + 0.5 * np.sin(2.0 * np.pi * (2.0 + 0.3 * h) * t + rng.uniform(0, 2 * np.pi))) * np.sin(h * phase)
    gate = ((t % 0.5) >= 0.15).astype(np.float64)       # 0.15 s of pause in every half second, the first at the start
    k = np.hanning(161)
    gate = np.convolve(gate, k / k.sum(), mode="same")
    return x * gate
