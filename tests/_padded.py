"""Zero-padded batches, silence and quiet audio: the inputs of tests/test_padded_host.py and tests/test_gpu_padded.py, the table of
cases both files go through, and the oracle's results on them, computed once per process.  A helper, not a test file; needs no GPU.

A batch of four items of one length L, cut from `_gla_torch.wellcond`:

    item 0  silent from 0.6 L on                                     (an utterance padded to the longest of its batch)
    item 1  silent up to 0.25 L, and over 3 n_fft samples centred on L / 2      (leading silence and a pause)
    item 2  full length, 4 n_fft samples centred on L / 2 scaled by 2^quiet_pow  (a quiet passage)
    item 3  all zeros

and the whole batch times `scale`, a power of two.  A frame over silence has a target of exactly 0, and after the first inverse
transform an estimate of exactly 0 too: the projection S m / (|S| + 1e-16) is then evaluated at S = 0, m = 0."""
import collections
import functools

import numpy as np

import _agla_oracle as ao
import _cgla_oracle as co
import _misi_oracle as mo
import oracle
from _gla_torch import wellcond
from _proj_torch import hamming
from _util import hann, rel_l2
from oracle.stftlib import args_helper, signal_length

Case = collections.namedtuple("Case", "x spec mag start kw length dead silent quiet")
BATCH = 4


def _runs(idx):
    """the longest run of consecutive integers in the sorted index list `idx`"""
    best = cur = 0
    for i, v in enumerate(idx):
        cur = cur + 1 if i and v == idx[i - 1] + 1 else 1
        best = max(best, cur)
    return best


def _window(n_fft, extra, dtype):
    wl = extra.get("win_length", n_fft)
    # (center=False: a Hamming window - under a Hann window the envelope vanishes at the first sample, 0 / 0 in the reference too)
    return hamming(wl, dtype) if extra.get("center") is False else hann(wl, dtype)


def padded_case(n_fft, hop, frames, extra, dtype, quiet_pow=-20, scale=1.0):
    """-> Case: x (4, L) the padded signals (float32 values, in `dtype`); spec their STFT, float32 arithmetic; mag = |spec| widened to
    `dtype`, so that both dtypes see the same numbers; start: the true phase + 0.5 rad rms on those magnitudes, exactly 0 where the
    bin is 0, computed in complex64 and widened; kw the stft kwargs (the float32 window widened); per item the mask `dead` of the
    samples that only silent frames cover and the list `silent` of silent frames; quiet = (begin, end) of item 2's quiet stretch."""
    assert np.log2(scale) == int(np.log2(scale))
    seed = n_fft + hop + frames
    w32 = _window(n_fft, extra, np.float32)
    kw32 = dict(hop_length=hop, window=w32, **extra)
    F = n_fft // 2 + 1 if extra.get("onesided", True) else n_fft
    a = args_helper(F, np.float32, **kw32)
    L = signal_length(frames, a)
    x = np.zeros((BATCH, L), np.float32)
    x[:3] = wellcond(3, L, seed)
    x[0, int(0.6 * L):] = 0
    x[1, :int(0.25 * L)] = 0
    g0 = max(0, L // 2 - (3 * n_fft) // 2)
    x[1, g0:g0 + 3 * n_fft] = 0
    q0 = max(0, L // 2 - 2 * n_fft)
    quiet = (q0, min(L, q0 + 4 * n_fft))
    x[2, quiet[0]:quiet[1]] *= np.float32(2.0 ** quiet_pow)
    x *= np.float32(scale)
    spec = oracle.stft(x, a)
    assert spec.dtype == np.complex64 and spec.shape == (BATCH, F, frames)
    mag = np.abs(spec)
    noise = (0.5 * np.random.default_rng(seed + 1).standard_normal(spec.shape)).astype(np.float32)
    phase = np.angle(spec) + noise
    start = (mag * (np.cos(phase) + 1j * np.sin(phase))).astype(np.complex64)
    assert np.array_equal(start == 0, mag == 0) and np.array_equal(np.abs(start) == 0, mag == 0)
    live = mag.max(1) > 0                                                      # (4, frames)
    silent = [np.flatnonzero(~live[b]) for b in range(BATCH)]
    covered = np.zeros((BATCH, L + 2 * a.padding), bool)                        # by a frame that is not silent
    for b in range(BATCH):
        for t in np.flatnonzero(live[b]):
            covered[b, t * hop:t * hop + n_fft] = True
    dead = ~covered[:, a.padding:a.padding + L]
    for b in (0, 1, 3):
        assert _runs(silent[b]) >= n_fft / hop + 2, (b, _runs(silent[b]), n_fft / hop + 2)
    assert len(silent[3]) == frames and dead[3].all() and not len(silent[2]) and dead[:2].any(1).all() and not dead[2].any()
    kw = dict(kw32, window=w32.astype(dtype))
    cd = np.complex64 if dtype == np.float32 else np.complex128
    return Case(x.astype(dtype), spec, mag.astype(dtype), start.astype(cd), kw, L, dead, silent, quiet)


# ---- the methods ---------------------------------------------------------------------------------------------------------------------
# name: (kind, iterations, parameters).  Iteration counts and coefficients: 5 at alpha 0.99, 3 at rho 0.5; a
# start from the magnitudes goes through phase_init (its float32 cumulative sum: DESIGN 3.9), and takes 3 at alpha 0.3 where 5 at 0.99
# is beyond the cap of 1e-3 on the oracle's own float32-against-float64 distance (MAG_GENTLE).
AGLA_PARAMS = {"fgla": (0.99, None, 1.0), "general": (0.5, 1.2, 0.7)}      # tests/test_gpu_agla.py's PARAMS
METHODS = {
    "gla": ("gla", 5, 0.99), "gla_mag": ("gla", 5, 0.99), "admm": ("admm", 3, 0.5),
    "agla_fgla": ("agla", 5, AGLA_PARAMS["fgla"]), "agla_general": ("agla", 5, AGLA_PARAMS["general"]),
    "misi": ("misi", 5, None), "cgla": ("cgla", 5, AGLA_PARAMS["general"]),
}
GENTLE = ("gla", 3, 0.3)
CAP = {"gla": 1e-5, "admm": 1e-5, "agla_fgla": 1e-5, "agla_general": 1e-5, "misi": 1e-5, "cgla": 1e-5, "gla_mag": 1e-3, "rtisi": 5e-3}
# dead samples are exactly 0 in the reference's result (ADMM's dual variable leaks into them; MISI's coupling step adds the other
# source's error); the all-silent item is exactly 0 under every method
DEAD_ZERO = ("gla", "gla_mag", "agla_fgla", "agla_general", "cgla", "rtisi")


def method_of(key, method):
    """(kind, iterations, parameters) of `method` on the case `key`"""
    return GENTLE if method == "gla_mag" and key in MAG_GENTLE else METHODS[method]


def items_of(method):
    """the items of the batch a method runs on: MISI's two sources are items 0 and 1, their sum is the mixture"""
    return [0, 1] if method == "misi" else [0, 1, 2, 3]


def cgla_constraint(c):
    """the bins below F / 4 known (the true STFT) and the samples of the first quarter known: (known_spec, spec_mask, known_wave, wave_mask)"""
    M = np.zeros(c.spec.shape, bool)
    F = c.spec.shape[1]
    k = np.arange(F)
    if not c.kw.get("onesided", True):                   # a two-sided spectrum: the mirror bins with them (a Hermitian mask)
        k, F = np.minimum(k, F - k), F // 2 + 1
    M[:, k < F // 4] = True
    W = np.zeros(c.x.shape, bool)
    W[:, :c.length // 4] = True
    return c.spec.astype(c.start.dtype), M, c.x, W


def run_oracle(c, kind, iters, prm, from_mag=False):
    """The oracle on the case `c` (in c's dtype), the last iteration evaluating: (y, sums) with sums = (sum (|S| - m)^2 / count, sum m^2)
    from float64 accumulation, or None where the method's evaluation is not compared."""
    spec = c.mag if from_mag else c.start
    with np.errstate(all="ignore"):
        if kind == "gla":
            tr = []
            y = oracle.griffin_lim(spec, max_iter=iters, alpha=prm, tol=0, eva_iter=iters, trace=tr, **c.kw)
        elif kind == "admm":
            tr = []
            y = oracle.admm(spec, max_iter=iters, rho=prm, tol=0, eva_iter=iters, trace=tr, **c.kw)
        elif kind == "agla":
            tr = []
            y = ao.agla(spec, iters, alpha=prm[0], beta=prm[1], gamma=prm[2], eva_iter=iters, trace=tr, **c.kw)
        elif kind == "misi":
            tr = []
            y = mo.misi(spec[None, :2], c.x[0] + c.x[1], iters, eva_iter=iters, trace=tr, **c.kw)[0]
        elif kind == "cgla":
            K, M, xk, W = cgla_constraint(c)
            y = co.cgla(spec, iters, K, M, xk, W, alpha=prm[0], beta=prm[1], gamma=prm[2], eva_iter=iters, **c.kw)
            return y, None
    m = np.abs(spec[:2] if kind == "misi" else spec).astype(np.float64)
    return y, (tr[-1][2], float((m * m).sum()))


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
# name: n_fft, hop, frames, extra stft kwargs, dtype, route.  The shape and routing tables of tests/test_gpu_agla.py at 34 - 48 frames.
# Routes: "plain" - the planner's own choice for a small problem (k_semi / k_semi2 + overlap-add; k_wave_iter); "chunked" - the
# chunk-walking float32 kernels switched on for small problems (conftest: chunked_kernel); "generic" - force_generic with the coverage
# kernel switched off (k_iter_pair).  1024 / 77 of that table cannot hold n_fft / hop + 2 = 15.3 consecutive silent frames in item 0 at
# 48 frames: hop 77 runs at n_fft 512.  Shapes that missed a cap of tests/test_padded_host.py were replaced within their kernel family:
# 1024 / 512 (1.8e-5 from the complex start) by 512 / 256, the two-sided 1024 / 256 and 1024 / 300 (1.5e-3, 2.8e-3 from the
# magnitudes) by 512 / 128 and 512 / 150, 2048 / 512 at 34 frames by 40.
f32, f64 = np.float32, np.float64
CASES = {
    # fused float32
    "1024/256": (1024, 256, 40, {}, f32, "chunked"),
    "2048/512": (2048, 512, 40, {}, f32, "chunked"),
    "2048/512 skewed": (2048, 512, 40, {}, f32, "chunked"),                    # two chunks of 20 frames, 4 of skew (gla alone)
    "512/256": (512, 256, 36, {}, f32, "chunked"),                             # hop = n_fft / 2
    "2048/256": (2048, 256, 48, {}, f32, "chunked"),                           # hop = n_fft / 8
    "4096/1024": (4096, 1024, 34, {}, f32, "chunked"),                         # (not from the magnitudes: NO_MAG)
    "4096/512": (4096, 512, 40, {}, f32, "chunked"),
    # frame kernels
    "512/128 semi": (512, 128, 40, {}, f32, "plain"),
    "1024/256 center=False": (1024, 256, 40, dict(center=False), f32, "plain"),
    "512/128 two-sided": (512, 128, 38, dict(onesided=False), f32, "plain"),
    # hop kernels
    "512/77": (512, 77, 48, {}, f32, "chunked"),
    "1024/300": (1024, 300, 40, {}, f32, "chunked"),
    "512/150 two-sided": (512, 150, 34, dict(onesided=False), f32, "chunked"),
    # coverage kernels
    "256/64": (256, 64, 40, dict(pad_mode="constant"), f32, "plain"),
    "256/77": (256, 77, 40, {}, f32, "plain"),
    "400/160": (400, 160, 40, {}, f32, "plain"),
    "512/128 f64": (512, 128, 40, {}, f64, "plain"),
    "2048/512 f64": (2048, 512, 40, {}, f64, "plain"),
    # (odd frame counts here: a silence boundary then falls inside one of the frame PAIRS these kernels transform together)
    "256/64 generic": (256, 64, 39, dict(pad_mode="constant"), f32, "generic"),
    "256/77 generic": (256, 77, 40, {}, f32, "generic"),
    "400/160 generic": (400, 160, 40, {}, f32, "generic"),
    "512/128 f64 generic": (512, 128, 39, {}, f64, "generic"),
    "2048/512 f64 generic": (2048, 512, 45, {}, f64, "generic"),
}
# what launch_geometry must report: (Griffin-Lim, every other method; Griffin-Lim with keep_state runs the latter too), the least
# count of chunks, the frames per chunk to force (None: the planner's split)
GEOMETRY = {
    "1024/256": ("k_fused4_td", "k_fused4", 2, None), "2048/512": ("k_fused4_td", "k_fused4", 2, None),
    "2048/512 skewed": ("k_fused4_td", "k_fused4", 2, 20),
    "512/256": ("k_fused_td", "k_fused", 2, None), "2048/256": ("k_fused_td", "k_fused", 2, None),
    "4096/1024": ("k_fused", "k_fused", 2, None), "4096/512": ("k_fused", "k_fused", 2, None),
    "512/128 semi": ("k_semi", "k_semi", 1, None), "1024/256 center=False": ("k_semi", "k_semi", 1, None),
    "512/128 two-sided": ("k_semi", "k_semi", 1, None),
    "512/77": ("k_hop_td", "k_hop", 2, None), "1024/300": ("k_hop_td", "k_hop", 2, None), "512/150 two-sided": ("k_hop", "k_hop", 2, None),
    "256/64": ("k_wave_iter", "k_wave_iter", 1, None), "256/77": ("k_wave_iter", "k_wave_iter", 1, None),
    "400/160": ("k_wave_iter", "k_wave_iter", 1, None), "512/128 f64": ("k_wave_iter", "k_wave_iter", 1, None),
    "2048/512 f64": ("k_wave_iter", "k_wave_iter", 1, None),
    "256/64 generic": ("k_iter_pair",) * 2 + (1, None), "256/77 generic": ("k_iter_pair",) * 2 + (1, None),
    "400/160 generic": ("k_iter_pair",) * 2 + (1, None), "512/128 f64 generic": ("k_iter_pair",) * 2 + (1, None),
    "2048/512 f64 generic": ("k_iter_pair",) * 2 + (1, None),
}
OVERLAP_ADD = {"256/64": "registers", "256/77": "ring", "400/160": "ring"}      # where k_wave_iter's overlap-add runs
# From the magnitudes the oracle's float32 run is 1.05e-3 (26 frames, 3 iterations at alpha 0.3) or more from its float64 run at
# 4096 / 1024 whatever the frame count between 20 and 40 - the phase of phase_init reaches 1e5 rad there, 8e-3 rad to a float32 ulp;
# that start of the 4096 kernel runs at hop 512.
NO_MAG = ("4096/1024",)
CASE_METHODS = [(k, m) for k in CASES for m in METHODS
                if (k != "2048/512 skewed" or m == "gla") and not (m == "gla_mag" and k in NO_MAG)]
# (case, quiet_pow, scale): int16-range and very quiet audio on one fused, one hop and one coverage shape, and a quiet stretch at
# 2^-40, below the |S| = 3e-9 from which the float32 wave-level chain differs from the reference by design (fast_core.h)
SCALE_CASES = [(k, -20, s) for k in ("1024/256", "1024/300", "256/77") for s in (2.0 ** 15, 2.0 ** -20)]
DEEP_CASES = [(k, -40, 1.0) for k in ("1024/256", "1024/300", "256/77")]
SCALE_METHODS = ("gla", "gla_mag", "agla_general")
# cases whose start from the magnitudes takes 3 iterations at alpha 0.3 (see METHODS): 5 at 0.99 measured 1.2e-3 ... 2.2e-3 there
MAG_GENTLE = {"2048/512", "2048/512 f64", "2048/512 f64 generic", "512/256", "4096/512", "512/150 two-sided"}

# RTISI_LA: name: n_fft, hop, frames, dtype, look_ahead; 2 inner iterations, alpha 0.99.  The comparison is on item 0 (trailing
# silence) under the asymmetric window: the quiet-stretch item is ill-conditioned there (1e-2 ... 3e-1 between the oracle's own
# float32 and float64 runs), as is hop = n_fft / 2; the exact zeros hold under both window forms.
RTISI_CASES = {
    "2048/512 LA3": (2048, 512, 40, f32, 3),            # k_rtisi_fast
    "1024/128 LA7": (1024, 128, 48, f32, 7),            # k_rtisi_fast
    "256/64 f64": (256, 64, 40, f64, -1),               # the generic RTISI kernel
}
RTISI_ITERS, RTISI_ALPHA = 2, 0.99


def _key(name, quiet_pow=-20, scale=1.0):
    return (name, quiet_pow, scale)


@functools.lru_cache(maxsize=None)
def case(name, dtype=None, quiet_pow=-20, scale=1.0):
    """the inputs of CASES[name] (or RTISI_CASES[name]), in the case's dtype unless `dtype` says otherwise; left unchanged"""
    if name in CASES:
        n_fft, hop, frames, extra, dt, _ = CASES[name]
    else:
        n_fft, hop, frames, dt, _ = RTISI_CASES[name]
        extra = {}
    c = padded_case(n_fft, hop, frames, extra, dtype or dt, quiet_pow, scale)
    for v in (c.x, c.spec, c.mag, c.start, c.dead, c.kw["window"]):
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(name, method, dtype, quiet_pow=-20, scale=1.0):
    """the oracle's (y, sums) on a case, inputs and arithmetic in `dtype`; computed once and left unchanged"""
    kind, iters, prm = method_of(name, method)
    y, sums = run_oracle(case(name, dtype, quiet_pow, scale), kind, iters, prm, from_mag=method == "gla_mag")
    y.setflags(write=False)
    return y, sums


@functools.lru_cache(maxsize=None)
def rtisi_reference(name, asym, dtype):
    n_fft, hop, frames, _, la = RTISI_CASES[name]
    c = case(name, dtype)
    with np.errstate(all="ignore"):
        y = oracle.rtisi_la(c.mag, look_ahead=la, asymmetric_window=asym, max_iter=RTISI_ITERS, alpha=RTISI_ALPHA, **c.kw)
    y.setflags(write=False)
    return y


def item_rel_l2(y, ref):
    """per item ||y - ref|| / ||ref|| over the samples where ref is finite; nan for an item whose reference is all zeros"""
    y, ref = np.asarray(y, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref) & np.isfinite(y)
    d, r = np.where(fin, y - ref, 0.0), np.where(fin, ref, 0.0)
    nr = np.linalg.norm(r, axis=1)
    with np.errstate(all="ignore"):
        return np.where(nr > 0, np.linalg.norm(d, axis=1) / nr, np.nan)


def block_measure(y, ref, hop):
    """Errors that hide next to a boundary: per item, the largest error over blocks of `hop` samples, each block's error norm
    divided by the item's RMS block norm ||ref||_item / sqrt(n_blocks); nan for an item whose reference is all zeros."""
    y, ref = np.asarray(y, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref) & np.isfinite(y)
    d, r = np.where(fin, y - ref, 0.0), np.where(fin, ref, 0.0)
    nb = -(-y.shape[1] // hop)
    d = np.pad(d, ((0, 0), (0, nb * hop - y.shape[1]))).reshape(y.shape[0], nb, hop)
    nr = np.linalg.norm(r, axis=1)
    with np.errstate(all="ignore"):
        return np.where(nr > 0, np.linalg.norm(d, axis=2).max(1) / (nr / np.sqrt(nb)), np.nan)


@functools.lru_cache(maxsize=None)
def measures(name, method, quiet_pow=-20, scale=1.0):
    """(noise32, block32): per item, the oracle's float32 run against its float64 run on the same float32 numbers - the whole-item
    rel-L2 and the block measure"""
    hop = (CASES[name] if name in CASES else RTISI_CASES[name])[1]
    y32, y64 = reference(name, method, f32, quiet_pow, scale)[0], reference(name, method, f64, quiet_pow, scale)[0]
    return item_rel_l2(y32, y64), block_measure(y32, y64, hop)


@functools.lru_cache(maxsize=None)
def rtisi_measures(name):
    hop = RTISI_CASES[name][1]
    y32, y64 = rtisi_reference(name, True, f32), rtisi_reference(name, True, f64)
    return item_rel_l2(y32, y64), block_measure(y32, y64, hop)


def stretch_of(c, n_fft):
    """the samples of item 2's quiet stretch that only frames inside the stretch cover"""
    return slice(c.quiet[0] + n_fft, c.quiet[1] - n_fft)


@functools.lru_cache(maxsize=None)
def stretch_noise(name, method, quiet_pow, scale=1.0):
    """`measures`' rel-L2 on the quiet stretch of item 2 alone"""
    s = stretch_of(case(name, f32, quiet_pow, scale), CASES[name][0])
    y32, y64 = reference(name, method, f32, quiet_pow, scale)[0], reference(name, method, f64, quiet_pow, scale)[0]
    return rel_l2(y32[2, s], y64[2, s])


F64_GATE = 1e-10                # tests/test_gpu_agla.py's float64 gate
F64_BLOCK_GATE = 1e-9           # ... which bounds the block measure by sqrt(n_blocks) x 1e-10 < 1e-9 at 48 blocks or fewer


def gates(name, method, dtype, quiet_pow=-20, scale=1.0):
    """(gate on the per-item rel-L2, gate on the block measure), per item: the suite's rule (test_gpu_agla._reference_and_gate) - the
    larger of a floor and 6 x the oracle's own float32-against-float64 figure; the floor is 2e-5 from a complex start, 1e-4 from the
    magnitudes, and 1e-4 on the block measure"""
    n = len(items_of(method))
    if dtype == f64:
        return np.full(n, F64_GATE), np.full(n, F64_BLOCK_GATE)
    noise, block = measures(name, method, quiet_pow, scale)
    floor = 1e-4 if method == "gla_mag" else 2e-5
    return np.fmax(floor, 6 * noise), np.fmax(1e-4, 6 * block)
