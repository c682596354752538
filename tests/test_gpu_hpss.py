"""hpss on the device against the definition in NumPy float64 (tests/_hpss_oracle.py) on the input's own bits.

k_hpss gives a workgroup TF x 32 outputs (f, t): 32 along time always; TF = 32 rows for float32 magnitudes with k_h + k_p <= 129,
16 rows for every other float32 size and wherever the staged values are float64 (a float64 or a complex input).  So the edges are
31, 32, 33 frames, and 15, 16, 17 and 31, 32, 33 rows; every shape below runs every size in every dtype, with (2, 70, 2), (2, 2, 70),
(2, 5, 3), (1, 3, 5) and (1, 1) shorter than half of most windows.  There is one selection path, so the sweep over every odd size
on one input - float32 changes its tile between 63 and 65 there - is what guards its loop bounds.

Tolerances (none measured into being):
  medians, real or complex64 input: bit for bit - a median is a window element, and rounding is monotonic, so the float64 oracle
    rounded to the output dtype is the rounded element.
  medians, complex128: 2 ulp, the float64 sum of squares and its root are not exact there.
  masks and components, float32 / complex64: |out - ref| <= 2^-23 |ref|: the value is computed in float64 and rounded once (2^-24);
    the bound is one float32 ulp, twice that.
  masks and components, float64 / complex128: 32 * 2^-52 |ref|.  Each quotient carries half an ulp, amplified by p <= 3; pow adds
    1 ulp to a and to r; the sum and the last quotient half an ulp each: under 7 ulp, and the bound is four times that.
  p = inf: exact, the comparison X > m Y is one IEEE float64 product on both sides.
"""
import numpy as np
import pytest
import torch

import spectrogram_inversion_amd as si
from _hpss_oracle import masks, masks_of, medians, times

pytestmark = pytest.mark.gpu

F16, BF16, F32, F64, C32, C64, C128 = (torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.complex32,
                                       torch.complex64, torch.complex128)
DEV = "cuda"
NAME = {F32: "f32", F64: "f64", C64: "c64", C128: "c128"}
NP_REAL = {F32: np.float32, C64: np.float32, F64: np.float64, C128: np.float64}
T_REAL = {F32: F32, C64: F32, F64: F64, C128: F64}

# (B (None: unbatched), F, T): the issue's six, then 31 / 32 / 33 frames and 15 / 16 / 17 / 31 / 32 / 33 rows (the tiles' edges) with
# 40 on the other axis
SHAPES = [(None, 1, 1), (1, 3, 5), (2, 5, 3), (2, 70, 2), (2, 2, 70), (3, 33, 129),
          (2, 40, 31), (2, 40, 32), (2, 40, 33), (2, 31, 40), (2, 32, 40), (2, 33, 40), (2, 15, 40), (2, 16, 40), (2, 17, 40)]
SIZES = [1, 3, 5, 17, 31, 127, (31, 5), (5, 127)]
POWERS = (1, 2, 0.5, 3)
MARGINS = (1, (2, 1), (1, 3.5))


def _pair(v):
    return v if isinstance(v, tuple) else (v, v)


def _make(kind, shape, dtype, seed):
    """a CPU tensor of `dtype`: 'random' magnitudes, 'quarters' (magnitudes quantised to quarters, every third row and column exact
    zeros: ties in every window, silent frames, Z < tiny bins), or random complex values for a complex dtype"""
    gen = torch.Generator().manual_seed(seed)
    full = tuple(d for d in shape if d is not None)
    if dtype.is_complex:
        re, im = torch.randn(full, generator=gen, dtype=F64), torch.randn(full, generator=gen, dtype=F64)
        return torch.complex(re, im).to(dtype)
    if kind == "random":
        return torch.randn(full, generator=gen, dtype=F64).abs().to(dtype)
    x = torch.round(8 * torch.rand(full, generator=gen, dtype=F64)) / 4
    x[..., ::3, :] = 0
    x[..., :, ::3] = 0
    return x.to(dtype)


def _np(x):
    return x.numpy()


def _rounded(ref, dtype):
    return torch.from_numpy(np.ascontiguousarray(ref)).to(T_REAL[dtype])


KINDS = [("random", F32), ("random", F64), ("quarters", F32), ("quarters", F64), ("complex", C64)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(d) for d in s if d is not None))
@pytest.mark.parametrize("kind,dtype", KINDS, ids=lambda v: NAME.get(v, v))
def test_medians_are_the_definitions_bit_for_bit(shape, kind, dtype):
    x = _make(kind, shape, dtype, seed=sum(d or 0 for d in shape))
    xd = x.to(DEV)
    for size in SIZES:
        k_h, k_p = _pair(size)
        harm, perc = si.hpss_medians(xd, size)
        rh, rp = medians(_np(x), k_h, k_p)
        assert harm.dtype == perc.dtype == T_REAL[dtype] and harm.shape == perc.shape == x.shape and harm.device.type == "cuda"
        assert torch.equal(harm.cpu(), _rounded(rh, dtype)), (size, "harm")
        assert torch.equal(perc.cpu(), _rounded(rp, dtype)), (size, "perc")
        if not dtype.is_complex:                       # input elements, bit for bit
            assert np.isin(_np(harm.cpu()), _np(x)).all() and np.isin(_np(perc.cpu()), _np(x)).all()


@pytest.mark.parametrize("shape", [(2, 5, 3), (3, 33, 129), (2, 17, 40)], ids=lambda s: "x".join(map(str, s)))
def test_medians_of_complex128_within_two_ulp(shape):
    x = _make("complex", shape, C128, seed=3)
    for size in SIZES:
        harm, perc = si.hpss_medians(x.to(DEV), size)
        for got, ref in zip((harm, perc), medians(_np(x), *_pair(size))):
            assert got.dtype == F64
            assert (np.abs(_np(got.cpu()) - ref) <= 2 * 2.0 ** -52 * ref).all(), size


@pytest.mark.parametrize("dtype", (F32, C64), ids=("f32", "c64"))
def test_every_odd_size_on_one_input(dtype):
    x = _make("quarters" if dtype == F32 else "complex", (2, 40, 40), dtype, seed=11)
    xd = x.to(DEV)
    for k in range(1, 128, 2):
        harm, perc = si.hpss_medians(xd, k)
        rh, rp = medians(_np(x), k, k)
        assert torch.equal(harm.cpu(), _rounded(rh, dtype)) and torch.equal(perc.cpu(), _rounded(rp, dtype)), k


def _within(got, ref, rel, what):
    got = _np(got.cpu())
    wide = got.astype(np.complex128 if np.iscomplexobj(got) else np.float64)
    parts = ((wide.real, ref.real), (wide.imag, ref.imag)) if np.iscomplexobj(ref) else ((wide, ref),)
    for g, r in parts:
        err = np.abs(g - r)
        worst = float((err / np.where(r == 0, 1.0, np.abs(r))).max())
        assert (err <= rel * np.abs(r)).all(), (what, worst, rel)
    return got


MASK_SHAPES = [(2, 5, 3), (2, 70, 2), (3, 33, 129)]
MASK_SIZES = [3, 31, (31, 5), (5, 127)]


@pytest.mark.parametrize("shape", MASK_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind,dtype", [("random", F32), ("quarters", F32), ("complex", C64), ("random", F64), ("quarters", F64),
                                        ("complex", C128)], ids=lambda v: NAME.get(v, v))
def test_masks_and_components(shape, kind, dtype):
    x = _make(kind, shape, dtype, seed=5 + shape[1])
    xd = x.to(DEV)
    rel = 2.0 ** -23 if T_REAL[dtype] == F32 else 32 * 2.0 ** -52
    for i, size in enumerate(MASK_SIZES):
        harm, perc = medians(_np(x), *_pair(size))
        for power in POWERS:
            # every margin on the largest shape, one of the three in turn on the others
            for m in (MARGINS if shape == MASK_SHAPES[-1] else (MARGINS[(i + POWERS.index(power)) % 3],)):
                ref_h, ref_p = masks_of(harm, perc, power, *(float(v) for v in _pair(m)), real_dtype=NP_REAL[dtype])
                mh, mp = si.hpss(xd, size, power, True, m)
                assert mh.dtype == mp.dtype == T_REAL[dtype] and mh.shape == x.shape
                for got, ref in ((mh, ref_h), (mp, ref_p)):
                    g = _within(got, ref, rel, (size, power, m, "mask"))
                    assert g.min() >= 0 and g.max() <= 1
                H, P = si.hpss(xd, size, power, False, m)
                assert H.dtype == P.dtype == dtype and H.shape == x.shape
                _within(H, times(_np(x), ref_h), rel, (size, power, m, "H"))
                _within(P, times(_np(x), ref_p), rel, (size, power, m, "P"))


@pytest.mark.parametrize("kind,dtype", [("quarters", F32), ("complex", C64), ("quarters", F64), ("complex", C128)],
                         ids=lambda v: NAME.get(v, v))
def test_binary_masks_are_exact(kind, dtype):
    x = _make(kind, (3, 33, 129), dtype, seed=8)
    for size in (5, (31, 5)):
        for m in MARGINS:
            mh, mp = si.hpss(x.to(DEV), size, float("inf"), True, m)
            ref_h, ref_p = masks(_np(x), *_pair(size), float("inf"), *(float(v) for v in _pair(m)), real_dtype=NP_REAL[dtype])
            assert torch.equal(mh.cpu(), _rounded(ref_h, dtype)) and torch.equal(mp.cpu(), _rounded(ref_p, dtype))
            assert np.isin(_np(mh.cpu()), (0.0, 1.0)).all()


def test_silence_takes_the_tiny_rule():
    z = torch.zeros(2, 9, 40, device=DEV)
    for out in si.hpss(z, 5, 2.0, True):
        assert (out == 0.5).all()
    for out in si.hpss(z, 5, 2.0, True, (2.0, 1.0)) + si.hpss(z, 5, 0.5, False):
        assert (out == 0).all()
    q = torch.full((4, 40), 1e-39, device=DEV)               # below float32's smallest normal number: silence in float32 ...
    assert (si.hpss(q, 3, 2.0, True)[0] == 0.5).all()
    assert (si.hpss(q.double(), 3, 3.0, True, (2.0, 1.0))[1] > 0).all()          # ... and not in float64


def test_components_of_a_complex_input_are_spec_times_mask():
    """H is S times the float64 mask rounded once; S times the returned mask rounds the mask and then the product: two roundings of
    2^-24 apart at most, per part"""
    x = _make("complex", (3, 33, 129), C64, seed=9).to(DEV)
    for m in MARGINS:
        (H, P), (mh, mp) = si.hpss(x, (31, 5), 2.0, False, m), si.hpss(x, (31, 5), 2.0, True, m)
        for got, mask in ((H, mh), (P, mp)):
            ref = _np((x.to(C128) * mask.double()).cpu())
            _within(got, ref, 2.0 ** -23 * (1 + 2.0 ** -20), ("spec * mask", m))
    # margin 1: H + P = S up to the roundings of H and P (2^-24 |H|, 2^-24 |P|, |H| + |P| = |S|) and of the float32 sum and
    # difference formed here (2^-24 |S| each), every one of them relative to its own part: 3 * 2^-24 |S| in all, held to 2^-22 |S|
    h2, p2 = si.hpss(x, 31)
    assert (_np((h2 + p2 - x).abs().cpu()) <= 2.0 ** -22 * _np(x.abs().cpu())).all()


@pytest.mark.parametrize("dtype,wide", ((F16, F32), (BF16, F32), (C32, C64)), ids=("f16", "bf16", "c32"))
def test_a_half_input_is_the_float32_call_rounded_back(dtype, wide):
    x = _make("complex" if dtype == C32 else "random", (2, 33, 40), C64 if dtype == C32 else F32, seed=4).to(DEV).to(dtype)
    real = F16 if dtype == C32 else dtype
    for got, ref in zip(si.hpss(x, 5) + si.hpss(x, 5, mask=True) + si.hpss_medians(x, 5),
                        si.hpss(x.to(wide), 5) + si.hpss(x.to(wide), 5, mask=True) + si.hpss_medians(x.to(wide), 5)):
        want = ref.to(dtype if ref.is_complex() else real)
        assert got.dtype == want.dtype and got.device.type == "cuda"
        assert torch.equal(got.to(C64), want.to(C64)) if got.is_complex() else torch.equal(got, want)


def test_a_cpu_tensor_comes_back_to_the_cpu_and_a_view_gives_the_contiguous_bits():
    x = _make("complex", (2, 33, 40), C64, seed=6)
    for got, ref in zip(si.hpss(x, 5) + si.hpss_medians(x, 5), si.hpss(x.to(DEV), 5) + si.hpss_medians(x.to(DEV), 5)):
        assert got.device.type == "cpu" and got.dtype == ref.dtype and torch.equal(got, ref.cpu())
    xt = _make("random", (2, 40, 33), F32, seed=7).to(DEV).transpose(1, 2)
    assert not xt.is_contiguous()
    for got, ref in zip(si.hpss(xt, (5, 17)), si.hpss(xt.contiguous(), (5, 17))):
        assert torch.equal(got, ref)
    one = si.hpss_medians(xt[1], 5)
    assert torch.equal(one[0], si.hpss_medians(xt, 5)[0][1]) and si.hpss(torch.zeros(0, 4, 5, device=DEV))[0].shape == (0, 4, 5)


def test_no_item_bound_is_hidden():
    """batch is part of the flattened grid: 70000 items, and more workgroups than one launch takes (2^22)"""
    x = _make("random", (70000, 2, 3), F32, seed=12)
    harm, perc = si.hpss_medians(x.to(DEV), 3)
    rh, rp = medians(_np(x), 3, 3)
    assert torch.equal(harm.cpu(), _rounded(rh, F32)) and torch.equal(perc.cpu(), _rounded(rp, F32))
    y = torch.rand((1 << 22) + 5, 1, 1, device=DEV)
    harm, perc = si.hpss_medians(y, 3)                        # a single bin is every element of its windows
    assert torch.equal(harm, y) and torch.equal(perc, y)
    assert (si.hpss(y, 3, mask=True)[1] == 0.5).all()


def test_offsets_beyond_two_to_the_31():
    """33 x 8192 x 8192 bins: the last item lies past 2^31 elements; its corner against the definition (the crop's own top row and
    left column reflect differently, so they are left out)"""
    x = torch.rand(33, 8192, 8192, device=DEV)
    assert x.numel() > 1 << 31
    harm, perc = si.hpss_medians(x, 3)
    crop = x[-1, -50:, -50:].cpu()
    rh, rp = medians(_np(crop), 3, 3)
    assert torch.equal(harm[-1, -49:, -49:].cpu(), _rounded(rh, F32)[1:, 1:])
    assert torch.equal(perc[-1, -49:, -49:].cpu(), _rounded(rp, F32)[1:, 1:])


AUDIO = dict(hop_length=32, window=torch.hann_window(128))


def _audio(dtype=F32):
    gen = torch.Generator().manual_seed(21)
    t = torch.arange(2048, dtype=F64)
    tone = torch.sin(2 * np.pi * 0.05 * t) + 0.5 * torch.sin(2 * np.pi * 0.13 * t)
    clicks = torch.zeros(2, 2048, dtype=F64)
    clicks[:, ::256] = 4.0
    return (tone + clicks + 0.05 * torch.randn(2, 2048, generator=gen, dtype=F64)).to(dtype).to(DEV)


def test_hpss_audio_without_iterations_is_the_composition():
    x = _audio()
    x_h, x_p = si.hpss_audio(x, 128, **AUDIO)
    H, P = si.hpss(si.stft(x, 128, **AUDIO), 31, 2.0, False, 1.0)
    assert torch.equal(x_h, si.istft(H, **AUDIO)) and torch.equal(x_p, si.istft(P, **AUDIO))
    assert x_h.shape == x_p.shape == (2, 2048) and x_h.dtype == F32
    y_h, y_p = si.hpss_audio(x, 128, (17, 5), 1.0, (2.0, 1.5), **AUDIO)
    H, P = si.hpss(si.stft(x, 128, **AUDIO), (17, 5), 1.0, False, (2.0, 1.5))
    assert torch.equal(y_h, si.istft(H, **AUDIO)) and torch.equal(y_p, si.istft(P, **AUDIO))
    assert torch.equal(si.harmonic(x, 128, **AUDIO), x_h) and torch.equal(si.percussive(x, 128, **AUDIO), x_p)


def test_hpss_audio_with_iterations_is_misi_from_the_components():
    x = _audio()
    x_h, x_p = si.hpss_audio(x, 128, max_iter=3, verbose=False, **AUDIO)
    H, P = si.hpss(si.stft(x, 128, **AUDIO), 31, 2.0, False, 1.0)
    y = si.misi(torch.stack([H, P], -3), x, max_iter=3, verbose=False, **AUDIO)
    assert tuple(y.shape) == (2, 2, 2048)
    assert torch.equal(x_h, y[:, 0]) and torch.equal(x_p, y[:, 1])
    L = x_h.shape[-1]
    eps = np.finfo(np.float32).eps
    gap = float((x_h.double() + x_p.double() - x[:, :L].double()).abs().max())
    bound = 4 * 2 * eps * float(y.abs().max())                 # tests/test_gpu_misi.py's bound for the sum of K = 2 sources
    print(f"sum gap {gap:.3e} bound {bound:.3e}")
    assert gap <= bound
    assert torch.equal(si.harmonic(x, 128, max_iter=3, verbose=False, **AUDIO), x_h)
    assert torch.equal(si.percussive(x, 128, max_iter=3, verbose=False, **AUDIO), x_p)
    one_h, one_p = si.hpss_audio(x[0], 128, max_iter=3, verbose=False, **AUDIO)
    assert one_h.shape == one_p.shape == (2048,)


def test_a_call_does_not_disturb_a_running_method():
    from spectrogram_inversion_amd.plan import args_helper, get_plan
    x = _audio()
    spec = si.stft(x, 128, **AUDIO)
    plan = get_plan(args_helper(spec, **AUDIO), 2, spec.shape[-1], F32, spec.device)

    def run(between):
        plan.gla_init(spec, spec.abs(), 0.99)
        plan.iterate(2)
        between()
        plan.iterate(2)
        return plan.wave().clone()

    quiet = run(lambda: None)
    busy = run(lambda: (si.hpss(spec), si.hpss_medians(spec.abs(), (5, 127)), si.hpss(spec.abs().double(), 127, mask=True)))
    assert torch.equal(quiet, busy)
