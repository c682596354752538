"""Speech enhancement without a GPU: the definition pinned through its float64 oracle (tests/_enhance_oracle.py) - E1, the tracker on
stationary and stepped noise, the SNR gained on a voiced signal, chunking through the state, bounds and conditioning - the
condition under which the GPU tests may compare every element, the table of the device's E1 scheme, and the argument checks of
`noise_psd`, `spectral_gain` and `denoise`, which come before the device is touched.  Setup of the signal tests: 16 kHz, 512 / 128
periodic Hann, 2 s, seeded.  The figures beside the asserts are what the oracle gives."""
import os
import re

import numpy as np
import pytest
import torch

import _enhance_inputs as ei
import _enhance_oracle as eo
import spectrogram_inversion_amd as si
from spectrogram_inversion_amd import enhance

N = 2 * ei.SR


def db(x):
    return 10.0 * np.log10(x)


# ---- E1

def test_e1_matches_scipy():
    special = pytest.importorskip("scipy.special")
    v = np.concatenate([np.logspace(-12, np.log10(300.0), 4000), [1.0, np.nextafter(1.0, 2.0), 300.0]])
    err = np.abs(eo.e1(v) / special.exp1(v) - 1.0).max()
    print(f"oracle E1 against scipy on [1e-12, 300]: {err:.2e}")          # 7.2e-15
    assert err <= 1e-12


def test_e1_tabulated_values():
    # Abramowitz & Stegun, table 5.1, and E1(1e-12) = -gamma - ln(1e-12) + 1e-12
    table = {0.5: 0.5597735947761608, 1.0: 0.21938393439552029, 2.0: 0.04890051070806112, 10.0: 4.156968929685324e-06}
    for v, ref in table.items():
        assert abs(eo.e1(np.array([v]))[0] / ref - 1.0) <= 1e-12, v
    assert abs(eo.e1(np.array([1e-12]))[0] / (-eo.EULER - np.log(1e-12) + 1e-12) - 1.0) <= 1e-14


def _device_e1(v):
    """the device's scheme (csrc/kernels_enhance.h: enh_e1) restated on the committed table"""
    path = os.path.join(os.path.dirname(os.path.abspath(enhance.__file__)), "csrc", "enhance_e1_table.h")
    text = open(path).read()

    def array(name):
        body = re.search(name + r"(?:\[\w+(?: \+ 1)?\])+ = \{(.*?)\};", text, re.S).group(1)
        return np.array([float(x) for x in re.findall(r"-?\d[\d.]*(?:e[-+]?\d+)?", body)])

    series, mid, scale = array("kE1SeriesCoef"), array("kE1Mid"), array("kE1Scale")
    cheb = array("kE1Cheb").reshape(len(mid), -1)
    assert len(series) == 18 and cheb.shape == (8, 16)
    v = np.asarray(v, dtype=np.float64)
    out = np.zeros_like(v)
    lo = v <= 1.0
    x = v[lo]
    s = np.full_like(x, series[-1])
    for c in series[-2::-1]:
        s = s * x + c
    out[lo] = (s * x - np.log(x)) - eo.EULER
    hi = ~lo & (v <= 700.0)
    x = v[hi]
    j = np.minimum(np.frexp(x)[1] - 1, len(mid) - 1)
    rv = 1.0 / x
    t = (2.0 * rv - mid[j]) * scale[j]
    tab = cheb[j]
    b1, b2 = np.zeros_like(x), np.zeros_like(x)
    for k in range(tab.shape[1] - 1, 0, -1):
        b1, b2 = tab[:, k] + (2.0 * t * b1 - b2), b1
    out[hi] = np.exp(-x) * rv * (tab[:, 0] + (t * b1 - b2))
    return out


def test_device_e1_scheme_is_within_its_stated_bound():
    """The series and the Chebyshev table the kernel evaluates, in NumPy against the oracle: the bound DESIGN 3.30 states is 1e-13."""
    edges = np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0])
    v = np.concatenate([np.logspace(-12, 0, 2000), np.minimum(np.logspace(0, np.log10(700.0), 8000), 700.0), edges, np.nextafter(edges, 0),
                        np.nextafter(edges, 1e3), [700.0]])
    err = np.abs(_device_e1(v) / eo.e1(v) - 1.0).max()
    print(f"device E1 scheme against the oracle on [1e-12, 700]: {err:.2e}")          # 8.7e-15, the oracle's own error; 4.9e-16 against 50 digits
    assert err <= 1e-13
    assert (_device_e1(np.array([700.1, 1e3, 1e300])) == 0).all()


# ---- the tracker

def test_stationary_noise_level():
    X = ei.stft(ei.white(N, 1))
    P = eo.power(X)
    sig = eo.enhance(P, rule="wiener")["noise"]
    bias = db(sig[:, 50:].mean() / P[:, 50:].mean())
    print(f"stationary white noise: sigma2 against the mean periodogram {bias:+.2f} dB")     # -1.07 dB
    assert abs(bias) <= 2.0


def test_noise_step_is_followed():
    x = ei.white(N, 2)
    x[N // 2:] *= 10.0 ** 0.5                      # + 10 dB from the middle on
    P = eo.power(ei.stft(x))
    sig = eo.enhance(P, rule="wiener")["noise"]
    step = (N // 2) // ei.HOP                       # the first frame that starts in the louder half
    new = P[:, step + 4:].mean()
    level = db(sig.mean(axis=0) / new)
    inside = np.nonzero(np.abs(level[step:]) <= 3.0)[0]
    print(f"+10 dB step: within 3 dB of the new level after {inside[0]} frames")          # 32
    assert inside.size and inside[0] <= 60
    assert (np.abs(level[step + inside[0]:]) <= 3.0).all()


@pytest.mark.parametrize("snr_db", (0.0, 5.0))
def test_snr_gain_on_a_voiced_signal(snr_db):
    s = ei.voice(N, 3)
    n = ei.white(N, 4)
    n *= np.sqrt((s ** 2).mean() / (n ** 2).mean() / 10.0 ** (snr_db / 10.0))
    S, X = ei.stft(s), ei.stft(s + n)
    snr_in = db((np.abs(S) ** 2).sum() / (np.abs(X - S) ** 2).sum())
    P = eo.power(X)
    for rule in ("wiener", "lsa"):
        G = eo.enhance(P, rule=rule)["gain"]
        snr_out = db((np.abs(S) ** 2).sum() / (np.abs(G * X - S) ** 2).sum())
        print(f"voiced signal at {snr_db:g} dB: {snr_in:.2f} -> {snr_out:.2f} dB ({rule})")
        # 0 dB: 0.02 -> 7.13 (wiener) / 7.22 (lsa) ;  5 dB: 5.02 -> 10.12 / 10.28
        assert snr_out - snr_in >= 3.0


# ---- the state, the bypass, bounds

def _speechy():
    s = ei.voice(N, 5)
    return eo.power(ei.stft(s + ei.white(N, 6, 0.3)))[:64, :200]


@pytest.mark.parametrize("rule", ("wiener", "lsa"))
def test_chunked_equals_one_shot_bit_for_bit(rule):
    P = _speechy()
    one = eo.enhance(P, rule=rule)
    # (the start rule reads min(init_frames, T) frames, so the first chunk holds at least init_frames = 5 of them)
    for cut in (5, 6, 77, 199):
        a = eo.enhance(P[:, :cut], rule=rule)
        b = eo.enhance(P[:, cut:], rule=rule, state=a["state"])
        for k in ("noise", "spp", "gain", "snr"):
            assert np.array_equal(np.concatenate([a[k], b[k]], axis=1), one[k]), (cut, k)
        assert np.array_equal(b["state"], one["state"])
    # three chunks, through two states
    a = eo.enhance(P[:, :40], rule=rule)
    b = eo.enhance(P[:, 40:41], rule=rule, state=a["state"])
    c = eo.enhance(P[:, 41:], rule=rule, state=b["state"])
    assert np.array_equal(np.concatenate([a["gain"], b["gain"], c["gain"]], axis=1), one["gain"])
    assert np.array_equal(c["state"], one["state"])


def test_given_noise_makes_the_tracker_irrelevant():
    P = _speechy()
    noise = np.full((64, 1), 0.7)
    a = eo.enhance(P, noise=noise)
    b = eo.enhance(P, noise=noise, init_frames=1, alpha_pow=0.1, alpha_spp=0.2, prior_snr_db=3.0)
    for k in ("noise", "gain", "snr", "state"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["noise"], np.broadcast_to(noise, P.shape))
    assert np.array_equal(eo.enhance(P, noise=np.float64(0.7))["gain"], a["gain"])


@pytest.mark.parametrize("rule", ("wiener", "lsa"))
def test_gain_bounds_and_finiteness(rule):
    g_min = 10.0 ** (-20.0 / 20.0)
    rng = np.random.default_rng(7)
    loud = rng.standard_normal((8, 60)) ** 2
    cases = [_speechy(), np.zeros((4, 40)), loud * 1e-60, loud * 1e60,
             np.concatenate([np.zeros((8, 10)), loud * 1e30], axis=1),          # a zero start: sigma2 = 0 under a huge P
             np.concatenate([loud, np.zeros((8, 30))], axis=1)]
    for P in cases:
        res = eo.enhance(P, rule=rule)
        for k, v in res.items():
            assert np.isfinite(v).all(), k
        assert (res["gain"] >= g_min).all() and (res["gain"] <= 1.0).all() and g_min > 0
        assert (res["noise"] >= 0).all() and (res["snr"] > 0).all()
    res = eo.enhance(loud, noise=np.zeros((8, 1)), rule=rule)                   # a given sigma2 of 0
    assert all(np.isfinite(v).all() for v in res.values())
    assert (res["gain"] == 1.0).all()


def test_conditioning_of_the_chain():
    """Scaling the input by 1 + 1e-15 moves sigma2 and G by a factor s times that: what the GPU tolerances are derived from."""
    P = _speechy()
    eps = 2.0 ** -50                                         # 8.9e-16, exactly representable: P scales by (1 + eps)^2
    worst = 0.0
    for rule in ("wiener", "lsa"):
        a = eo.enhance(P, rule=rule)
        b = eo.enhance(P * ((1.0 + eps) * (1.0 + eps)), rule=rule)
        # sigma2 scales with P (remove that), G does not
        s_sig = np.abs(b["noise"] / a["noise"] / ((1.0 + eps) * (1.0 + eps)) - 1.0).max() / eps
        s_g = np.abs(b["gain"] / a["gain"] - 1.0).max() / eps
        print(f"conditioning ({rule}): s = {s_sig:.1f} (sigma2), {s_g:.1f} (G)")      # 9.2 and 24.1 (wiener), 9.2 and 14.8 (lsa)
        worst = max(worst, s_sig, s_g)
    assert worst <= 100.0


def test_the_branch_cannot_flip_on_any_gpu_input():
    """|Pbar_l - 0.99| over every spectrogram the GPU tests feed the tracker: the definition's one branch then gives the same side
    on the device (whose Pbar differs by a few 1e-16 s), and the GPU tests exclude no element."""
    assert ei.TILE == enhance._TILE_FRAMES
    closest = np.inf
    for label, spec in ei.every_gpu_input():
        P = eo.power(spec).reshape(-1, spec.shape[-1])
        pbar = eo.enhance(P, rule="wiener")["pbar"]
        closest = min(closest, np.abs(pbar - 0.99).min())
        assert closest >= 1e-9, label
    print(f"closest Pbar to 0.99 over the GPU tests' inputs: {closest:.2e}")          # 7.9e-6


# ---- the wrappers' argument checks

def test_exports():
    assert si.noise_psd is enhance.noise_psd and si.spectral_gain is enhance.spectral_gain and si.denoise is enhance.denoise
    assert isinstance(enhance._TILE_FRAMES, int) and enhance._TILE_FRAMES >= 2


def test_wrapper_argument_errors():
    X = torch.zeros(5, 7, dtype=torch.complex64)
    with pytest.raises(TypeError):
        si.noise_psd(np.zeros((5, 7)))
    with pytest.raises(TypeError):
        si.spectral_gain(torch.zeros(5, 7, dtype=torch.int32))
    with pytest.raises(ValueError):
        si.noise_psd(torch.zeros(7))
    with pytest.raises(ValueError):
        si.spectral_gain(torch.zeros(2, 2, 5, 7))
    with pytest.raises(ValueError):
        si.noise_psd(torch.zeros(0, 7))
    for kw in ({"init_frames": 0}, {"init_frames": 2.0}, {"init_frames": True}, {"alpha_pow": 1.5}, {"alpha_spp": -0.1},
               {"alpha_pow": "0.8"}, {"prior_snr_db": float("nan")}, {"prior_snr_db": None}):
        with pytest.raises(ValueError):
            si.noise_psd(X, **kw)
        with pytest.raises(ValueError):
            si.spectral_gain(X, **kw)
    for kw in ({"rule": "stsa"}, {"rule": None}, {"alpha": 1.01}, {"alpha": True}, {"xi_min_db": float("inf")},
               {"gain_floor_db": 1.0}, {"gain_floor_db": float("-inf")}):
        with pytest.raises(ValueError):
            si.spectral_gain(X, **kw)
        with pytest.raises(ValueError):
            si.denoise(torch.zeros(4000), 512, **kw)
    with pytest.raises(TypeError):
        si.spectral_gain(X, noise=0.5)
    with pytest.raises(TypeError):
        si.spectral_gain(X, noise=torch.zeros(5, 1, dtype=torch.complex64))
    with pytest.raises(ValueError):
        si.spectral_gain(X, noise=torch.zeros(4, 1))
    with pytest.raises(ValueError):
        si.spectral_gain(X, noise=torch.zeros(2, 5, 7))
    with pytest.raises(TypeError):
        si.noise_psd(X, state=torch.zeros(5, 3))
    with pytest.raises(TypeError):
        si.noise_psd(X, state=[0.0])
    with pytest.raises(ValueError):
        si.noise_psd(X, state=torch.zeros(7, 3, dtype=torch.float64))
    with pytest.raises(ValueError):
        si.noise_psd(X, state=torch.zeros(7, 3, dtype=torch.float64), frame_major=False)
    with pytest.raises(ValueError):
        si.spectral_gain(X, state=torch.zeros(5, 3, dtype=torch.float64), frame_major=True)      # F is 7 there
    with pytest.raises(NotImplementedError):
        si.noise_psd(torch.zeros(5, 7, requires_grad=True))
    with pytest.raises(NotImplementedError):
        si.spectral_gain(X, noise=torch.ones(5, 1, requires_grad=True))
    with pytest.raises(NotImplementedError):
        si.spectral_gain(X, state=torch.zeros(5, 3, dtype=torch.float64, requires_grad=True))
    with pytest.raises(TypeError):
        si.denoise([0.0] * 4000, 512)
    with pytest.raises(ValueError):
        si.denoise(torch.zeros(4000), 512, gamma=0.0)
    with pytest.raises(ValueError):
        si.denoise(torch.zeros(4000), 512, n_iter=-1)
    with pytest.raises(NotImplementedError):
        si.denoise(torch.zeros(4000, requires_grad=True), 512)


def test_empty_batch_needs_no_gpu():
    X = torch.zeros(0, 5, 7, dtype=torch.complex64)
    G, xi, sig, Y, st = si.spectral_gain(X, return_snr=True, return_noise=True, return_enhanced=True, return_state=True)
    assert G.shape == X.shape and G.dtype == torch.float32 and Y.dtype == torch.complex64 and st.shape == (0, 5, 3)
    assert st.dtype == torch.float64 and xi.shape == X.shape and sig.shape == X.shape
    assert si.noise_psd(X.to(torch.complex128)).dtype == torch.float64


def test_entry_argument_errors_do_not_need_a_gpu():
    """specinv_enhance's checks, in the header's order, on pointers that are never read"""
    from spectrogram_inversion_amd import _lib, build
    build.build_lib()
    lib = _lib.load()
    p = [0x1000 * (i + 1) for i in range(9)]       # spec, noise, state_in, noise_out, spp_out, gain_out, snr_out, enhanced_out, state_out

    def call(ptrs, batch=1, n_freq=5, n_frames=7, init_frames=5, mode=_lib.ENHANCE_TRACK, rule=1, a_pow=0.8, a_spp=0.9, prior=31.6,
             alpha=0.98, xi_min=3e-3, g_min=0.1, dtype=_lib.F32):
        return lib.specinv_enhance(*ptrs, batch, n_freq, n_frames, init_frames, mode, rule, a_pow, a_spp, prior, alpha, xi_min, g_min, 1,
                                   0, dtype, 0, None)

    track = [p[0], None, None, p[3], p[4], p[5], p[6], p[7], p[8]]
    given = [p[0], p[1], p[2], None, None, p[5], p[6], p[7], p[8]]
    assert call([None] + track[1:]) == _lib.EINVAL and b"NULL spec" in lib.specinv_last_error()
    assert call([p[0]] + [None] * 8) == _lib.EINVAL and b"every output" in lib.specinv_last_error()
    assert call(track, mode=3) == _lib.EINVAL
    assert call(track, mode=_lib.ENHANCE_NOISE_FULL) == _lib.EINVAL
    assert call(given, mode=_lib.ENHANCE_TRACK) == _lib.EINVAL
    assert call(given[:3] + [p[3]] + given[4:], mode=_lib.ENHANCE_NOISE_PROFILE) == _lib.EINVAL
    assert b"noise_out and spp_out must be NULL" in lib.specinv_last_error()
    assert call(track[:5] + [p[0]] + track[6:]) == _lib.EINVAL and b"gain_out must not alias spec" in lib.specinv_last_error()
    assert call(track[:8] + [p[5]]) == _lib.EINVAL and b"state_out must not alias gain_out" in lib.specinv_last_error()
    for kw in ({"batch": 0}, {"n_freq": 0}, {"n_frames": 0}, {"batch": 1 << 40, "n_freq": 1 << 20}, {"init_frames": 0}, {"dtype": 7},
               {"rule": 2}, {"a_pow": 1.5}, {"a_spp": -0.1}, {"alpha": float("nan")}, {"prior": 0.0}, {"xi_min": float("inf")},
               {"g_min": 0.0}, {"g_min": 1.5}):
        assert call(track, **kw) == _lib.EINVAL, kw
        assert call(given, mode=_lib.ENHANCE_NOISE_FULL, **kw) == _lib.EINVAL, kw
