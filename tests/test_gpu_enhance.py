"""noise_psd, spectral_gain and denoise on the device, against the float64 definition (tests/_enhance_oracle.py).

Tolerances.  A float32 output is held to |out - oracle| <= 2^-23 |oracle| against the unrounded float64 oracle value: one rounding
of the output (2^-24) plus the chain's error, at most 10 s 1e-13 = 1e-10 with the conditioning s <= 100 that
tests/test_enhance_host.py asserts (it measures 24).  A float64 output, and the float64 state of either dtype, is held to the
relative bound 10 s (E1's stated bound) = 10 x 100 x 1e-13 = 1e-10.  No element is excluded: the host test asserts that on every
input used here (tests/_enhance_inputs.py) the oracle's Pbar stays 1e-9 away from 0.99, so the definition's one branch cannot flip.

Shapes.  F in {1, 63, 65, 257} (below, around and beyond the 64 chains of a workgroup), T in {1, 3 (below init_frames), tile - 1,
tile, tile + 1, 2 tile + 5} with tile = enhance._TILE_FRAMES, B in {1, 3}; both layouts, both rules; complex64, real float32 and
complex128.  One shape beyond 4096 workgroups of chains takes the looped grid.  The oracle runs once per (T, kind, rule) over the
chains of all shapes together and is shared."""
import itertools

import numpy as np
import pytest
import torch

import _enhance_inputs as ei
import _enhance_oracle as eo
import spectrogram_inversion_amd as si
from spectrogram_inversion_amd import enhance

pytestmark = pytest.mark.gpu

DEV = "cuda"
TILE = enhance._TILE_FRAMES
TOL32 = 2.0 ** -23
TOL64 = 10 * 100 * 1e-13
RULES = ("wiener", "lsa")


def _to_dev(a, frame_major):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t.transpose(-1, -2).contiguous() if frame_major else t


def _to_np(t, frame_major):
    return (t.transpose(-1, -2) if frame_major else t).cpu().numpy()


def _close(got, want, tol, what):
    got = np.asarray(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), what
    err = np.abs(got.astype(np.float64) - want)
    bad = err > tol * np.abs(want)
    assert not bad.any(), (what, int(bad.sum()), float((err / np.maximum(np.abs(want), 1e-300)).max()))


def _close_c(got, want, tol, what):
    if np.iscomplexobj(want):
        _close(got.real, want.real, tol, what + " re")
        _close(got.imag, want.imag, tol, what + " im")
    else:
        _close(got, want, tol, what)


def _tol(kind):
    return TOL64 if kind == "complex128" else TOL32


def test_tile_constant():
    assert ei.TILE == TILE


@pytest.mark.parametrize("frame_major", (False, True), ids=("bin-major", "frame-major"))
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("kind", ei.KINDS)
def test_gain_grid_against_oracle(kind, rule, frame_major):
    tol = _tol(kind)
    for (B, F, T) in ei.grid_shapes(TILE):
        want = ei.grid_oracle(T, kind, rule)[(B, F)]
        spec = ei.make_spec(B, F, T, kind)
        G, xi, sig, Y, st = si.spectral_gain(_to_dev(spec, frame_major), rule=rule, return_snr=True, return_noise=True,
                                             return_enhanced=True, return_state=True, frame_major=frame_major)
        what = f"{(B, F, T)}"
        assert G.dtype == (torch.float64 if kind == "complex128" else torch.float32) and Y.dtype == _to_dev(spec, False).dtype
        assert st.dtype == torch.float64 and st.shape == (B, F, 3)
        _close(_to_np(G, frame_major), want["gain"], tol, what + " G")
        _close(_to_np(xi, frame_major), want["snr"], tol, what + " xi")
        _close(_to_np(sig, frame_major), want["noise"], tol, what + " sigma2")
        _close_c(_to_np(Y, frame_major), want["gain"] * spec.astype(np.complex128 if np.iscomplexobj(spec) else np.float64), tol,
                 what + " G X")
        _close(st.cpu().numpy(), want["state"], TOL64, what + " state")


@pytest.mark.parametrize("frame_major", (False, True), ids=("bin-major", "frame-major"))
@pytest.mark.parametrize("kind", ei.KINDS)
def test_noise_psd_grid_against_oracle(kind, frame_major):
    tol = _tol(kind)
    for (B, F, T) in ei.grid_shapes(TILE):
        want = ei.grid_oracle(T, kind, "wiener")[(B, F)]
        spec = ei.make_spec(B, F, T, kind)
        sig, spp, st = si.noise_psd(_to_dev(spec, frame_major), return_spp=True, return_state=True, frame_major=frame_major)
        what = f"{(B, F, T)}"
        _close(_to_np(sig, frame_major), want["noise"], tol, what + " sigma2")
        _close(_to_np(spp, frame_major), want["spp"], tol, what + " p")
        _close(st.cpu().numpy()[..., :2], want["state"][..., :2], TOL64, what + " state")
    # a 2-D input is one item
    spec = ei.make_spec(1, 63, TILE + 1, kind)
    a = si.noise_psd(_to_dev(spec[0], frame_major), frame_major=frame_major)
    b = si.noise_psd(_to_dev(spec, frame_major), frame_major=frame_major)
    assert a.dim() == 2 and torch.equal(a, b[0])


@pytest.mark.parametrize("frame_major", (False, True), ids=("bin-major", "frame-major"))
def test_looped_grid(frame_major):
    spec = ei.named("looped")                                    # more groups of chains than a launch has workgroups
    want = eo.enhance(eo.power(spec), rule="wiener")
    G, sig = si.spectral_gain(_to_dev(spec, frame_major), rule="wiener", return_noise=True, frame_major=frame_major)
    _close(_to_np(G, frame_major), want["gain"], TOL32, "G")
    _close(_to_np(sig, frame_major), want["noise"], TOL32, "sigma2")


@pytest.mark.parametrize("frame_major", (False, True), ids=("bin-major", "frame-major"))
def test_every_nullable_output_on_and_off(frame_major):
    x = _to_dev(ei.named("nullable"), frame_major)
    names = ("return_snr", "return_noise", "return_enhanced", "return_state")
    full = si.spectral_gain(x, frame_major=frame_major, **{n: True for n in names})
    for flags in itertools.product((False, True), repeat=4):
        got = si.spectral_gain(x, frame_major=frame_major, **dict(zip(names, flags)))
        got = got if isinstance(got, tuple) else (got,)
        ref = [full[0]] + [full[i + 1] for i, on in enumerate(flags) if on]
        assert len(got) == len(ref)
        for a, b in zip(got, ref):
            assert torch.equal(a, b), flags
    full = si.noise_psd(x, return_spp=True, return_state=True, frame_major=frame_major)
    assert torch.equal(si.noise_psd(x, frame_major=frame_major), full[0])
    a = si.noise_psd(x, return_spp=True, frame_major=frame_major)
    b = si.noise_psd(x, return_state=True, frame_major=frame_major)
    assert torch.equal(a[0], full[0]) and torch.equal(a[1], full[1]) and torch.equal(b[0], full[0]) and torch.equal(b[1], full[2])
    # the tracker is the same launch in both entry points
    assert torch.equal(si.spectral_gain(x, return_noise=True, frame_major=frame_major)[1], full[0])


@pytest.mark.parametrize("frame_major", (False, True), ids=("bin-major", "frame-major"))
@pytest.mark.parametrize("rule", RULES)
def test_given_noise_bypasses_the_tracker(rule, frame_major):
    spec = ei.named("halves")
    B, F, T = spec.shape
    rng = np.random.default_rng(5)
    P = eo.power(spec)
    x = _to_dev(spec, frame_major)
    full = (P.mean() * 10.0 ** rng.uniform(-1, 1, size=(B, F, T))).astype(np.float32)
    profile = (P.mean() * 10.0 ** rng.uniform(-1, 1, size=(F, 1))).astype(np.float32)
    scalar = np.float32(P.mean())
    for noise, shaped in ((full, _to_dev(full, frame_major)),
                          (profile, torch.from_numpy(profile.T.copy() if frame_major else profile).to(DEV)),
                          (scalar, torch.tensor(float(scalar), device=DEV))):
        want = eo.enhance(P, noise=noise, rule=rule)
        G, xi, sig, st = si.spectral_gain(x, noise=shaped, rule=rule, return_snr=True, return_noise=True, return_state=True,
                                          frame_major=frame_major)
        _close(_to_np(G, frame_major), want["gain"], TOL32, "G")
        _close(_to_np(xi, frame_major), want["snr"], TOL32, "xi")
        assert np.array_equal(_to_np(sig, frame_major), np.broadcast_to(noise, P.shape))
        _close(st.cpu().numpy(), want["state"], TOL64, "state")
        other = si.spectral_gain(x, noise=shaped, rule=rule, return_snr=True, frame_major=frame_major, init_frames=1, alpha_pow=0.1,
                                 alpha_spp=0.2, prior_snr_db=3.0)
        assert torch.equal(other[0], G) and torch.equal(other[1], xi)


@pytest.mark.parametrize("dtype", (np.float64, np.float32))
def test_e1_grid(dtype):
    """w g on 200 log-spaced points of [1e-12, 1e3] in one frame: alpha = 1 makes xi the state's A^2 / sigma^2, a given noise of 1
    and P = 2000 make g = 2000, and floors of -400 dB keep the gain's clamps out of the way."""
    v = np.logspace(-12, 3, 200)
    m = np.full((200, 1), np.sqrt(2000.0)).astype(dtype)
    P = eo.power(m)
    w = v / P[:, 0]
    state = np.stack([np.ones(200), np.zeros(200), w / (1.0 - w)], axis=-1)
    kw = dict(alpha=1.0, xi_min_db=-400.0, gain_floor_db=-400.0, rule="lsa")
    want = eo.enhance(P, noise=np.float64(1.0), state=state, **kw)
    wg = want["snr"] / (1.0 + want["snr"]) * P
    assert wg.min() < 1.1e-12 and wg.max() > 900 and ((wg > 0.5) & (wg < 2)).sum() >= 5
    G = si.spectral_gain(torch.from_numpy(m).to(DEV), noise=torch.ones((), device=DEV), state=torch.from_numpy(state).to(DEV), **kw)
    err = np.abs(G.cpu().numpy().astype(np.float64) / want["gain"] - 1.0).max()
    print(f"E1 grid, {np.dtype(dtype).name}: G within {err:.2e} of the oracle")
    _close(G.cpu().numpy(), want["gain"], TOL64 if dtype == np.float64 else TOL32, "G")
    assert (want["gain"] < 1.0).all() and (want["gain"] > 1e-19).all()


@pytest.mark.parametrize("frame_major", (False, True), ids=("bin-major", "frame-major"))
@pytest.mark.parametrize("rule", RULES)
def test_chunked_equals_one_shot_bit_for_bit(rule, frame_major):
    x = _to_dev(ei.named("chunks"), frame_major)                 # 2 tile + 5 frames
    names = dict(return_snr=True, return_noise=True, return_enhanced=True, return_state=True, frame_major=frame_major, rule=rule)
    one = si.spectral_gain(x, **names)
    t_dim = 1 if frame_major else 2
    for cut in (5, TILE - 1, TILE, TILE + 1, 2 * TILE):
        a = si.spectral_gain(x.narrow(t_dim, 0, cut), **names)
        b = si.spectral_gain(x.narrow(t_dim, cut, x.shape[t_dim] - cut), state=a[4], **names)
        for i in range(4):
            assert torch.equal(torch.cat([a[i], b[i]], dim=t_dim), one[i]), (cut, i)
        assert torch.equal(b[4], one[4]), cut
    sa = si.noise_psd(x.narrow(t_dim, 0, TILE), return_spp=True, return_state=True, frame_major=frame_major)
    sb = si.noise_psd(x.narrow(t_dim, TILE, TILE + 5), state=sa[2], return_spp=True, return_state=True, frame_major=frame_major)
    so = si.noise_psd(x, return_spp=True, return_state=True, frame_major=frame_major)
    assert torch.equal(torch.cat([sa[0], sb[0]], dim=t_dim), so[0]) and torch.equal(torch.cat([sa[1], sb[1]], dim=t_dim), so[1])
    assert torch.equal(sb[2], so[2])


@pytest.mark.parametrize("kind", ("complex64", "float32", "complex128"))
@pytest.mark.parametrize("rule", RULES)
def test_frame_major_equals_the_transposed_call_bit_for_bit(rule, kind):
    B, F, T, _, seed = ei.NAMED["layout"]
    x = torch.from_numpy(ei.make_spec(B, F, T, kind, seed)).to(DEV)
    names = dict(return_snr=True, return_noise=True, return_enhanced=True, return_state=True, rule=rule)
    a = si.spectral_gain(x, **names)
    b = si.spectral_gain(x.transpose(1, 2).contiguous(), frame_major=True, **names)
    for i in range(4):
        assert torch.equal(a[i], b[i].transpose(1, 2)), i
    assert torch.equal(a[4], b[4])
    p = si.noise_psd(x, return_spp=True)
    q = si.noise_psd(x.transpose(1, 2).contiguous(), return_spp=True, frame_major=True)
    assert torch.equal(p[0], q[0].transpose(1, 2)) and torch.equal(p[1], q[1].transpose(1, 2))


def test_strided_and_conjugated_inputs_equal_the_dense_call():
    x = torch.from_numpy(ei.named("strided")).to(DEV)
    names = dict(return_snr=True, return_enhanced=True)
    dense = si.spectral_gain(x, **names)
    wide = torch.zeros(x.shape[0], x.shape[1], 2 * x.shape[2] + 1, dtype=x.dtype, device=DEV)
    wide[:, :, 1::2] = x
    strided = wide[:, :, 1::2]
    assert not strided.is_contiguous()
    got = si.spectral_gain(strided, **names)
    for a, b in zip(got, dense):
        assert torch.equal(a, b)
    lazy = x.conj().clone().conj()                               # the same values behind the conjugate bit
    assert lazy.is_conj()
    got = si.spectral_gain(lazy, **names)
    for a, b in zip(got, dense):
        assert torch.equal(a, b)
    # a view that is the frame-major array
    got = si.spectral_gain(x.transpose(1, 2), frame_major=True, **names)
    for a, b in zip(got, dense):
        assert torch.equal(a.transpose(1, 2), b)


@pytest.mark.parametrize("rule", RULES)
def test_zero_and_tiny_items_beside_a_normal_one(rule):
    x = torch.from_numpy(ei.named("batch")).to(DEV)              # (1, F, T)
    batch = torch.cat([torch.zeros_like(x), x, x * 1e-30], dim=0)
    names = dict(return_snr=True, return_noise=True, return_enhanced=True, return_state=True, rule=rule)
    alone = si.spectral_gain(x, **names)
    got = si.spectral_gain(batch, **names)
    g_min = 10.0 ** (-20.0 / 20.0)
    for a, b in zip(got, alone):
        assert torch.isfinite(torch.view_as_real(a) if a.is_complex() else a).all()
        assert torch.equal(a[1:2], b)
    assert (got[0] >= np.float32(g_min)).all() and (got[0] <= 1).all()
    assert (got[2][0] == 0).all() and (got[3][0] == 0).all()
    sig, spp = si.noise_psd(batch, return_spp=True)
    assert torch.isfinite(sig).all() and torch.isfinite(spp).all() and torch.equal(sig, got[2])


@pytest.mark.parametrize("consistent", (False, True))
def test_denoise_is_the_composition_of_the_public_calls(consistent):
    rng = np.random.default_rng(21)
    t = np.arange(6000) / 16000.0
    x = np.stack([np.sin(2 * np.pi * 440.0 * t) * (t > 0.1), np.sin(2 * np.pi * 300.0 * t * (1 + t)) * (t > 0.15)])
    x = torch.from_numpy((x + 0.3 * rng.standard_normal(x.shape)).astype(np.float32)).to(DEV)
    kw = dict(hop_length=128, window=torch.hann_window(512, periodic=True, device=DEV))
    for rule in RULES:
        y = si.denoise(x, 512, rule=rule, consistent=consistent, n_iter=4, gain_floor_db=-15.0, **kw)
        X = si.stft(x, 512, **kw)
        if consistent:
            G, xi, sig = si.spectral_gain(X, rule=rule, gain_floor_db=-15.0, return_snr=True, return_noise=True)
            want = si.istft(si.consistent_wiener(X, xi * sig, sig, gamma=1.0, n_iter=4, **kw)[0], **kw)
        else:
            want = si.istft(si.spectral_gain(X, rule=rule, gain_floor_db=-15.0) * X, **kw)
        assert y.shape == want.shape and y.dtype == torch.float32 and torch.isfinite(y).all()
        assert torch.equal(y, want)
    one = si.denoise(x[0], 512, **kw)
    assert one.dim() == 1


def test_cpu_and_half_inputs_round_trip():
    spec = ei.named("batch")
    x = torch.from_numpy(spec)
    ref = si.spectral_gain(x.to(DEV), return_noise=True, return_state=True)
    got = si.spectral_gain(x, return_noise=True, return_state=True)
    for a, b in zip(got, ref):
        assert a.device.type == "cpu" and torch.equal(a, b.cpu())
    m = x.abs().to(torch.float16)
    G, Y = si.spectral_gain(m.to(DEV), return_enhanced=True)
    G32, Y32 = si.spectral_gain(m.to(DEV).float(), return_enhanced=True)
    assert G.dtype == torch.float16 and Y.dtype == torch.float16
    assert torch.equal(G, G32.to(torch.float16)) and torch.equal(Y, Y32.to(torch.float16))
