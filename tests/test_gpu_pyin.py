"""pyin, pyin_observations and pyin_decode on the device, against the float64 definition (tests/_pyin_oracle.py).

Four configurations, each on the four items of `_yin_oracle.signals` (a vibrato voice, a decaying glide with a hole, noise, silence;
33 or 17 frames):

    frame / hop   sample_rate   fmin ... fmax   resolution     P   width   covers
    256 / 64         8000        80 ... 500        0.1        318     31   the smallest frame
    512 / 128       16000        65 ... 2000       0.1        594     31   2 P = 1188 states, more than 1024 lanes
    256 / 64         8000        80 ... 500        0.5         64      7   P a single wave; bins collide on the noise item
    512 / 256        8000        40 ... 1000       0.1        558    141   a band wider than a wave

Observation stage.  The oracle is fed the kernel's own `yin_cmnd` output, so every comparison that decides structure - troughs,
thresholds, ranks, the arg-min - is exact: the set of non-zero bins must be identical, and the values and voiced_prob within rtol
2.4e-7, two float32 roundings (the sums are float64 on both sides; only the final rounding can differ).  A p below float32's
smallest normal number (a far candidate of the noise item: w_k e^(-2 r) reaches 1e-41) is rounded on the subnormal grid, whose
step is absolute: there the same two roundings are 2 x 2^-149, and "non-zero" means non-zero as a float32.  The one inexact decision
is the rounding of a bin, 12 bps log2(.), to an integer: a candidate whose unrounded bin is within 1e-9 of a half-integer
(`bin_margin`) could be excluded, and the cap on such exclusions is zero - the test asserts that the margin is at least 1e-9
instead.  On the CPU restatement of d' (`cmnd_f32`) the smallest margin of the four configurations is 7.4e-5, on the device's d'
2.1e-5.

Decode stage.  `pyin_decode` is fed the kernel's observations.  The oracle scores the returned path under the dense 2P x 2P model:
within 1e-9 relative of the dense optimum (about six orders above the float64 rounding of 3 T additions of magnitude <= 709, and
far below the cost of any wrong pointer); voiced_flag equal on every frame; states equal on every frame the oracle calls voiced.
Unvoiced frames are not compared bin by bin: their bins tie exactly by symmetry.  The margin by which the dense decode chose each
voiced state of its path (`path_gap`) is asserted to be at least 1e-6; on the CPU restatement the smallest is 0.17, items 1 / 2
decode 32 / 29 voiced frames of 33 at the first configuration, noise and silence none.
"""
import functools
import math

import numpy as np
import pytest
import torch

import _layouts
import _pyin_oracle as po
import _yin_oracle as yo
import spectrogram_inversion_amd as si

pytestmark = pytest.mark.gpu

DEV = "cuda"
RTOL = 2.4e-7
F32_TINY, F32_STEP = 2.0 ** -126, 2.0 ** -149               # float32's smallest normal number and its subnormal step
# (frame, hop, sample_rate, fmin, fmax, resolution, P, width)
CONFIGS = [(256, 64, 8000, 80.0, 500.0, 0.1, 318, 31),
           (512, 128, 16000, 65.0, 2000.0, 0.1, 594, 31),
           (256, 64, 8000, 80.0, 500.0, 0.5, 64, 7),
           (512, 256, 8000, 40.0, 1000.0, 0.1, 558, 141)]
IDS = ["256-64-0.1", "512-128-0.1", "256-64-0.5", "512-256-0.1"]


def _kw(c):
    n, hop, sr, fmin, fmax, res, _, _ = CONFIGS[c]
    return dict(sample_rate=sr, fmin=fmin, fmax=fmax, frame_length=n, hop_length=hop, resolution=res)


@functools.lru_cache(maxsize=None)
def _signals(c):
    n, _, sr = CONFIGS[c][:3]
    x = yo.signals(n, sr)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _device(c):
    """the kernels' (d', obs, voiced_prob, states of pyin_decode) as NumPy arrays - computed once per configuration"""
    n, hop, sr, fmin, fmax, res, n_pitch, width = CONFIGS[c]
    x = torch.tensor(_signals(c)).to(DEV)
    dp = si.yin_cmnd(x, n, hop)
    obs, vp = si.pyin_observations(x, **_kw(c))
    half, bps = po.transition_width(sr, hop, res)
    assert 2 * half + 1 == width and obs.shape == (4, dp.shape[1], n_pitch) == (4, dp.shape[1], si.pyin_bins(fmin, fmax, res))
    assert obs.dtype == vp.dtype == torch.float32 and vp.shape == obs.shape[:2]
    states = si.pyin_decode(obs, vp, half, bps)
    assert states.dtype == torch.int32 and states.shape == vp.shape and states.device == obs.device
    out = tuple(t.cpu().numpy() for t in (dp, obs, vp, states))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _reference(c):
    """the oracle on the kernel's d': per item (obs float64, voiced_prob float64, unrounded bins)"""
    n, hop, sr, fmin, fmax, res, _, _ = CONFIGS[c]
    dp = _device(c)[0]
    tau_min, tau_max = yo.lag_range(sr, fmin, fmax)
    return [po.observations(row, sr, fmin, fmax, tau_min, tau_max, po.prior(), resolution=res) for row in dp]


@functools.lru_cache(maxsize=None)
def _dense(c):
    """the dense decode of the kernel's observations: per item (states, score, path_gap)"""
    n, hop, sr, _, _, res, _, _ = CONFIGS[c]
    _, obs, vp, _ = _device(c)
    half, _ = po.transition_width(sr, hop, res)
    return [po.viterbi(o.astype(np.float64), v.astype(np.float64), half, 0.01, gaps=True) for o, v in zip(obs, vp)]


@pytest.mark.parametrize("c", range(4), ids=IDS)
def test_observation_stage(c):
    _, obs, vp, _ = _device(c)
    n_pitch = CONFIGS[c][6]
    lost = 0
    for item, (want, want_vp, raw) in enumerate(_reference(c)):
        margin = po.bin_margin(raw)
        lost += po.collisions(raw, n_pitch)
        want32 = want.astype(np.float32)
        normal = want >= F32_TINY
        err = np.abs(obs[item].astype(np.float64) - want)[normal] / want[normal]
        err_vp = np.abs(vp[item].astype(np.float64) - want_vp) / np.maximum(want_vp, 1e-300)
        print(f"{IDS[c]} item {item}: {int((want32 != 0).sum())} non-zero bins ({int((~normal & (want32 != 0)).sum())} subnormal), "
              f"at most {max(len(r) for r in raw)} candidates a frame, bin_margin {margin:.3g}, "
              f"obs rel {err.max() if err.size else 0.0:.3g}, voiced_prob rel {err_vp.max():.3g}, "
              f"voiced_prob {vp[item].min():.3g} ... {vp[item].max():.3g}")
        assert margin >= 1e-9
        assert np.array_equal(obs[item] != 0, want32 != 0)
        np.testing.assert_allclose(obs[item][normal], want[normal], rtol=RTOL, atol=0)
        assert np.abs(obs[item].astype(np.float64) - want)[~normal].max(initial=0.0) <= 2 * F32_STEP
        np.testing.assert_allclose(vp[item], want_vp, rtol=RTOL, atol=0)
        assert (vp[item] >= 0).all() and (vp[item] <= 1).all()
    print(f"{IDS[c]}: {lost} candidates lost their bin to a larger lag")
    assert not obs[3].any() and not vp[3].any()               # silence: no trough, no candidate
    assert vp[0].max() > 0.9 and vp[2].max() < 0.1            # the voice is voiced, the noise is not
    if c == 2:
        assert lost >= 1                                      # the collision rule was exercised


@pytest.mark.parametrize("c", range(4), ids=IDS)
def test_decode_stage(c):
    n, hop, sr, _, _, res, n_pitch, _ = CONFIGS[c]
    _, obs, vp, states = _device(c)
    half, _ = po.transition_width(sr, hop, res)
    for item, (want, best, gap) in enumerate(_dense(c)):
        got = states[item].astype(np.int64)
        assert got.min() >= 0 and got.max() < 2 * n_pitch
        voiced = want < n_pitch
        score = po.path_score(got, obs[item].astype(np.float64), vp[item].astype(np.float64), half, 0.01)
        low = float(gap[voiced].min()) if voiced.any() else math.inf
        print(f"{IDS[c]} item {item}: {int(voiced.sum())} voiced frames of {len(want)}, score {score:.6f} against {best:.6f} "
              f"(rel {abs(score - best) / abs(best):.3g}), smallest voiced path_gap {low:.3g}")
        assert low >= 1e-6
        assert abs(score - best) <= 1e-9 * abs(best)
        assert np.array_equal(got < n_pitch, voiced)
        assert np.array_equal(got[voiced], want[voiced])
    voiced = [int((d[0] < n_pitch).sum()) for d in _dense(c)]
    assert voiced[0] >= 0.9 * len(states[0]) and voiced[1] >= 0.75 * len(states[0]) and voiced[2] == voiced[3] == 0


def _same(got, want):
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape
        if a.dtype.is_floating_point:
            assert torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(-7.0), b.nan_to_num(-7.0))
        else:
            assert torch.equal(a, b)


@pytest.mark.parametrize("c", range(4), ids=IDS)
def test_pyin_is_the_composition_of_its_stages(c):
    n, hop, sr, fmin, fmax, res, n_pitch, _ = CONFIGS[c]
    _, obs, vp, states = _device(c)
    x = torch.tensor(_signals(c)).to(DEV)
    f0, voiced, prob, st = si.pyin(x, **_kw(c), return_states=True)
    assert (f0.dtype, voiced.dtype, prob.dtype, st.dtype) == (torch.float32, torch.bool, torch.float32, torch.int32)
    assert f0.shape == voiced.shape == prob.shape == st.shape == states.shape and f0.device == x.device
    assert np.array_equal(st.cpu().numpy(), states)
    assert np.array_equal(prob.cpu().numpy(), vp)
    assert np.array_equal(voiced.cpu().numpy(), states < n_pitch)
    bps = math.ceil(1 / res)
    want = (fmin * 2.0 ** ((states % n_pitch) / (12 * bps))).astype(np.float32)
    got = f0.cpu().numpy()
    assert np.isnan(got[states >= n_pitch]).all() and not np.isnan(got[states < n_pitch]).any()
    np.testing.assert_allclose(got[states < n_pitch], want[states < n_pitch], rtol=1.2e-7, atol=0)      # exp2 in torch, one rounding
    three = si.pyin(x, **_kw(c))
    assert len(three) == 3
    _same(three, (f0, voiced, prob))
    # fill_na lands on the unvoiced frames and nowhere else
    filled = si.pyin(x, **_kw(c), fill_na=-1.0)[0].cpu().numpy()
    assert (filled[states >= n_pitch] == -1.0).all() and np.array_equal(filled[states < n_pitch], got[states < n_pitch])
    # silence is unvoiced throughout, with nothing observed
    assert not voiced[3].any() and not prob[3].any()
    # the voice's track follows its vibrato: within a semitone of 110 Hz 2^(+-0.3) at every voiced frame
    v = got[0][states[0] < n_pitch]
    assert (v > 110 * 2 ** -0.4).all() and (v < 110 * 2 ** 0.4).all()


@pytest.mark.parametrize("name", ("strided", "offset"))
def test_layouts_give_the_dense_result_bit_for_bit(name):
    c = 0
    z = torch.tensor(_signals(c)[:3, :1001]).to(DEV).contiguous()
    want = si.pyin(z, **_kw(c), return_states=True) + si.pyin_observations(z, **_kw(c))
    view, base = _layouts.build(name, z)
    before = base.clone()
    _same(si.pyin(view, **_kw(c), return_states=True) + si.pyin_observations(view, **_kw(c)), want)
    assert torch.equal(base, before)


def test_single_items_cpu_tensors_and_dtypes():
    c = 0
    z = torch.tensor(_signals(c)[:3, :1001]).to(DEV).contiguous()
    want = si.pyin(z, **_kw(c), return_states=True)
    one = si.pyin(z[1], **_kw(c), return_states=True)                                       # (L,) gives (T,)
    _same(one, tuple(w[1] for w in want))
    host = si.pyin(z.cpu(), **_kw(c), return_states=True)                                   # a CPU tensor comes back to the CPU
    assert all(t.device.type == "cpu" for t in host)
    _same(host, tuple(w.cpu() for w in want))
    obs, vp = si.pyin_observations(z, **_kw(c))
    obs1, vp1 = si.pyin_observations(z[1].cpu(), **_kw(c))
    assert obs1.device.type == "cpu" and torch.equal(obs1, obs[1].cpu()) and torch.equal(vp1, vp[1].cpu())
    half, bps = po.transition_width(CONFIGS[c][2], CONFIGS[c][1], CONFIGS[c][5])
    assert torch.equal(si.pyin_decode(obs1, vp1, half, bps), want[3][1].cpu())              # (T, P) gives (T,)
    assert torch.equal(si.pyin_decode(obs.transpose(1, 2).contiguous().transpose(1, 2), vp, half, bps), want[3])
    # float16 / bfloat16 are computed in float32
    for dt in (torch.float16, torch.bfloat16):
        _same(si.pyin(z.to(dt), **_kw(c), return_states=True), si.pyin(z.to(dt).float(), **_kw(c), return_states=True))


def test_no_items_one_frame_and_the_given_prior():
    c = 0
    kw = _kw(c)
    f0, voiced, prob = si.pyin(torch.zeros(0, 500, device=DEV), **kw)
    assert f0.shape == voiced.shape == prob.shape == (0, 1 + 500 // 64) and f0.device.type == "cuda"
    # L < hop: a single frame, no transition at all
    x = torch.tensor(_signals(c)[:2, 300:340]).to(DEV)
    f0, voiced, prob, st = si.pyin(x, **kw, return_states=True)
    assert st.shape == (2, 1) and (st >= 0).all() and (st < 2 * 318).all()
    # threshold_prior equal to the default gives the default's bits
    z = torch.tensor(_signals(c)).to(DEV)
    want = si.pyin(z, **kw, return_states=True)
    for prior in (po.prior(), torch.tensor(po.prior()), list(po.prior())):
        _same(si.pyin(z, **kw, threshold_prior=prior, return_states=True), want)
    _same(si.pyin(z, **kw, beta_parameters=(2.5, 1), threshold_prior=po.prior(), return_states=True), want)
    # another prior is another result: all the weight on the lowest threshold leaves the glide's frames without a candidate below it
    low = np.zeros(100)
    low[0] = 1.0
    assert not torch.equal(si.pyin(z, **kw, threshold_prior=low)[2], want[2])


def test_the_limits_raise():
    x = torch.zeros(2, 4096, device=DEV)
    with pytest.raises(NotImplementedError, match="1024"):
        si.pyin(x, 16000, 20, 4000, resolution=0.05)
    with pytest.raises(NotImplementedError, match="1025"):
        si.pyin(x, 16000, 65, 2000, max_transition_rate=2000.0)
    with pytest.raises(ValueError, match="1024"):
        si.pyin(x, 16000, 65, 2000, n_thresholds=1025)
    with pytest.raises(NotImplementedError, match="float32"):
        si.pyin(x.double(), 16000, 65, 2000)
    with pytest.raises(NotImplementedError, match="513|1025"):
        si.pyin_decode(torch.zeros(1, 4, 40, device=DEV), torch.zeros(1, 4, device=DEV), 513, 10)


def test_the_caps_run():
    """P = 1024 bins and a band of 1025: sixteen waves, the largest LDS footprint; a track with jumps and a pause"""
    n_pitch, half, n_frames = 1024, 512, 8
    obs = np.zeros((1, n_frames, n_pitch), dtype=np.float32)
    for t, b in ((0, 0), (1, 3), (2, 1023), (3, 1020), (6, 500), (7, 501)):
        obs[0, t, b] = 0.9
    vp = obs.sum(axis=-1)
    got = si.pyin_decode(torch.tensor(obs).to(DEV), torch.tensor(vp).to(DEV), half, 10).cpu().numpy()[0].astype(np.int64)
    want, best, gap = po.viterbi(obs[0].astype(np.float64), vp[0].astype(np.float64), half, 0.01, gaps=True)
    voiced = want < n_pitch
    print(f"dense path {want.tolist()}, kernel {got.tolist()}, smallest voiced path_gap {gap[voiced].min():.3g}")
    assert voiced.sum() >= 4 and gap[voiced].min() >= 1e-6
    assert abs(po.path_score(got, obs[0].astype(np.float64), vp[0].astype(np.float64), half, 0.01) - best) <= 1e-9 * abs(best)
    assert np.array_equal(got < n_pitch, voiced) and np.array_equal(got[voiced], want[voiced])
