"""pYIN without a GPU: the oracle against itself (tests/_pyin_oracle.py: the prior, the Boltzmann weights, the banded restatement of
the decode against the dense one, librosa's clipping / dropping / collision rules on hand-made d' rows), and the argument checks of
`pyin`, `pyin_observations`, `pyin_decode` and `pyin_bins`, which come before the device is touched."""
import math

import numpy as np
import pytest
import torch

import _pyin_oracle as po
import _yin_oracle as yo
import spectrogram_inversion_amd as si
from spectrogram_inversion_amd import pitch


def test_prior_sums_to_one_and_is_positive():
    for k_thr, a, b in ((100, 2, 18), (7, 1, 1), (1024, 3, 5)):
        w = po.prior(k_thr, a, b)
        assert w.shape == (k_thr,) and (w > 0).all()
        assert abs(w.sum() - 1.0) < 1e-14
        # the two halves of the binomial sum are one distribution
        for x in (0.0, 0.013, 0.4, 1.0):
            assert abs(po.beta_cdf(x, a, b) + po.beta_tail(x, a, b) - 1.0) < 1e-14
    assert np.array_equal(po.prior(), np.array(pitch._integer_prior(100, 2, 18)))


def test_prior_matches_scipy():
    stats = pytest.importorskip("scipy.stats")
    for k_thr, a, b in ((100, 2, 18), (50, 3, 5)):
        ref = np.diff(stats.beta.cdf(np.linspace(0, 1, k_thr + 1), a, b))
        # (scipy's cdf is good to a few units in the last place of values up to 1, and ref is a difference of two of them)
        assert np.abs(po.prior(k_thr, a, b) - ref).max() < 1e-14


def test_boltzmann_weights_of_a_threshold_sum_to_one():
    for lam in (0.5, 2.0, 7.0):
        boltz, inv = po.boltzmann(lam, 40)
        for n in (1, 2, 5, 40):
            assert abs(boltz[:n].sum() * inv[n] - 1.0) < 1e-14


def test_package_tables_are_the_oracles():
    w = tuple(po.prior())
    tab = pitch._obs_tables.__wrapped__(w, 2.0, 9, "cpu").numpy()
    boltz, inv = po.boltzmann(2.0, 9)
    assert np.array_equal(tab[:100], np.arange(1, 101) / 100)
    assert np.array_equal(tab[100:200], po.prior())
    np.testing.assert_allclose(tab[200:301], np.concatenate([[0.0], np.cumsum(po.prior())]), rtol=1e-15, atol=0)
    np.testing.assert_allclose(tab[301:310], boltz, rtol=1e-15, atol=0)
    np.testing.assert_allclose(tab[310:], inv, rtol=1e-15, atol=0)
    for n_pitch, half in ((64, 3), (318, 15), (20, 30)):
        ltri, nlz = po.decode_tables(n_pitch, half)
        dec = pitch._decode_tables.__wrapped__(n_pitch, half, "cpu").numpy()
        np.testing.assert_allclose(dec[:half + 1], ltri, rtol=0, atol=1e-15)
        np.testing.assert_allclose(dec[half + 1:], nlz, rtol=0, atol=1e-14)
        # the folded Z is the row sum of the literal band
        width = 2 * half + 1
        j = np.arange(n_pitch)
        tri = np.where(np.abs(j[:, None] - j[None]) <= half, 1.0 - np.abs(j[:, None] - j[None]) / ((width + 1) / 2), 0.0)
        np.testing.assert_allclose(np.exp(-nlz), tri.sum(axis=1), rtol=1e-14)
        np.testing.assert_allclose(po.band(n_pitch, half).sum(axis=1), 1.0, rtol=1e-14)


def _row(w_lags, lows):
    """a d' row of w_lags + 1 lags that is 1 everywhere but for the troughs {lag: value}"""
    row = np.ones(w_lags + 1, dtype=np.float32)
    for lag, v in lows.items():
        row[lag] = v
    return row


def test_candidates_on_hand_made_rows():
    w = po.prior()
    cum = np.concatenate([[0.0], np.cumsum(w)])
    # one trough at 0.05: caught by the thresholds 0.06 ... 1, alone each time, and it is the arg-min with m = 5
    taus, p = po.candidates(_row(128, {40: 0.05}), 10, 100, w, 2.0, 0.01)
    assert taus.tolist() == [40]
    assert abs(p[0] - ((1.0 - cum[5]) + 0.01 * cum[5])) < 1e-15
    # two troughs: the shorter lag has rank 0 wherever both are caught
    taus, p = po.candidates(_row(128, {30: 0.5, 60: 0.2}), 10, 100, w, 2.0, 0.01)
    assert taus.tolist() == [30, 60]
    e2 = math.exp(-2.0)
    first = (1 - e2) / (1 - e2 * e2)
    want30 = (1.0 - cum[50]) * first
    want60 = (cum[50] - cum[20]) + (1.0 - cum[50]) * first * e2 + 0.01 * cum[20]
    np.testing.assert_allclose(p, [want30, want60], rtol=0, atol=1e-15)
    # the ends of the range use their real neighbours: a fall into tau_max from inside is a trough only if d'(tau_max + 1) is no lower
    row = _row(128, {100: 0.3, 101: 0.2})
    assert po.troughs(row, 10, 100).tolist() == []
    assert po.troughs(row, 10, 101).tolist() == [101]
    row = _row(128, {9: 0.2, 10: 0.3})
    assert po.troughs(row, 10, 100).tolist() == []           # d'(tau_min) is above its real left neighbour
    # equal neighbours: the first of a flat bottom is the trough
    assert po.troughs(_row(128, {50: 0.3, 51: 0.3}), 10, 100).tolist() == [50]
    # silence: no trough, no candidate, voiced_prob 0
    obs, vp, raw = po.observations(np.ones((2, 129), dtype=np.float32), 8000, 80, 500, 16, 100, w)
    assert not obs.any() and not vp.any() and po.bin_margin(raw) == math.inf


def test_clipping_dropping_and_collisions():
    w = po.prior()
    sr, fmin, fmax = 8000, 80.0, 500.0
    tau_min, tau_max = yo.lag_range(sr, fmin, fmax)           # 16 ... 100
    n_pitch = po.n_bins(fmin, fmax, 0.1)
    assert n_pitch == 318 == si.pyin_bins(fmin, fmax, 0.1)
    # lag 100 is exactly fmin: bin 0; lag 16 is exactly fmax = 500 Hz: bin rint(120 log2(6.25)) = 317 = P - 1
    obs, vp, raw = po.observations(np.stack([_row(128, {100: 0.1}), _row(128, {16: 0.1})]), sr, fmin, fmax, tau_min, tau_max, w)
    assert np.nonzero(obs[0])[0].tolist() == [0] and np.nonzero(obs[1])[0].tolist() == [317]
    assert abs(vp[0] - obs[0, 0]) < 1e-16
    # a wider lag range than the grid: a period above sr / fmin clips to bin 0, one below sr / fmax is dropped
    obs, vp, raw = po.observations(np.stack([_row(128, {110: 0.1}), _row(128, {12: 0.1})]), sr, fmin, fmax, 10, 120, w)
    assert np.nonzero(obs[0])[0].tolist() == [0] and not obs[1].any() and vp[1] == 0.0
    assert raw[0][0] < -0.5 and raw[1][0] > n_pitch - 0.5
    # two troughs in one bin at a coarse grid: the larger lag's value stands, and voiced_prob counts only what stands
    row = _row(128, {98: 0.3, 100: 0.2})                      # 12 log2(100 / 98) = 0.35 and 0: both bin 0
    taus, p = po.candidates(row, tau_min, tau_max, w)
    obs, vp, raw = po.observations(row[None], sr, fmin, fmax, tau_min, tau_max, w, resolution=1.0)
    assert np.rint(raw[0]).tolist() == [0.0, 0.0] and np.nonzero(obs[0])[0].tolist() == [0]
    assert obs[0, 0] == p[1] and vp[0] == p[1] and po.collisions(raw, po.n_bins(fmin, fmax, 1.0)) == 1
    assert 0 < po.bin_margin(raw) <= 0.5


@pytest.mark.parametrize("n_pitch,half,seed", [(24, 3, 0), (40, 0, 1), (33, 40, 2), (70, 9, 3)])
def test_banded_decode_is_the_dense_one(n_pitch, half, seed):
    """random sparse observations with voiced stretches, pauses and jumps wider than the band (the floor is then on the path)"""
    rng = np.random.default_rng(seed)
    n_frames = 40
    obs = np.zeros((n_frames, n_pitch))
    track = rng.integers(0, n_pitch)
    for t in range(n_frames):
        if t % 13 in (5, 6):
            continue                                          # a pause
        track = int(np.clip(track + rng.integers(-2, 3), 0, n_pitch - 1)) if t % 9 else int(rng.integers(0, n_pitch))
        obs[t, track] = rng.uniform(0.3, 0.9)
        obs[t, rng.integers(0, n_pitch)] += rng.uniform(0.0, 0.1)
    obs = obs.astype(np.float32).astype(np.float64)
    vp = np.clip(obs.sum(axis=-1), 0, 1).astype(np.float32).astype(np.float64)
    dense, score, gap = po.viterbi(obs, vp, half, 0.01, gaps=True)
    banded, score_b = po.viterbi_banded(obs, vp, half, 0.01)
    voiced = dense < n_pitch
    assert voiced.any() and not voiced.all()
    assert abs(score - score_b) <= 1e-12 * abs(score)
    assert abs(po.path_score(dense, obs, vp, half, 0.01) - score) <= 1e-12 * abs(score)
    assert abs(po.path_score(banded, obs, vp, half, 0.01) - score) <= 1e-12 * abs(score)
    assert np.array_equal(banded < n_pitch, voiced)
    assert np.array_equal(banded[voiced], dense[voiced])
    assert gap.shape == (n_frames,) and (gap >= 0).all()


def test_pyin_bins():
    assert si.pyin_bins(65, 2000, 0.1) == 594
    assert si.pyin_bins(80, 500, 0.5) == 64
    assert si.pyin_bins(40, 1000, 0.1) == 558
    assert si.pyin_bins(100, 200, 1) == 13
    assert si.pyin_bins(100, 200, 0.3) == math.floor(12 * 4 * 1.0) + 1
    for bad in ((0, 100, 0.1), (100, 100, 0.1), (100, 200, 0), (100, 200, 1.5), (100, float("inf"), 0.1), ("a", 200, 0.1)):
        with pytest.raises(ValueError):
            si.pyin_bins(*bad)


X = torch.zeros(2, 4096)


@pytest.mark.parametrize("kwargs,exc,word", [
    (dict(fmin=20, fmax=4000, resolution=0.05), NotImplementedError, "1024"),             # P = 1835
    (dict(fmin=65, fmax=2000, max_transition_rate=2000.0), NotImplementedError, "1025"),  # width 7681
    (dict(fmin=65, fmax=2000, resolution=1.0, max_transition_rate=2.7), NotImplementedError, "odd"),       # m = 1, bps = 1: width 2
    (dict(fmin=65, fmax=2000, n_thresholds=0), ValueError, "n_thresholds"),
    (dict(fmin=65, fmax=2000, n_thresholds=1025), ValueError, "1024"),
    (dict(fmin=65, fmax=2000, switch_prob=0.0), ValueError, "switch_prob"),
    (dict(fmin=65, fmax=2000, switch_prob=1.0), ValueError, "switch_prob"),
    (dict(fmin=65, fmax=2000, no_trough_prob=-0.1), ValueError, "no_trough_prob"),
    (dict(fmin=65, fmax=2000, no_trough_prob=1.1), ValueError, "no_trough_prob"),
    (dict(fmin=65, fmax=2000, boltzmann_parameter=0.0), ValueError, "boltzmann_parameter"),
    (dict(fmin=65, fmax=2000, resolution=0.0), ValueError, "resolution"),
    (dict(fmin=65, fmax=2000, resolution=1.01), ValueError, "resolution"),
    (dict(fmin=65, fmax=2000, beta_parameters=(2.5, 18)), NotImplementedError, "threshold_prior"),
    (dict(fmin=65, fmax=2000, beta_parameters=(0, 18)), ValueError, "beta_parameters"),
    (dict(fmin=65, fmax=2000, threshold_prior=[0.5, 0.5]), ValueError, "threshold_prior"),
    (dict(fmin=65, fmax=2000, max_transition_rate=-1.0), ValueError, "max_transition_rate"),
    (dict(fmin=65, fmax=2000, fill_na="x"), ValueError, "fill_na"),
    (dict(fmin=5, fmax=2000), ValueError, "fmin"),                                        # the lag range of yin
    (dict(fmin=65, fmax=2000, frame_length=300), NotImplementedError, "frame_length"),
    (dict(fmin=65, fmax=2000, hop_length=0), ValueError, "hop_length"),
])
def test_pyin_argument_errors_come_before_the_device(kwargs, exc, word):
    with pytest.raises(exc, match=word):
        si.pyin(X, 16000, **kwargs)


def test_pyin_input_errors():
    with pytest.raises(NotImplementedError, match="float32"):
        si.pyin(X.double(), 16000, 65, 2000)
    with pytest.raises(TypeError):
        si.pyin(X.long(), 16000, 65, 2000)
    with pytest.raises(TypeError):
        si.pyin(X.numpy(), 16000, 65, 2000)
    with pytest.raises(ValueError, match="shape"):
        si.pyin(X[None], 16000, 65, 2000)
    with pytest.raises(NotImplementedError, match="differentiable"):
        si.pyin(X.clone().requires_grad_(), 16000, 65, 2000)
    with pytest.raises(NotImplementedError, match="float32"):
        si.pyin_observations(X.double(), 16000, 65, 2000)
    with pytest.raises(NotImplementedError, match="1024"):
        si.pyin_observations(X, 16000, 20, 4000, resolution=0.05)
    # non-integer beta parameters are fine once the prior itself is given: the next check is reached
    with pytest.raises(ValueError, match="switch_prob"):
        si.pyin(X, 16000, 65, 2000, beta_parameters=(2.5, 18), threshold_prior=np.full(100, 0.01), switch_prob=2)


def test_no_items_need_no_device():
    f0, voiced, prob, states = si.pyin(torch.zeros(0, 4096), 16000, 65, 2000, frame_length=1024, return_states=True)
    assert f0.shape == voiced.shape == prob.shape == states.shape == (0, 17)
    assert (f0.dtype, voiced.dtype, prob.dtype, states.dtype) == (torch.float32, torch.bool, torch.float32, torch.int32)
    obs, vp = si.pyin_observations(torch.zeros(0, 4096), 16000, 65, 2000, frame_length=1024)
    assert obs.shape == (0, 17, 594) and vp.shape == (0, 17)
    assert si.pyin_decode(obs, vp, 15, 10).shape == (0, 17)


def test_pyin_decode_argument_errors():
    obs, vp = torch.zeros(2, 5, 30), torch.zeros(2, 5)
    for args, exc in (((obs.double(), vp, 3, 10), TypeError), ((obs, vp[:1], 3, 10), ValueError), ((obs[0, 0], vp[0, 0], 3, 10), ValueError),
                      ((obs, vp, -1, 10), ValueError), ((obs, vp, 1.5, 10), ValueError), ((obs, vp, 513, 10), NotImplementedError),
                      ((obs, vp, 3, 0), ValueError), ((torch.zeros(2, 5, 1025), vp, 3, 10), NotImplementedError),
                      ((torch.zeros(2, 0, 30), torch.zeros(2, 0), 3, 10), ValueError), ((obs.numpy(), vp, 3, 10), TypeError)):
        with pytest.raises(exc):
            si.pyin_decode(*args)
    with pytest.raises(ValueError, match="switch_prob"):
        si.pyin_decode(obs, vp, 3, 10, switch_prob=1.0)
    with pytest.raises(NotImplementedError, match="differentiable"):
        si.pyin_decode(obs.clone().requires_grad_(), vp, 3, 10)


def test_c_entries_check_their_arguments_without_a_device():
    import ctypes as C

    from spectrogram_inversion_amd import _lib, build
    build.build_lib()
    lib = _lib.load()
    p = [C.c_void_p(4096 * (i + 1)) for i in range(6)]       # never dereferenced: every call fails before the device
    obs = lambda **k: lib.specinv_pyin_obs(*[k.get(n, d) for n, d in (          # noqa: E731
        ("cmnd", p[0]), ("tables", p[1]), ("obs_out", p[2]), ("vprob_out", p[3]), ("frames", 4), ("frame", 256), ("tau_min", 16),
        ("tau_max", 100), ("n_thresholds", 100), ("n_ranks", 43), ("n_bins", 318), ("bps", 10), ("sample_rate", 8000.0),
        ("fmin", 80.0), ("q", 0.01), ("dtype", _lib.F32), ("device", 0), ("stream", None))])
    for kw, code, word in ((dict(cmnd=None), _lib.EINVAL, b"NULL cmnd"), (dict(vprob_out=p[2]), _lib.EINVAL, b"alias"),
                           (dict(frames=0), _lib.EINVAL, b"frames"), (dict(dtype=5), _lib.EINVAL, b"dtype"),
                           (dict(dtype=_lib.F64), _lib.EUNSUPPORTED, b"float32"), (dict(frame=384), _lib.EUNSUPPORTED, b"frame"),
                           (dict(n_bins=1025), _lib.EUNSUPPORTED, b"1024"), (dict(n_thresholds=1025), _lib.EUNSUPPORTED, b"1024"),
                           (dict(tau_max=128), _lib.EINVAL, b"tau_max"), (dict(n_ranks=42), _lib.EINVAL, b"n_ranks"),
                           (dict(bps=0), _lib.EINVAL, b"bins_per_semitone"), (dict(fmin=0.0), _lib.EINVAL, b"fmin"),
                           (dict(q=1.5), _lib.EINVAL, b"no_trough_prob")):
        assert obs(**kw) == code, kw
        assert word in lib.specinv_last_error(), (kw, lib.specinv_last_error())
    vit = lambda **k: lib.specinv_pyin_viterbi(*[k.get(n, d) for n, d in (      # noqa: E731
        ("obs", p[0]), ("vprob", p[1]), ("tables", p[2]), ("backptr", p[3]), ("states_out", p[4]), ("ticks_out", None), ("batch", 2),
        ("n_frames", 5), ("n_bins", 318), ("half", 15), ("switch", 0.01), ("dtype", _lib.F32), ("device", 0), ("stream", None))])
    for kw, code, word in ((dict(backptr=None), _lib.EINVAL, b"NULL backptr"), (dict(ticks_out=p[4]), _lib.EINVAL, b"alias"),
                           (dict(n_frames=0), _lib.EINVAL, b"n_frames"), (dict(dtype=_lib.F64), _lib.EUNSUPPORTED, b"float32"),
                           (dict(n_bins=1025), _lib.EUNSUPPORTED, b"1024"), (dict(half=513), _lib.EUNSUPPORTED, b"1025"),
                           (dict(switch=0.0), _lib.EINVAL, b"switch_prob")):
        assert vit(**kw) == code, kw
        assert word in lib.specinv_last_error(), (kw, lib.specinv_last_error())
