"""yin, yin_cmnd and pitch_shift(formant_order="f0") on the device, against the float64 definition (tests/_yin_oracle.py).

Shapes: frame lengths 256 ... 2048, each with the default hop N / 4 and with hop 100, centred and not, on the four signals of
`_yin_oracle.signals` (L = 8 N + 37: 33 centred frames at N / 4, a last workgroup that is not full), plus L = 5.

Tolerance for d'.  The yardstick is `cmnd_f32`, the kernel's arithmetic restated with NumPy on the CPU (complex64 FFT, float64
sums, the lags 1 ... 8 from the literal sum), against the float64 oracle over lags 0 ... W on the same inputs.  Its largest error
over the sixteen cases of a size, measured on the CPU, is YARD below; the kernel gets four times that for another FFT factorisation
and summation order.  Measured on the device, the kernel's largest error was 5.13e-6 / 2.50e-6 / 1.98e-6 / 6.65e-7 at N 256 / 512 /
1024 / 2048 - 2.50 / 1.17 / 1.06 / 1.32 yardsticks.  (With every lag through the FFT the yardstick was 4.28e-6 / 4.58e-6 / 4.57e-6 /
7.13e-6, nearly all of it at lags 2 ... 7, where c(tau) is a sum of a few small differences of large numbers.)

The pick is compared twice.  Against the oracle's `pick` and `refine` applied to the kernel's own float32 d' it must agree on every
frame, exactly (period: to one float32 ulp).  Against the float64 oracle it must agree on every frame whose `tie_margin` - the
smallest amount by which a comparison of the pick could flip - is at least ten d' tolerances (8.2e-5 / 8.5e-5 / 7.5e-5 / 2.0e-5), and
at most 2 frames per item may be set aside for a smaller margin; the float64 oracle alone decides which.  On these signals at most
1 frame per item is set aside in any of the sixteen cases, and no frame outside the margin disagrees with float64.

f0 on the voiced frames outside the margin: the same yardstick gave a relative error of 1.18e-7 / 1.06e-7 / 1.37e-7 / 1.64e-7
(F0_YARD, the rounding of f0 to float32 included); the kernel gets four times that and measured 0.53 ... 1.36 of it.
"""
import functools

import numpy as np
import pytest
import torch

import _layouts
import _yin_oracle as o
import spectrogram_inversion_amd as si

pytestmark = pytest.mark.gpu

DEV = "cuda"
SR, FMAX, THRESHOLD = o.SR, 1000.0, 0.1
SIZES = (256, 512, 1024, 2048)
# cmnd_f32 against the float64 oracle, the largest error over hop (N / 4, 100) x center x the four items, measured on the CPU
YARD = {256: 2.05e-6, 512: 2.13e-6, 1024: 1.87e-6, 2048: 5.03e-7}
TOL = {n: 4 * y for n, y in YARD.items()}                 # 8.20e-6, 8.52e-6, 7.48e-6, 2.01e-6
MARGIN = {n: 10 * t for n, t in TOL.items()}              # 8.20e-5, 8.52e-5, 7.48e-5, 2.01e-5
F0_YARD = {256: 1.18e-7, 512: 1.06e-7, 1024: 1.37e-7, 2048: 1.64e-7}
F0_TOL = {n: 4 * y for n, y in F0_YARD.items()}
CAP = 2                                                   # frames per item that may be set aside for a small tie margin

CASES = [(n, hop, center) for n in SIZES for hop in (n // 4, 100) for center in (True, False)]
IDS = [f"{n}-{hop}-{'centred' if center else 'plain'}" for n, hop, center in CASES]


def _fmin(n):
    return max(60.0, o.smallest_fmin(SR, n))


def _lags(n):
    return o.lag_range(SR, _fmin(n), FMAX)


@functools.lru_cache(maxsize=None)
def _signals(n):
    x = o.signals(n)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _reference(n, hop, center):
    """(d' float64 (4, T, W + 1), the yardstick's error) - computed once per case and left alone"""
    x = _signals(n)
    d64 = np.stack([o.cmnd(row, n, hop, center) for row in x])
    yard = max(float(np.abs(o.cmnd_f32(row, n, hop, center) - ref).max()) for row, ref in zip(x, d64))
    d64.setflags(write=False)
    return d64, yard


@functools.lru_cache(maxsize=None)
def _device(n, hop, center):
    """the kernel's (d', f0, voiced, aperiodicity, tau) as NumPy arrays"""
    x = torch.tensor(_signals(n)).to(DEV)
    dp = si.yin_cmnd(x, n, hop, center)
    f0, voiced, ap, tau = si.yin(x, SR, _fmin(n), FMAX, n, hop, THRESHOLD, center, return_tau=True)
    t = o.n_frames(x.shape[-1], n, hop, center)
    assert dp.shape == (4, t, n // 2 + 1) and dp.dtype == torch.float32 and dp.device == x.device
    assert f0.shape == voiced.shape == ap.shape == tau.shape == (4, t) == (4, si.yin_frames(x.shape[-1], n, hop, center))
    assert (f0.dtype, voiced.dtype, ap.dtype, tau.dtype) == (torch.float32, torch.bool, torch.float32, torch.int32)
    return tuple(a.cpu().numpy() for a in (dp, f0, voiced, ap, tau))


@pytest.mark.parametrize("n,hop,center", CASES, ids=IDS)
def test_cmnd_against_the_float64_oracle(n, hop, center):
    d64, yard = _reference(n, hop, center)
    dp = _device(n, hop, center)[0]
    assert yard <= 1.01 * YARD[n], (yard, YARD[n])               # the constants are this restatement's, not a stale one's
    assert np.isfinite(dp).all() and (dp[..., 0] == 1).all()
    err = [float(np.abs(a - b).max()) for a, b in zip(dp, d64)]
    print(f"N {n} hop {hop} center {center}: T {dp.shape[1]}, yardstick here {yard:.2e} (size {YARD[n]:.2e}), kernel "
          + " ".join(f"{e:.2e}" for e in err) + f" ({max(err) / YARD[n]:.2f} x)")
    assert max(err) <= TOL[n], (err, TOL[n])


@pytest.mark.parametrize("n,hop,center", CASES, ids=IDS)
def test_the_pick_is_exact_on_the_kernels_own_numbers(n, hop, center):
    dp, f0, voiced, ap, tau = _device(n, hop, center)
    tau_min, tau_max = _lags(n)
    for item in range(4):
        for t in range(dp.shape[1]):
            row = dp[item, t]
            want = o.pick(row, tau_min, tau_max, THRESHOLD)
            assert tau[item, t] == want, (item, t, tau[item, t], want)
            assert ap[item, t] == row[want]                                                  # bit for bit
            assert voiced[item, t] == (np.float64(ap[item, t]) < THRESHOLD)
            # period within one float32 ulp of the oracle's: f0 = float32(SR / float64(period)) is then one of three numbers
            period = np.float32(o.refine(row, want)[0])
            near = (np.nextafter(period, np.float32(0)), period, np.nextafter(period, np.float32(np.inf)))
            assert f0[item, t] in [np.float32(SR / np.float64(p)) for p in near], (item, t, f0[item, t], period)


@pytest.mark.parametrize("n,hop,center", CASES, ids=IDS)
def test_the_pick_against_float64(n, hop, center):
    d64, _ = _reference(n, hop, center)
    _, f0, voiced, _, tau = _device(n, hop, center)
    tau_min, tau_max = _lags(n)
    aside, worst = [], 0.0
    for item in range(4):
        want_f0, want_voiced, _, want_tau = o.yin(None, SR, _fmin(n), FMAX, n, hop, THRESHOLD, center, dp=d64[item])
        safe = np.array([o.tie_margin(row, tau_min, tau_max, THRESHOLD) for row in d64[item]]) >= MARGIN[n]
        assert (tau[item][safe] == want_tau[safe]).all() and (voiced[item][safe] == want_voiced[safe]).all(), (item, safe)
        sel = safe & want_voiced
        if sel.any():
            worst = max(worst, float(np.abs(f0[item][sel].astype(np.float64) / want_f0[sel] - 1).max()))
        aside.append(int((~safe).sum()))
    print(f"N {n} hop {hop} center {center}: frames set aside per item {aside} of {d64.shape[1]}, f0 relative error {worst:.2e} "
          f"({worst / F0_YARD[n]:.2f} x)")
    assert worst <= F0_TOL[n], (worst, F0_TOL[n])
    assert max(aside) <= CAP, aside


@pytest.mark.parametrize("n", SIZES)
def test_silence_is_exact(n):
    tau_min, _ = _lags(n)
    for hop, center in ((n // 4, True), (100, False)):
        dp, f0, voiced, ap, tau = _device(n, hop, center)
        assert (dp[3] == 1).all() and (tau[3] == tau_min).all() and not voiced[3].any() and (ap[3] == 1).all()
        assert (f0[3] == np.float32(SR / tau_min)).all()                                     # period = tau_min exactly
    # the frame of zeros inside item 2 is noise at 0.005, not silence; a silent item beside a loud one is the case above


@pytest.mark.parametrize("n", SIZES)
def test_a_power_of_two_scale_changes_nothing_in_the_pick(n):
    x = torch.tensor(_signals(n)).to(DEV)
    _, _, voiced, _, tau = _device(n, n // 4, True)
    f0s, vs, aps, taus = si.yin(x * 2.0 ** -10, SR, _fmin(n), FMAX, n, n // 4, THRESHOLD, True, return_tau=True)
    assert (taus.cpu().numpy() == tau).all() and (vs.cpu().numpy() == voiced).all()


def test_five_samples_are_one_frame_of_padding():
    x = torch.tensor([[0.3, -0.2, 0.5, 0.1, -0.4], [0.0, 0.0, 0.0, 0.0, 0.0]])
    for n in SIZES:
        tau_min, tau_max = _lags(n)
        dp = si.yin_cmnd(x.to(DEV), n).cpu().numpy()
        assert dp.shape == (2, 1, n // 2 + 1)
        ref = np.stack([o.cmnd(row, n, n // 4) for row in x.numpy()])
        assert np.abs(dp - ref).max() <= TOL[n] and (dp[1] == 1).all()
        f0, voiced, ap, tau = si.yin(x.to(DEV), SR, _fmin(n), FMAX, n, return_tau=True)
        assert tau[0, 0].item() == o.pick(dp[0, 0], tau_min, tau_max, THRESHOLD) and tau[1, 0].item() == tau_min
        assert f0.shape == (2, 1) and not voiced[1, 0].item()


def test_halves_are_computed_in_float32():
    x = torch.tensor(_signals(256)[:3])
    for dtype in (torch.float16, torch.bfloat16):
        h = x.to(dtype)
        got = si.yin(h.to(DEV), SR, _fmin(256), FMAX, 256, 100, return_tau=True)
        want = si.yin(h.float().to(DEV), SR, _fmin(256), FMAX, 256, 100, return_tau=True)
        assert got[0].dtype == torch.float32
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        assert torch.equal(si.yin_cmnd(h.to(DEV), 256, 100), si.yin_cmnd(h.float().to(DEV), 256, 100))


@pytest.mark.parametrize("name", ("strided", "step_last", "step_batch", "offset", "neg"))
def test_layouts_give_the_dense_result_bit_for_bit(name):
    Z = torch.tensor(_signals(256)[:3, :1001]).to(DEV).contiguous()
    args = (SR, _fmin(256), FMAX, 256, 100)
    want = si.yin(Z, *args, return_tau=True) + (si.yin_cmnd(Z, 256, 100),)
    view, base = _layouts.build(name, Z)
    before = base.clone()
    for arg in (view, _layouts.dense_twin(view, Z)):
        got = si.yin(arg, *args, return_tau=True) + (si.yin_cmnd(arg, 256, 100),)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
    assert torch.equal(base, before)
    one = si.yin(Z[1], *args, return_tau=True)                                               # (L,) gives (T,)
    for a, b in zip(one, want):
        assert a.shape == b.shape[1:] and torch.equal(a, b[1])


def test_more_items_than_one_call_is_given():
    """70 000 items of five samples are 70 000 workgroups of one frame: the wrapper hands the entry point at most 65 535"""
    seven = torch.randn(7, 5, generator=torch.Generator().manual_seed(5)).to(DEV)
    seven[3] = 0
    many = seven.repeat(10000, 1)
    want = si.yin(seven, SR, 63.0, FMAX, 256, return_tau=True) + (si.yin_cmnd(seven, 256),)
    got = si.yin(many, SR, 63.0, FMAX, 256, return_tau=True) + (si.yin_cmnd(many, 256),)
    for a, b in zip(got, want):
        assert a.shape[0] == 70000 and torch.equal(a, b.repeat((10000,) + (1,) * (b.dim() - 1)))


def test_another_stream_and_a_cpu_tensor():
    x = torch.tensor(_signals(512)[:2])
    args = (SR, 60.0, FMAX, 512, 100)
    want = si.yin(x.to(DEV), *args, return_tau=True)
    stream = torch.cuda.Stream()
    xg = x.to(DEV)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        got = si.yin(xg, *args, return_tau=True)
    stream.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    home = si.yin(x, *args, return_tau=True) + (si.yin_cmnd(x, 512, 100),)
    assert all(a.device.type == "cpu" for a in home)
    for a, b in zip(home, want):
        assert torch.equal(a, b.cpu())


# ---- the consumer: pitch_shift(..., formant_order="f0") ----------------------------------------------------------------------------

PS_SR, PS_L = 16000, 8192


def _ps_kw():
    return dict(n_fft=512, hop_length=128, window=torch.hann_window(512), max_iter=4, verbose=False)


def _order_by_the_definition(x):
    f0, voiced, _ = si.yin(x, PS_SR, fmin=PS_SR / 1000, fmax=PS_SR / 20, frame_length=2048)
    if not voiced.any():
        return si.default_envelope_order(PS_SR)
    return min(512 // 2, si.envelope_order_for_f0(PS_SR, f0[voiced].median().item()))


def test_pitch_shift_reads_the_order_off_f0():
    from _envelope_oracle import voice
    low = torch.from_numpy(voice(110.0, 1.0, PS_L, PS_SR)).float()
    x = torch.stack([low, low.flip(0)]).to(DEV)
    order = _order_by_the_definition(x)
    print("order for the 110 Hz voice:", order, "default:", si.default_envelope_order(PS_SR))
    assert 65 <= order <= 80 and order != si.default_envelope_order(PS_SR)      # 16000 / 220 = 72.7, were f0 exactly 110 Hz
    got = si.pitch_shift(x, PS_SR, 3, preserve_formants=True, formant_order="f0", **_ps_kw())
    assert torch.equal(got, si.pitch_shift(x, PS_SR, 3, preserve_formants=True, formant_order=order, **_ps_kw()))
    silent = torch.zeros(2, PS_L, device=DEV)
    assert _order_by_the_definition(silent) == si.default_envelope_order(PS_SR)
    got = si.pitch_shift(silent, PS_SR, 3, preserve_formants=True, formant_order="f0", **_ps_kw())
    assert torch.equal(got, si.pitch_shift(silent, PS_SR, 3, preserve_formants=True, **_ps_kw()))
    plain = si.pitch_shift(x, PS_SR, 3, **_ps_kw())
    assert torch.equal(si.pitch_shift(x, PS_SR, 3, preserve_formants=False, formant_order="f0", **_ps_kw()), plain)
