"""spectral_envelope, impose_envelope and pitch_shift(preserve_formants=True) on the device.

Parity is against the float64 definition (tests/_envelope_oracle.py).  The bound is not a constant: the test runs the same
definition as a float32 torch chain on the CPU (`_chain32`: torch's log, irfft, a multiply, rfft, maximum), and that chain's largest
error in V against the oracle is the yardstick - the kernel has the same arithmetic depth, another butterfly order and the device's
log / exp, and may sit at up to 4 times that figure on the same input; for E the same figure, relative.

The yardstick is taken per input and order, as the chain's largest error over the iteration counts run on them (0, 1, 5, 16), not
per single setting.  At order 0 a frame's V is one number, at order 1 two, and with one to five frames the chain's error at a
single setting is the rounding of those few numbers: it came out as low as 1.2e-8 (n_fft 2048, T 1, order 0, n_iter 1), under
a tenth of an ulp of the float32 sum that carries the value, where the kernel's 2.3e-7 is within one ulp of it.  Setting by setting
over the 1024 combinations of the cases below, the kernel / chain ratio had median 1.19 and 90th percentile 2.09, and exceeded 4 in
18 of them, every one at order 0 or 1 with at most five frames (largest 19.4 at the setting above; the kernel's error in those 18
was at most 1.4e-6 absolute).  Per input and order the largest ratio was 3.39.  Figures: profiles/envelope_bench.json, DESIGN 3.27.

Frame tiles of the kernel (csrc/kernels_envelope.h): 32 frames up to n_fft 512, 16 at 1024, 8 at 2048; T runs over 1, 2, 5 and two
tiles plus one."""
import math

import numpy as np
import pytest
import torch

import _layouts
import spectrogram_inversion_amd as si
from _envelope_oracle import envelope_distance_db, log_envelope, voice
from spectrogram_inversion_amd.timescale import shift_rate

pytestmark = pytest.mark.gpu

DEV = "cuda"
TILE = {256: 32, 512: 32, 1024: 16, 2048: 8}
N_ITERS = (0, 1, 5, 16)
FLOOR = 1e-6


def _orders(n_fft):
    return (0, 1, n_fft // 16, n_fft // 2)


def _chain32(S, order, n_iter, floor=FLOOR):
    """The definition in float32 torch ops on the CPU: S (B, F, T) float32 / complex64 -> V (B, F, T) float32."""
    mag = S.abs()
    amin = (mag.amax(dim=(1, 2), keepdim=True) * floor).to(torch.float32)
    live = amin > 0
    a0 = torch.where(live, torch.log(torch.maximum(mag, torch.where(live, amin, torch.ones_like(amin)))), torch.zeros_like(mag))
    n_fft = 2 * (S.shape[1] - 1)
    q = torch.arange(n_fft)
    lift = (torch.minimum(q, n_fft - q) <= order).to(torch.float32)[None, :, None]

    def smooth(a):
        return torch.fft.rfft(torch.fft.irfft(a, n_fft, dim=1) * lift, n_fft, dim=1).real

    v = smooth(a0)
    for _ in range(n_iter):
        v = smooth(torch.maximum(a0, v))
    return v


def _spectrogram(n_fft, batch, n_frames, cplx, seed):
    """Harmonic-looking magnitudes over about 80 dB with some noise: V ranges over about +-10."""
    g = torch.Generator().manual_seed(seed)
    f = torch.arange(n_fft // 2 + 1, dtype=torch.float64)[None, :, None]
    pitch = 6 + 10 * torch.rand(batch, 1, n_frames, generator=g, dtype=torch.float64)
    comb = 0.5 + 0.5 * torch.cos(2 * math.pi * f / pitch)
    tilt = torch.exp(-6 * f / f.max()) * (1 + 3 * torch.exp(-((f - 0.2 * f.max()) / (0.05 * f.max())) ** 2))
    mag = 30 * tilt * comb ** 4 * (0.2 + torch.rand(batch, n_fft // 2 + 1, n_frames, generator=g, dtype=torch.float64)) + 1e-5
    if not cplx:
        return mag.float()
    ph = 2 * math.pi * torch.rand(mag.shape, generator=g, dtype=torch.float64)
    return torch.polar(mag, ph).to(torch.complex64)


def _check(S, order, n_iters, label, frame_major=False, two_dim=False):
    """S (B, F, T) on the CPU: the kernel's V and E against the oracle at every iteration count of `n_iters`, within 4 yardsticks;
    returns (yardstick, the kernel's largest error in V)"""
    arg = S.to(DEV)
    if frame_major:
        arg = arg.transpose(1, 2).contiguous()
    if two_dim:
        arg = arg[0]
    refs = {n: log_envelope(S.numpy(), order, n, FLOOR) for n in n_iters}
    chain = {n: float(np.abs(_chain32(S, order, n).double().numpy() - refs[n]).max()) for n in n_iters}
    yard = max(chain.values())
    worst = 0.0
    for n_iter in n_iters:
        ref = refs[n_iter]
        out = []
        for log in (True, False):
            got = si.spectral_envelope(arg, order, n_iter, FLOOR, log=log, frame_major=frame_major)
            assert got.shape == arg.shape and got.dtype == torch.float32 and got.device == arg.device
            got = got[None] if two_dim else got
            out.append((got.transpose(1, 2) if frame_major else got).double().cpu().numpy())
        v, e = out
        assert np.isfinite(v).all() and np.isfinite(e).all()
        err_v = float(np.abs(v - ref).max())
        err_e = float(np.abs(e / np.exp(ref) - 1).max())
        print(f"{label} order {order} n_iter {n_iter}: V in [{ref.min():.1f}, {ref.max():.1f}], float32 chain {chain[n_iter]:.2e} "
              f"(yardstick {yard:.2e}), kernel V {err_v:.2e} ({err_v / yard:.2f} x), E rel {err_e:.2e}")
        assert err_v <= 4 * yard, (label, order, n_iter, err_v, yard)
        assert err_e <= 4 * yard, (label, order, n_iter, err_e, yard)
        worst = max(worst, err_v)
    return yard, worst


@pytest.mark.parametrize("layout", ("FT", "BFT", "frame_major"))
@pytest.mark.parametrize("cplx", (False, True), ids=("real", "complex"))
@pytest.mark.parametrize("n_fft", (256, 512, 1024, 2048))
def test_parity_with_the_oracle(n_fft, cplx, layout):
    worst = 0.0
    for n_frames in (1, 2, 5, 2 * TILE[n_fft] + 1):
        batch = 1 if layout == "FT" else 3
        S = _spectrogram(n_fft, batch, n_frames, cplx, seed=n_fft + n_frames)
        for order in _orders(n_fft):
            yard, err_v = _check(S, order, N_ITERS, f"n_fft {n_fft} {layout} B {batch} T {n_frames}",
                                 frame_major=layout == "frame_major", two_dim=layout == "FT")
            worst = max(worst, err_v / yard)
    print(f"n_fft {n_fft} {layout}: the kernel's largest error is {worst:.2f} x the yardstick")


@pytest.mark.parametrize("n_fft", (256, 2048))
def test_silence_and_scale(n_fft):
    """a silent frame in the middle, an all-zero item beside a loud one, magnitudes scaled by 1e-4 and 1e4"""
    n_frames = TILE[n_fft] + 3
    for cplx in (False, True):
        S = _spectrogram(n_fft, 3, n_frames, cplx, seed=5)
        S[0, :, n_frames // 2] = 0
        S[1] = 0
        for scale in (1.0, 1e-4, 1e4):
            for order in (1, n_fft // 16):
                _check(S * scale, order, (0, 5, 16), f"n_fft {n_fft} {'complex' if cplx else 'real'} x {scale:g}")
        v = si.spectral_envelope((S * 1e4).to(DEV), n_fft // 16, 16, log=True)
        e = si.spectral_envelope((S * 1e4).to(DEV), n_fft // 16, 16)
        assert (v[1] == 0).all() and (e[1] == 1).all()


@pytest.mark.parametrize("name", ("strided", "step_last", "step_batch", "offset", "conj", "conj_strided"))
def test_layouts_give_the_dense_result_bit_for_bit(name):
    x = torch.randn(3, 2048, generator=torch.Generator().manual_seed(3)).to(DEV)
    S = torch.stft(x, 256, 64, window=torch.hann_window(256, device=DEV), return_complex=True)
    assert not S.is_contiguous()                                      # torch.stft's own output is a strided view
    Z = S.contiguous()
    want = si.spectral_envelope(Z, 16, 5)
    assert torch.equal(si.spectral_envelope(S, 16, 5), want)
    view, base = _layouts.build(name, Z)
    before = base.clone()
    assert torch.equal(si.spectral_envelope(view, 16, 5), want)
    assert torch.equal(si.spectral_envelope(_layouts.dense_twin(view, Z), 16, 5), want)
    assert torch.equal(base, before)
    if name in _layouts.REAL:
        M = Z.abs()
        rview, _ = _layouts.build(name, M)
        assert torch.equal(si.spectral_envelope(rview, 16, 5), si.spectral_envelope(M, 16, 5))
    # frame-major is the transpose, and a CPU tensor comes back to the CPU
    assert torch.equal(si.spectral_envelope(Z.transpose(1, 2), 16, 5, frame_major=True).transpose(1, 2), want)
    got = si.spectral_envelope(Z.cpu(), 16, 5)
    assert got.device.type == "cpu" and torch.equal(got, want.cpu())


def test_more_items_than_one_call_is_given():
    """70 000 items of one frame are 70 000 workgroups: the wrapper hands the entry point at most 65 535 at a time"""
    seven = _spectrogram(256, 7, 1, False, seed=9).to(DEV)
    many = seven.repeat(10000, 1, 1)
    want = si.spectral_envelope(seven, 16, 5, log=True)
    got = si.spectral_envelope(many, 16, 5, log=True)
    assert got.shape == many.shape and torch.equal(got, want.repeat(10000, 1, 1))


def test_halves_are_computed_in_float32():
    S = _spectrogram(256, 2, 9, False, seed=8)
    for dtype in (torch.float16, torch.bfloat16):
        h = S.to(dtype)
        got = si.spectral_envelope(h.to(DEV), 16, 5, log=True)
        assert got.dtype == dtype
        assert torch.equal(got, si.spectral_envelope(h.float().to(DEV), 16, 5, log=True).to(dtype))


# ---- impose_envelope and pitch_shift -----------------------------------------------------------------------------------------------

L, SR = 8192, 16000


def _kw():
    return dict(n_fft=512, hop_length=128, window=torch.hann_window(512))


def _fit(y, n):
    return y[..., :n] if y.shape[-1] >= n else torch.nn.functional.pad(y, (0, n - y.shape[-1]))


@pytest.fixture(scope="module")
def spoken():
    return torch.from_numpy(voice(150.0, 1.0, L, SR)).float().to(DEV)


def test_imposing_a_signals_own_envelope_is_the_stft_round_trip(spoken):
    x = torch.stack([spoken, spoken.flip(0)])
    want = _fit(si.istft(si.stft(x, **_kw()), hop_length=128, window=_kw()["window"]), L)
    got = si.impose_envelope(x, x, order=27, **_kw())
    assert got.shape == x.shape and got.dtype == x.dtype
    print("largest difference to istft(stft(x)):", float((got - want).abs().max()))
    assert torch.equal(got, want)                                      # the gain is exactly 1


def test_impose_envelope_is_the_composition(spoken):
    y = torch.roll(spoken, 100) * torch.linspace(0.5, 1.5, L, device=DEV)
    kw = dict(hop_length=128, window=torch.hann_window(512))
    Y, X = si.stft(y, 512, **kw), si.stft(spoken, 512, **kw)
    vy, vx = (si.spectral_envelope(s, 20, 8, 1e-5, log=True) for s in (Y, X))
    g = 30.0 * math.log(10.0) / 20.0
    want = _fit(si.istft(Y * torch.exp(torch.clamp(vx - vy, -g, g)), **kw), L)
    got = si.impose_envelope(y, spoken, 512, 20, 8, 1e-5, 30.0, **kw)
    assert torch.equal(got, want)
    assert not torch.equal(got, si.impose_envelope(y, spoken, 512, 20, 8, 1e-5, 3.0, **kw))       # the clamp is live


@pytest.mark.parametrize("n_steps", (4, -4), ids=("+4", "-4"))
def test_pitch_shift_keeps_the_formants_only_when_asked(spoken, n_steps):
    x = spoken
    kw = dict(max_iter=8, verbose=False, **_kw())
    rate, orig = shift_rate(SR, n_steps)
    today = _fit(si.resample(si.time_stretch(x, rate, **kw), orig, SR, 6, 0.99), L)     # pitch_shift as it stood: its own test's words
    plain = si.pitch_shift(x, SR, n_steps, **kw)
    assert torch.equal(plain, today)
    assert torch.equal(si.pitch_shift(x, SR, n_steps, preserve_formants=False, formant_order=40, formant_iter=3, **kw), today)
    kept = si.pitch_shift(x, SR, n_steps, preserve_formants=True, **kw)
    assert kept.shape == x.shape and kept.dtype == x.dtype and kept.device == x.device
    stft_kw = dict(hop_length=128, window=kw["window"])
    assert torch.equal(kept, si.impose_envelope(plain, x, 512, si.default_envelope_order(SR), 16, **stft_kw))
    assert torch.equal(si.pitch_shift(x, SR, n_steps, preserve_formants=True, formant_order=20, formant_iter=4, **kw),
                       si.impose_envelope(plain, x, 512, 20, 4, **stft_kw))
    r = 2.0 ** (n_steps / 12)
    x64 = x.double().cpu().numpy()
    d_plain = envelope_distance_db(plain.double().cpu().numpy(), x64, 512, 128, 27, r)
    d_kept = envelope_distance_db(kept.double().cpu().numpy(), x64, 512, 128, 27, r)
    print(f"{n_steps:+d} semitones: envelope distance to x {d_plain:.2f} dB without, {d_kept:.2f} dB with preserve_formants")
    assert d_kept <= 0.5 * d_plain
