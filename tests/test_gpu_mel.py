"""Mel inversion on the device (mel_to_stft / mel_to_audio, k_mel_nnls) against the float64 restatement of its algorithm
(tests/_mel_oracle.py): fixed-iteration parity over filterbank shapes, powers, dtypes and edge cases; convergence; the two-stage
pipeline; the bench geometry."""
import numpy as np
import pytest
import torch

import _mel_oracle as mo
import spectrogram_inversion_amd as si
from spectrogram_inversion_amd import _lib
from spectrogram_inversion_amd.mel import mel_filterbank
from spectrogram_inversion_amd.plan import Plan, args_helper

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
# float32 against the float64 restatement, per item: FISTA's momentum carries the float32 rounding of every iteration forward
# (bound set from the first run on the MI355X: largest figure 1e-5 order; 1e-4 leaves room and stays far below 1e-3)
TOL = {torch.float64: 1e-10, torch.float32: 1e-4}


def _banks():
    rng = np.random.default_rng(7)
    dense = rng.random((64, 513))
    holes = mel_filterbank(16000, 512, 40).astype(np.float64)
    holes[5] = 0.0                  # an all-zero row
    holes[:, 100] = 0.0             # ... and column
    return {
        "slaney80x1025": mel_filterbank(22050, 2048, 80).astype(np.float64),
        "htk128x513": mel_filterbank(16000, 1024, 128, htk=True).astype(np.float64),
        "fmin_fmax_nonorm40x257": mel_filterbank(16000, 512, 40, fmin=300.0, fmax=6000.0, norm=None).astype(np.float64),
        "dense64x513": dense,
        "zero_row_col40x257": holes,
    }


BANKS = _banks()


def _mel_input(M, B, T, power, seed):
    """mel of random magnitudes (B, n_mels, T), with a silent frame and undershooting (negative) entries"""
    rng = np.random.default_rng(seed)
    S = rng.random((B, M.shape[1], T)) ** 2
    mel = np.einsum("mf,bft->bmt", M, S ** power)
    mel *= 1.0 + 0.05 * rng.standard_normal(mel.shape)
    mel[:, :, T // 3] = 0.0
    mel[:, rng.integers(0, M.shape[0], 4), 1] = -0.05 * np.abs(mel).max()
    return mel


def _per_item_rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    a, b = a.reshape(-1, *a.shape[-2:]), b.reshape(-1, *b.shape[-2:])
    return max(float(np.linalg.norm(x - y) / max(np.linalg.norm(y), 1e-300)) for x, y in zip(a, b))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(BANKS))
def test_fixed_iteration_parity(name, dtype):
    M = BANKS[name]
    Mt = M.astype(np.float32).astype(np.float64) if dtype == torch.float32 else M
    for power in (1.0, 2.0, 0.5):
        mel3 = _mel_input(M, 3, 37, power, seed=10 * list(BANKS).index(name) + int(4 * power))
        mel3 = mel3.astype(np.float32).astype(np.float64) if dtype == torch.float32 else mel3
        for n_iter in (1, 7, 100):
            got3 = si.mel_to_stft(torch.from_numpy(mel3).to(DEV, dtype), torch.from_numpy(M).to(dtype), power=power, n_iter=n_iter)
            ref3 = mo.mel_to_stft(Mt, mel3, n_iter, power)
            assert got3.shape == (3, M.shape[1], 37) and got3.dtype == dtype and got3.device == DEV
            got3 = got3.cpu().numpy()
            assert np.all(np.isfinite(got3)) and got3.min() >= 0
            assert np.all(got3[:, :, 37 // 3] == 0.0), "a silent frame gives exact zeros"
            err = _per_item_rel(got3, ref3)
            assert err <= TOL[dtype], (name, power, n_iter, err)
            got2 = si.mel_to_stft(torch.from_numpy(mel3[1, :, :29]).to(DEV, dtype), M, power=power, n_iter=n_iter)
            assert got2.shape == (M.shape[1], 29)
            assert _per_item_rel(got2.cpu().numpy(), mo.mel_to_stft(Mt, mel3[1, :, :29], n_iter, power)) <= TOL[dtype]
    if name == "zero_row_col40x257":
        assert np.all(got3[:, 100] == 0.0), "a bin no band touches stays zero"


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_n_fft_8192(dtype):
    M = mel_filterbank(44100, 8192, 96).astype(np.float64)
    Mt = M.astype(np.float32).astype(np.float64) if dtype == torch.float32 else M
    mel3 = _mel_input(M, 2, 11, 1.0, seed=3)
    mel3 = mel3.astype(np.float32).astype(np.float64) if dtype == torch.float32 else mel3
    got = si.mel_to_stft(torch.from_numpy(mel3).to(DEV, dtype), M, n_iter=7).cpu().numpy()
    assert _per_item_rel(got, mo.mel_to_stft(Mt, mel3, 7)) <= TOL[dtype]


def test_convergence():
    M = mel_filterbank(22050, 2048, 80).astype(np.float64)
    S = mo.magnitude(mo.chirp_signal())
    for power, kkt, sc in ((1.0, 1e-6, 3e-4), (2.0, 1e-4, 3e-3)):
        Y = M @ S ** power
        s300 = si.mel_to_stft(torch.from_numpy(Y).to(DEV), M, power=power, n_iter=300).cpu().numpy() ** power
        assert mo.kkt_violation(M, Y, s300) < kkt
        for dtype, slack in ((torch.float64, 1.0), (torch.float32, 1.5)):
            s100 = si.mel_to_stft(torch.from_numpy(Y).to(DEV, dtype), M, power=power).cpu().double().numpy() ** power
            assert mo.mel_sc(M, Y, s100) <= sc * slack, (power, dtype)


def _hann(n):
    return torch.hann_window(n, dtype=torch.float64).float()


@pytest.mark.parametrize("method,kw", [("griffin_lim", dict(max_iter=30, alpha=0.99)), ("ADMM", dict(max_iter=30, rho=0.1)),
                                       ("RTISI_LA", dict(max_iter=4, look_ahead=3))])
def test_mel_to_audio_is_the_two_calls(method, kw):
    M = mel_filterbank(22050, 1024, 64)
    mel = torch.from_numpy(_mel_input(M.astype(np.float64), 2, 41, 1.0, seed=5)).float().to(DEV)
    stft = dict(hop_length=256, window=_hann(1024))
    a = si.mel_to_audio(mel, M, n_iter=50, method=method, verbose=False, **kw, **stft)
    mag = si.mel_to_stft(mel, M, n_iter=50, **stft)
    b = getattr(si, method)(mag, verbose=False, **kw, **stft)
    assert a.shape == b.shape and torch.equal(a, b)


def test_end_to_end_mel_sc():
    """The mel of the waveform rebuilt from the mel (NNLS 100 + Griffin-Lim 100) against the same Griffin-Lim on the true
    magnitude: within 2 x its mel-domain SC."""
    n_fft, hop = 2048, 512
    M = mel_filterbank(22050, n_fft, 80)
    x = torch.from_numpy(mo.chirp_signal(seconds=3.0)).float().to(DEV)
    win = torch.hann_window(n_fft, device=DEV)
    mag = torch.stft(x, n_fft, hop, window=win, return_complex=True).abs()
    Mt = torch.from_numpy(M).to(DEV)
    mel = Mt @ mag
    kw = dict(max_iter=100, hop_length=hop, window=win.cpu(), verbose=False, tol=0)

    def mel_sc(y):
        m = Mt @ torch.stft(y, n_fft, hop, window=win, return_complex=True).abs()
        n = min(m.shape[-1], mel.shape[-1])
        return float(torch.linalg.norm(m[:, :n] - mel[:, :n]) / torch.linalg.norm(mel[:, :n]))

    sc_mel = mel_sc(si.mel_to_audio(mel, M, **kw))
    sc_true = mel_sc(si.griffin_lim(mag, **kw))
    assert sc_mel <= 2.0 * sc_true, (sc_mel, sc_true)


def test_bench_size_sample():
    B, T, n_fft = 16, 1024, 2048
    M = mel_filterbank(22050, n_fft, 80)
    g = torch.Generator(device=DEV).manual_seed(0)
    mag = torch.rand((B, n_fft // 2 + 1, T), device=DEV, generator=g) ** 2
    mel = torch.from_numpy(M).to(DEV) @ mag
    out = si.mel_to_stft(mel, M, n_iter=100)
    assert out.shape == (B, n_fft // 2 + 1, T)
    rng = np.random.default_rng(1)
    Mt = M.astype(np.float64)
    for b, t in zip(rng.integers(0, B, 12), rng.integers(0, T, 12)):
        y = mel[b, :, t:t + 1].double().cpu().numpy()
        ref = mo.fista_nnls(Mt, y, 100)
        got = out[b, :, t:t + 1].double().cpu().numpy()
        assert np.linalg.norm(got - ref) <= TOL[torch.float32] * np.linalg.norm(ref), (b, t)


def test_cpu_half_and_cache():
    M = mel_filterbank(16000, 512, 40)
    mel = torch.from_numpy(_mel_input(M.astype(np.float64), 1, 23, 1.0, seed=2)[0]).float()
    a = si.mel_to_stft(mel, M)                               # CPU in, CPU out, 2-D
    assert a.device.type == "cpu" and a.shape == (257, 23)
    args = args_helper(torch.empty(1, 257, 1))
    from spectrogram_inversion_amd.plan import get_plan
    plan = get_plan(args, 1, 23, torch.float32, DEV)
    key = plan._nnls_key
    b = si.mel_to_stft(mel, torch.from_numpy(M))             # the same bank again (a tensor this time): the plan keeps its setup
    assert plan._nnls_key == key and torch.equal(a, b)
    c = si.mel_to_stft(mel.half(), M)
    assert c.dtype == torch.float16 and c.device.type == "cpu"
    assert torch.allclose(c.float(), a, rtol=2e-2, atol=1e-3 * float(a.abs().max()))
    d = si.mel_to_stft(mel.bfloat16().to(DEV), M)
    assert d.dtype == torch.bfloat16 and d.device == DEV


def test_nnls_before_setup_and_errors():
    args = args_helper(torch.empty(1, 257, 1))
    plan = Plan(args, 1, 4, torch.float32, DEV)
    y = torch.zeros(1, 40, 4, device=DEV)
    out = torch.empty(1, 257, 4, device=DEV)
    assert plan.lib.specinv_mel_nnls(plan._h, y.data_ptr(), 10, 1.0, out.data_ptr()) == _lib.EINVAL
    assert b"setup" in plan.lib.specinv_last_error()
    with pytest.raises(ValueError):
        si.mel_to_stft(torch.zeros(40, 4, device=DEV), np.zeros((40, 257)))
    with pytest.raises(ValueError):
        si.mel_to_stft(torch.zeros(30, 4, device=DEV), mel_filterbank(16000, 512, 40))
