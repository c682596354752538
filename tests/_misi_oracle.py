"""MISI (Gunawan & Sen 2010) in NumPy on the oracle's STFT building blocks: what `spectrogram_inversion_amd.misi` and the
`specinv_misi_*` entry points compute.  A helper of the MISI tests, not a test file.

    x = istft(C), mixed ; repeat: S = stft(x) ; Y = S m / (|S| + 1e-16) ; y = istft(Y) ; x = mix step(y)
    mix step: s = x_0 + x_1 + ... (ascending k) ; e = (mix - s) / K ; x_k = x_k + e

All arithmetic in the dtype of the start, the envelope of the first inverse transform kept (the reference's
torch_specinv/methods.py:233, :248), the evaluation by its `_training_loop` rule (:180-190)."""
import numpy as np

from oracle import methods as _om
from oracle.stftlib import args_helper, istft, signal_length, stft


def mix_step(x, mix, mix_on=True):
    """x (B, K, L), mix (B, L) -> x_k + (mix - sum_k x_k) / K"""
    if not mix_on:
        return x
    K = x.shape[1]
    s = x[:, 0].copy()
    for k in range(1, K):
        s = s + x[:, k]
    e = (mix - s) / x.dtype.type(K)
    return x + e[:, None, :]


def misi(C, mix, max_iter, tol=0.0, eva_iter=10, metric="sc", trace=None, sums=None, mix_on=True, **stft_kwargs):
    """C (B, K, F, T) or (K, F, T) complex, mix (B, L_m) or (L_m,).  Returns x (B, K, L) / (K, L).
    `trace` receives the (iteration, metric, mse) of every evaluation, `sums` its (sum (|S| - m)^2, sum |S|^2, sum m^2, count).
    mix_on=False leaves the coupling out: Griffin-Lim without momentum from a complex start."""
    C = np.asarray(C)
    squeeze = C.ndim == 3
    C4 = C[None] if squeeze else C
    B, K, F, T = C4.shape
    a = args_helper(F, C4.dtype, **stft_kwargs)
    L = signal_length(T, a)
    rdt = np.float32 if C4.dtype == np.complex64 else np.float64
    mix2 = np.asarray(mix, dtype=rdt).reshape(B, -1)[:, :L]
    Cf = C4.reshape(B * K, F, T)
    m = np.abs(Cf)
    with np.errstate(all="ignore"):
        x, env = istft(Cf, a)
    st = {"x": mix_step(x.astype(rdt).reshape(B, K, L), mix2, mix_on)}

    def closure():
        S = stft(st["x"].reshape(B * K, L), a)
        out = np.abs(S)
        if sums is not None:
            d = out.astype(np.float64) - m
            sums.append((float((d * d).sum()), float((out.astype(np.float64) ** 2).sum()),
                         float((m.astype(np.float64) ** 2).sum()), float(m.size)))
        Y = S * m / (out + rdt(1e-16))
        with np.errstate(all="ignore"):
            y, _ = istft(Y, a, envelope=env)
        st["x"] = mix_step(y.astype(rdt).reshape(B, K, L), mix2, mix_on)
        return out

    _om.training_loop(closure, m, max_iter, tol, eva_iter, metric, trace)
    return st["x"][0] if squeeze else st["x"]


def mixture_phase_start(mag, mix, **stft_kwargs):
    """polar(mag, angle(STFT(mix))): mag (B, K, F, T) real, mix (B, L_m); the angle of an exact 0 is 0."""
    mag = np.asarray(mag)
    B, K, F, T = mag.shape
    a = args_helper(F, mag.dtype, **stft_kwargs)
    L = signal_length(T, a)
    S = stft(np.asarray(mix, dtype=mag.dtype).reshape(B, -1)[:, :L], a)
    ph = np.angle(S).astype(mag.dtype)
    cd = np.complex64 if mag.dtype == np.float32 else np.complex128
    return (mag * (np.cos(ph) + 1j * np.sin(ph))[:, None]).astype(cd)
