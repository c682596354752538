"""tests/_misi_oracle.py restated in torch, so that autograd differentiates it on the CPU: the reference of `misi_unfolded`'s
gradients.  A helper of the MISI tests, not a test file.

    C0 = specs (complex)  or  polar(specs, angle(stft(mix)))          (_misi_oracle.mixture_phase_start)
    x = mix step(istft(C0)) ; repeat: S = stft(x) ; Y = S m / (|S| + 1e-16) ; x = mix step(istft(Y))
    mix step: s = x_0 + x_1 + ... (ascending k) ; e = (mix - s) / K ; x_k = x_k + e

The transforms are oracle/stftlib.py's: `torch.stft`; the inverse real / complex transform of every frame, times the window,
overlap-added, divided by the window-square envelope.  All arithmetic in the dtype of `specs`.  The target m is |specs| for a
complex start and `specs` itself for magnitudes (what the device gets)."""
import numpy as np
import torch

from oracle.stftlib import args_helper, signal_length


def _setup(F, dtype, stft_kwargs):
    """(StftArgs, window as a torch tensor of `dtype`)"""
    kw = {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in stft_kwargs.items()}
    a = args_helper(F, np.float64 if dtype == torch.float64 else np.float32, **kw)
    return a, torch.from_numpy(np.ascontiguousarray(a.window)).to(dtype)


def stft(x, a, w):
    """(B, L) -> (B, F, T) complex"""
    return torch.stft(x, a.n_fft, hop_length=a.hop_length, win_length=a.n_fft, window=w, center=a.center, pad_mode=a.pad_mode,
                      normalized=a.normalized, onesided=a.onesided, return_complex=True)


def _overlap_add(fr, hop, padding):
    """(B, T, N) -> (B, (T - 1) hop + N - 2 padding): y[b, t hop + k - padding] += fr[b, t, k]"""
    b, t, n = fr.shape
    full = torch.zeros((b, (t - 1) * hop + n), dtype=fr.dtype)
    for i in range(t):
        full[:, i * hop:i * hop + n] = full[:, i * hop:i * hop + n] + fr[:, i]
    return full[:, padding:full.shape[1] - padding] if padding else full


def envelope(n_frames, a, w):
    return _overlap_add((w * w).expand(1, n_frames, a.n_fft), a.hop_length, a.padding)[0]


def istft(spec, a, w, env):
    """(B, F, T) complex -> (B, L), no zero guard on the envelope"""
    norm = "ortho" if a.normalized else "backward"
    s = spec.transpose(1, 2)
    fr = torch.fft.irfft(s, n=a.n_fft, dim=-1, norm=norm) if a.onesided else torch.fft.ifft(s, n=a.n_fft, dim=-1, norm=norm).real
    return _overlap_add(fr * w, a.hop_length, a.padding) / env


def mix_step(x, mix):
    """x (B, K, L), mix (B, L) -> x_k + (mix - sum_k x_k) / K"""
    K = x.shape[1]
    s = x[:, 0]
    for k in range(1, K):
        s = s + x[:, k]
    return x + ((mix - s) / K)[:, None, :]


def misi(specs, mix, n_iter, **stft_kwargs):
    """specs (B, K, F, T) complex or real, mix (B, L_m) real, CPU tensors of one precision.  Returns x (B, K, L) after `n_iter`
    iterations; differentiable with respect to both."""
    B, K, F, T = specs.shape
    rdt = mix.dtype
    a, w = _setup(F, rdt, stft_kwargs)
    L = signal_length(T, a)
    env = envelope(T, a, w)
    mix = mix[:, :L]
    if specs.is_complex():
        C, m = specs, specs.abs()
    else:
        C, m = torch.polar(specs, torch.angle(stft(mix, a, w))[:, None].expand(B, K, F, T)), specs
    C, m = C.reshape(B * K, F, T), m.reshape(B * K, F, T)
    x = mix_step(istft(C, a, w, env).reshape(B, K, L), mix)
    for _ in range(n_iter):
        S = stft(x.reshape(B * K, L), a, w)
        x = mix_step(istft(S * m / (S.abs() + 1e-16), a, w, env).reshape(B, K, L), mix)
    return x
