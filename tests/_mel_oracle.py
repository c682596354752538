"""Float64 NumPy restatement of the mel NNLS (spectrogram_inversion_amd.mel_inverse.mel_to_stft, include/specinv.h:
specinv_mel_nnls): per frame, FISTA from zero on 1/2 |M s - y|^2 subject to s >= 0, step 1 / L, L = lambda_max(M M^T)."""
import numpy as np


def lipschitz(M):
    M = np.asarray(M, dtype=np.float64)
    return float(np.linalg.eigvalsh(M @ M.T)[-1])


def fista_nnls(M, Y, n_iter, power=1.0, L=None):
    """M (n_mels, F), Y (n_mels, T) -> (F, T): every column at once (the iteration is column-wise)."""
    M = np.asarray(M, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64)
    if L is None:
        L = lipschitz(M)
    s = np.zeros((M.shape[1], Y.shape[1]))
    z = s.copy()
    t = 1.0
    for _ in range(n_iter):
        g = M.T @ (M @ z - Y)
        s_new = np.maximum(0.0, z - g / L)
        t_new = (1.0 + np.sqrt(1.0 + 4.0 * t * t)) / 2.0
        z = s_new + ((t - 1.0) / t_new) * (s_new - s)
        s, t = s_new, t_new
    return s ** (1.0 / power)


def mel_to_stft(M, mel, n_iter, power=1.0):
    """(n_mels, T) / (B, n_mels, T) -> (F, T) / (B, F, T)"""
    mel = np.asarray(mel, dtype=np.float64)
    if mel.ndim == 2:
        return fista_nnls(M, mel, n_iter, power)
    return np.stack([fista_nnls(M, m, n_iter, power) for m in mel])


def kkt_violation(M, Y, S, scale=None):
    """Largest violation of the optimality conditions of min 1/2 |M s - Y|^2, s >= 0 over the columns, relative to |M^T Y|:
    negativity of s, a negative gradient where s = 0, a non-zero gradient where s > 0."""
    M = np.asarray(M, dtype=np.float64)
    G = M.T @ (M @ S - Y)
    scale = scale if scale is not None else max(np.abs(M.T @ Y).max(), 1e-300)
    pos = S > 0
    return max(float(-S.min(initial=0.0)), float(np.abs(G[pos]).max(initial=0.0)), float(-G[~pos].min(initial=0.0))) / scale


def excess_objective(M, Y, S, S_opt):
    """(objective(S) - objective(S_opt)) / (1/2 |Y|^2), summed over the columns"""
    M = np.asarray(M, dtype=np.float64)
    f = 0.5 * ((M @ S - Y) ** 2).sum()
    f0 = 0.5 * ((M @ S_opt - Y) ** 2).sum()
    return float((f - f0) / (0.5 * (Y ** 2).sum()))


def mel_sc(M, Y, S):
    """mel-domain spectral convergence |M S - Y| / |Y|"""
    return float(np.linalg.norm(np.asarray(M, dtype=np.float64) @ S - Y) / np.linalg.norm(Y))


def chirp_signal(sr=22050, seconds=2.0, seed=0):
    """chirp + tone + a little noise"""
    rng = np.random.default_rng(seed)
    t = np.arange(int(sr * seconds)) / sr
    x = 0.5 * np.sin(2 * np.pi * (200 * t + 900 * t ** 2)) + 0.3 * np.sin(2 * np.pi * 440 * t)
    return x + 0.01 * rng.standard_normal(t.shape)


def magnitude(x, n_fft=2048, hop=512):
    """|STFT| (F, T) with a periodic Hann window, frames centred with reflect padding (torch.stft's defaults)"""
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)
    xp = np.pad(x, n_fft // 2, mode="reflect")
    n = 1 + (len(xp) - n_fft) // hop
    fr = np.stack([xp[i * hop:i * hop + n_fft] * w for i in range(n)], 1)
    return np.abs(np.fft.rfft(fr, axis=0))
