"""Accelerated Griffin-Lim with known bins and known samples in NumPy on the oracle's STFT building blocks: what
`spectrogram_inversion_amd.constrained_griffin_lim` and `specinv_agla_constrain` compute.  A helper of the constrained tests, not a
test file.  With M the mask of known bins, K their values, m the magnitudes, W the mask of known samples and xk their values:

    m_full = where(M, |K|, m) ;  start = where(M, K, spec)  (a real spec: where(M, K, phase_init(m_full)))
    c = istft(start) ; repeat: S = stft(c)
        split  (what the library computes):  u = istft(S m' / (|S| + 1e-16)) + k,   m' = where(M, 0, m), k = istft(where(M, K, 0))
        direct (the definition):             u = istft(where(M, K, S m / (|S| + 1e-16)))
        n = 1:  t = c = d = where(W, xk, u)
        n > 1:  t' = where(W, xk, (1 - gamma) d + gamma u) ; c = t' + alpha (t' - t) ; d = t' + beta (t' - t) ; t = t'
    result: t

All arithmetic in the dtype of the spectrogram and in the order written; (1 - gamma), gamma, alpha and beta are rounded to it once.
The envelope of the first inverse transform is kept, the evaluation is `oracle.methods.training_loop` on |stft(t)| against m_full."""
import numpy as np

from oracle import methods as _om
from oracle.stftlib import args_helper, istft, stft


def cgla(spec, max_iter, known_spec=None, spec_mask=None, known_wave=None, wave_mask=None, alpha=0.99, beta=None, gamma=1.0,
         tol=0.0, eva_iter=10, metric="sc", trace=None, direct=False, **stft_kwargs):
    """spec (B, F, T) or (F, T), complex (the start, its modulus the target) or real magnitudes; known_spec of its shape with
    spec_mask, known_wave (B, L) / (L,) with wave_mask, both masks broadcastable.  Returns t (B, L) / (L,).  `trace` receives the
    (iteration, metric, mse) of every evaluation."""
    spec = np.asarray(spec)
    squeeze = spec.ndim == 2
    spec3 = spec[None] if squeeze else spec
    cplx = np.iscomplexobj(spec3)
    m = np.abs(spec3) if cplx else spec3
    rdt, cdt = m.dtype.type, np.result_type(m.dtype, np.complex64)
    a = args_helper(m.shape[-2], m.dtype, **stft_kwargs)
    if known_spec is not None:
        M = np.broadcast_to(np.asarray(spec_mask, bool), spec.shape).reshape(spec3.shape)
        K = np.asarray(known_spec).astype(cdt).reshape(spec3.shape)
    else:
        M, K = np.zeros(spec3.shape, bool), np.zeros(spec3.shape, cdt)
    m_full = np.where(M, np.abs(K), m)
    m_free = np.where(M, rdt(0), m)
    start = np.where(M, K, spec3 if cplx else _om.phase_init(m_full, **stft_kwargs)).astype(cdt)
    with np.errstate(all="ignore"):
        c, env = istft(start, a)
        k, _ = istft(np.where(M, K, cdt.type(0)), a, envelope=env)
    c, k = c.astype(m.dtype), k.astype(m.dtype)
    if known_wave is not None:
        xk = np.asarray(known_wave).astype(m.dtype).reshape(c.shape)
        W = np.broadcast_to(np.asarray(wave_mask, bool), np.asarray(known_wave).shape).reshape(c.shape)
    else:
        xk, W = np.zeros_like(c), np.zeros(c.shape, bool)
    beta = alpha if beta is None else beta
    general = gamma != 1.0
    al, be, ga, omg = rdt(alpha), rdt(beta), rdt(gamma), rdt(1.0 - gamma)
    st = {"c": c, "t": None, "d": None, "n": 0}

    def closure():
        S = stft(st["c"], a)
        with np.errstate(all="ignore"):
            if direct:
                u, _ = istft(np.where(M, K, S * m / (np.abs(S) + rdt(1e-16))), a, envelope=env)
                u = u.astype(m.dtype)
            else:
                y, _ = istft(S * m_free / (np.abs(S) + rdt(1e-16)), a, envelope=env)
                u = y.astype(m.dtype) + k
            if st["t"] is None:
                t = np.where(W, xk, u)
                st["c"], st["d"] = t, (t if general else None)
            else:
                t = np.where(W, xk, omg * st["d"] + ga * u if general else u)
                diff = t - st["t"]
                st["c"] = t + al * diff
                if general:
                    st["d"] = t + be * diff
        st["t"] = t
        st["n"] += 1
        return np.abs(stft(t, a)) if st["n"] % eva_iter == 0 else None      # (training_loop reads it at those iterations alone)

    _om.training_loop(closure, m_full, max_iter, tol, eva_iter, metric, trace)
    return st["t"][0] if squeeze else st["t"]
