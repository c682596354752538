"""consistent_wiener without a device: properties of the definition (tests/_cwf_oracle.py, float64) and the argument errors, which
are raised before the device is touched - on a machine without one every accepted call would end in require_gpu's RuntimeError."""
import ctypes as C

import pytest
import torch

import spectrogram_inversion_amd as si
from spectrogram_inversion_amd import _lib, build
from _cwf_oracle import chirps_in_noise, consistency, consistency_adjoint, cwf_item, dot, sdr

F64 = torch.float64


def _kw(n_fft, hop):
    return dict(hop_length=hop, window=torch.hann_window(n_fft, dtype=F64))


def _spec(shape, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.complex(torch.randn(shape, generator=gen, dtype=F64), torch.randn(shape, generator=gen, dtype=F64))


@pytest.mark.parametrize("n_fft,hop,frames", [(64, 16, 5), (128, 32, 9), (400, 160, 6)])
def test_adjoint_identity(n_fft, hop, frames):
    """<G a, b> = <a, G' b> to float64 rounding, and G is not its own adjoint: <G a, b> - <a, G b> is of the products' size"""
    kw = _kw(n_fft, hop)
    a, b = _spec((n_fft // 2 + 1, frames), 1), _spec((n_fft // 2 + 1, frames), 2)
    lhs, rhs = dot(consistency(a, kw), b), dot(a, consistency_adjoint(b, kw))
    scale = (dot(a, a) * dot(b, b)) ** 0.5
    print(f"<Ga,b> {lhs:.6e} <a,G'b> {rhs:.6e} scale {scale:.3e}")
    assert abs(lhs - rhs) <= 1e-13 * scale
    assert abs(lhs - dot(a, consistency(b, kw))) > 1e-3 * scale


@pytest.fixture(scope="module")
def example():
    """the 512 / 128 example: 1 s of five chirping partials in white noise near 0 dB, both powers known"""
    kw = _kw(512, 128)
    s, n = chirps_in_noise(16000, 3, noise=0.85)
    St, Nt = (torch.stft(v, 512, return_complex=True, **kw) for v in (s, n))
    return kw, s, St + Nt, St.abs() ** 2, Nt.abs() ** 2


def test_objective_decreases_every_iteration(example):
    kw, _, X, vs, vn = example
    *_, res, obj = cwf_item(X, vs, vn, gamma=1.0, n_iter=12, with_objective=True, **kw)
    print("objective", " ".join(f"{o:.8e}" for o in obj))
    assert all(b < a for a, b in zip(obj, obj[1:]))
    assert res[0] == 1.0 and res[-1] < res[0]


def test_thirty_iterations_gain_sdr_over_the_wiener_estimate(example):
    kw, s, X, vs, vn = example
    S0 = cwf_item(X, vs, vn, n_iter=0, **kw)[0]
    S, N, res, _ = cwf_item(X, vs, vn, gamma=1.0, n_iter=30, **kw)
    x0, x = (torch.istft(Z, 512, **kw) for Z in (S0, S))
    ref = s[:x.numel()]
    print(f"input {sdr(ref, torch.istft(X, 512, **kw)):.2f} dB, Wiener {sdr(ref, x0):.2f} dB, consistent {sdr(ref, x):.2f} dB, "
          f"residual {res[-1]:.2e}")
    assert sdr(ref, x) > sdr(ref, x0)
    assert torch.equal(S + N, X) or (S + N - X).abs().max() <= 2 ** -52 * X.abs().max()
    incons = lambda Z: float((Z - consistency(Z, kw)).norm() / Z.norm())       # noqa: E731
    assert incons(S) < incons(S0)


def test_relative_gamma_is_scale_equivariant(example):
    kw, _, X, vs, vn = example
    X, vs, vn = X[:, :9], vs[:, :9], vn[:, :9]
    c = 3.7
    S1 = cwf_item(X, vs, vn, gamma=2.0, n_iter=6, **kw)[0]
    S2 = cwf_item(X * c, vs * c * c, vn * c * c, gamma=2.0, n_iter=6, **kw)[0]
    gap = float((S2 - c * S1).norm() / (c * S1).norm())
    print(f"relative gap {gap:.3e}")
    assert gap < 1e-12
    S3 = cwf_item(X * c, vs * c * c, vn * c * c, gamma=2.0, n_iter=6, relative=False, **kw)[0]
    assert float((S3 - c * S1).norm() / (c * S1).norm()) > 1e-6


def test_dead_and_silent_items_in_the_definition():
    kw = _kw(64, 16)
    X = _spec((33, 5), 4)
    one = torch.ones(33, 5, dtype=F64)
    S, N, res, _ = cwf_item(X, 0 * one, 0 * one, n_iter=3, **kw)
    assert not S.any() and torch.equal(N, X) and res == [0.0] * 4
    S, N, res, _ = cwf_item(0 * X, one, one, n_iter=3, **kw)
    assert not S.any() and not N.any() and res == [0.0] * 4


# ---- argument errors, before the device is touched -------------------------------------------------------------------------------
X = torch.zeros(2, 33, 5, dtype=torch.complex64)
V = torch.ones(2, 33, 5)
KW = dict(hop_length=16, window=torch.hann_window(64))

BAD = [
    (TypeError, lambda: si.consistent_wiener(X.real, V, V, **KW)),                       # a real mixture
    (TypeError, lambda: si.consistent_wiener(X, X, V, **KW)),                            # a complex variance
    (TypeError, lambda: si.consistent_wiener(X, V, V.long(), **KW)),
    (TypeError, lambda: si.consistent_wiener(X, V, 1.0, **KW)),
    (TypeError, lambda: si.consistent_wiener([1, 2], V, V, **KW)),
    (ValueError, lambda: si.consistent_wiener(X, V[:, :32], V, **KW)),                   # shapes that do not broadcast
    (ValueError, lambda: si.consistent_wiener(X, V, torch.ones(3, 1, 1), **KW)),
    (ValueError, lambda: si.consistent_wiener(X[0], V, V[0], **KW)),                     # ... or broadcast beyond the mixture
    (ValueError, lambda: si.consistent_wiener(X[0, 0], V[0, 0], V[0, 0], **KW)),
    (ValueError, lambda: si.consistent_wiener(X, V, V, gamma=0.0, **KW)),
    (ValueError, lambda: si.consistent_wiener(X, V, V, gamma=-1.0, **KW)),
    (ValueError, lambda: si.consistent_wiener(X, V, V, gamma=float("inf"), **KW)),
    (ValueError, lambda: si.consistent_wiener(X, V, V, gamma=float("nan"), **KW)),
    (ValueError, lambda: si.consistent_wiener(X, V, V, floor=0.0, **KW)),
    (ValueError, lambda: si.consistent_wiener(X, V, V, floor=1.0, **KW)),
    (ValueError, lambda: si.consistent_wiener(X, V, V, n_iter=-1, **KW)),
    (ValueError, lambda: si.consistent_wiener(X, V, V, n_iter=2.5, **KW)),
    (ValueError, lambda: si.consistent_wiener(X, V, V, tol=-1e-3, **KW)),
    (ValueError, lambda: si.consistent_wiener(X, V, V, eva_iter=0, **KW)),
    (NotImplementedError, lambda: si.consistent_wiener(X, V, V, onesided=False, **KW)),
    (NotImplementedError, lambda: si.consistent_wiener(X, V, V, hop_length=16, window=torch.hann_window(64) + 0j)),
    (NotImplementedError, lambda: si.consistent_wiener(X.clone().requires_grad_(), V, V, **KW)),
    (NotImplementedError, lambda: si.consistent_wiener(X, V.clone().requires_grad_(), V, **KW)),
    (TypeError, lambda: si.consistent_wiener_audio([0.0], V, V, 64, **KW)),
    (ValueError, lambda: si.consistent_wiener_audio(torch.zeros(64), V, V, 64, gamma=0.0, **KW)),
    (NotImplementedError, lambda: si.consistent_wiener_audio(torch.zeros(64, requires_grad=True), V, V, 64, **KW)),
]


@pytest.mark.parametrize("exc,call", BAD, ids=[str(i) for i in range(len(BAD))])
def test_argument_errors_are_raised_without_a_device(exc, call):
    with pytest.raises(exc):
        call()


def test_an_empty_batch_needs_no_device():
    S, N, info = si.consistent_wiener(X[:0], V[:0], V[:0], return_info=True, **KW)
    assert S.shape == N.shape == (0, 33, 5) and S.dtype == torch.complex64
    assert info["n_iter"] == 0 and info["residual"].shape == (0,)


def test_abi_argument_errors_do_not_need_a_gpu():
    build.build_lib()
    lib = _lib.load()
    buf = (C.c_char * 256)()
    base = (C.addressof(buf) + 15) & ~15
    a, b, c, d, e = (C.c_void_p(base + 32 * i) for i in range(5))
    run = lib.specinv_cwf_run

    def err(*args):
        assert run(*args) == _lib.EINVAL
        return lib.specinv_last_error()

    assert b"NULL mix" in err(None, None, b, c, 1.0, 1, 1e-8, 1, 1, 0.0, d, e, None, None)
    assert b"NULL N_out" in err(None, a, b, c, 1.0, 1, 1e-8, 1, 1, 0.0, d, None, None, None)
    assert b"alias" in err(None, a, b, c, 1.0, 1, 1e-8, 1, 1, 0.0, d, d, None, None)
    assert b"alias" in err(None, a, b, c, 1.0, 1, 1e-8, 1, 1, 0.0, a, e, None, None)
    assert b"aligned" in err(None, a, b, C.c_void_p(base + 72), 1.0, 1, 1e-8, 1, 1, 0.0, d, e, None, None)
    assert b"gamma" in err(None, a, b, c, 0.0, 1, 1e-8, 1, 1, 0.0, d, e, None, None)
    assert b"gamma" in err(None, a, b, c, float("inf"), 1, 1e-8, 1, 1, 0.0, d, e, None, None)
    assert b"floor" in err(None, a, b, c, 1.0, 1, 1.0, 1, 1, 0.0, d, e, None, None)
    assert b"n_iter" in err(None, a, b, c, 1.0, 1, 1e-8, -1, 1, 0.0, d, e, None, None)
    assert b"eva_iter" in err(None, a, b, c, 1.0, 1, 1e-8, 1, 0, 0.0, d, e, None, None)
    assert b"tol" in err(None, a, b, c, 1.0, 1, 1e-8, 1, 1, float("nan"), d, e, None, None)
    assert b"plan is NULL" in err(None, a, b, c, 1.0, 1, 1e-8, 1, 1, 0.0, d, e, None, None)
