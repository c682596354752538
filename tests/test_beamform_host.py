"""Mask-based beamforming without a GPU: properties of the float64 definition (tests/_beamform_oracle.py), the argument errors of
the Python layer, and two kinds of recorded figures.

1. Order sensitivity on the GPU test's inputs (tests/_beamform_inputs.py): d = (d_Y, d_w, d_Phi), the relative L2 distance
   between the oracle as written and the same oracle with reversed frame sums and a Cholesky solve.  test_order_sensitivity_table
   prints every case; _beamform_inputs.D_MEASURED holds them.  With at least as many frames as channels d stays below 1e-14; on
   the rank-deficient shapes (8 channels x 5 frames, 16 x 3, 2 x 1) at diag_load = 1e-7 d_w is 4e-10 ... 9e-9.  No case may exceed
   1e-6 in d_Y or d_w: beyond that a case would test its own conditioning and not the kernel.  The device tolerance is
   100 x max(d, 2^-53) (tests/test_gpu_beamform.py).

2. Quality, on 2 s of chirping harmonics with pauses at 16 kHz on a 4-microphone line array (whole-sample delays), with spatially
   white noise and one directional white-noise source, analysed 512 / 128: SNR = |S_ref|^2 / |Y - S_ref|^2 over all bins and
   frames, S_ref the source's image at the reference channel, so that distortion of the target counts against the result.  The
   reference channel itself is at 3.04 dB.  Measured with the float64 definition (test_quality_figure, QUALITY):

       solution     ideal ratio mask     spectral_gain's mask (the definition of tests/_enhance_oracle.py)
       souden       15.92 dB              9.17 dB
       rtf_power    15.04 dB              3.98 dB
       mwf          13.24 dB              8.68 dB
   (rtf_power with the estimated mask barely beats the reference channel at the default of three power iterations: they are too
   few there.  Measured on the same scene: n_power_iter 1, 3, 10, 50 give 3.47, 3.98, 8.82, 10.73 dB.)
"""
import numpy as np
import pytest
import torch

import _beamform_inputs as bi
import _beamform_oracle as bo
import _enhance_inputs as ei
import _enhance_oracle as eo
import spectrogram_inversion_amd as si


def _cg(rng, *shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0)


# ------------------------------------------------------------------------------------------------ the definition's properties

@pytest.mark.parametrize("C", (1, 2, 5))
def test_souden_and_rtf_power_coincide_and_are_distortionless_on_a_rank_one_target(C):
    rng = np.random.default_rng(C)
    a = _cg(rng, C)
    Ps = 2.5 * np.outer(a, a.conj())
    B = _cg(rng, C, C + 3)
    Pn = B @ B.conj().T / (C + 3)
    for ref in (0, C - 1):
        ws = bo.weights(Ps, Pn, "souden", ref, diag_load=0.0)
        wr = bo.weights(Ps, Pn, "rtf_power", ref, diag_load=0.0, n_power_iter=3)
        assert np.abs(np.vdot(ws, a) - a[ref]) <= 1e-12 * np.abs(a).max()          # w^H a = a_ref
        assert np.abs(np.vdot(wr, a) - a[ref]) <= 1e-12 * np.abs(a).max()
        assert np.linalg.norm(ws - wr) <= 1e-12 * np.linalg.norm(ws)


def test_mwf_without_noise_weight_is_the_reference_channel():
    rng = np.random.default_rng(4)
    B = _cg(rng, 4, 9)
    Ps = B @ B.conj().T / 9
    Pn = np.eye(4)
    for ref in range(4):
        w = bo.weights(Ps, Pn, "mwf", ref, diag_load=0.0, mu=0.0)
        assert np.linalg.norm(w - np.eye(4)[ref]) <= 1e-12


@pytest.mark.parametrize("solution", bo.SOLUTIONS)
def test_zero_cases_give_exact_zeros_and_no_nan(solution):
    rng = np.random.default_rng(5)
    X = _cg(rng, 3, 3, 20)
    X[:, 1] = 0.0
    m = rng.random((3, 20))
    Y, w, Ps, Pn = bo.beamform(X, m, solution=solution)
    assert not Y[1].any() and not w[1].any() and not Ps[1].any() and not Pn[1].any() and Y[0].any()
    for arr in bo.beamform(np.zeros_like(X), m, solution=solution) + bo.beamform(X, np.zeros_like(m), solution=solution)[:3]:
        assert not arr.any()
    for arr in (Y, w, Ps, Pn) + bo.beamform(X, np.zeros_like(m), solution=solution):
        assert np.isfinite(arr).all()
    Y, w, Ps, Pn = bo.beamform(X[:, :, :0], m[:, :0], solution=solution)                # no frames
    assert Y.shape == (3, 0) and not w.any() and not Ps.any() and not Pn.any()


def test_covariances_are_hermitian_and_normalised():
    rng = np.random.default_rng(6)
    X = _cg(rng, 4, 2, 30)
    m = rng.random((2, 30))
    _, _, Ps, Pn = bo.beamform(X, m)
    for P in (Ps, Pn):
        assert np.abs(P - P.conj().swapaxes(-1, -2)).max() <= 4 * np.finfo(np.float64).eps * np.abs(P).max()
        assert (np.linalg.eigvalsh(P) >= -1e-12).all()
    ones = bo.covariance(X[:, 0], np.ones(30))
    assert np.allclose(ones, X[:, 0] @ X[:, 0].conj().T / 30, rtol=1e-13, atol=0)
    assert np.allclose(bo.covariance(X[:, 0], 3.0 * m[0]), bo.covariance(X[:, 0], m[0]), rtol=1e-13, atol=0)      # a mask's scale cancels


def test_power_iteration_finds_the_principal_eigenvector():
    rng = np.random.default_rng(8)
    a = _cg(rng, 4)
    B = _cg(rng, 4, 40)
    Ps = 4.0 * np.outer(a, a.conj()) + 0.05 * (B @ B.conj().T / 40)
    Pn = np.eye(4)
    w = bo.weights(Ps, Pn, "rtf_power", 0, diag_load=0.0, n_power_iter=30)
    assert np.abs(np.vdot(w, a) - a[0]) <= 0.05 * np.abs(a[0])


# ------------------------------------------------------------------------------------------------ the Python layer's errors

def _spec(*shape, dtype=torch.complex64):
    return torch.zeros(shape, dtype=dtype)


def test_argument_errors_need_no_gpu():
    m = torch.ones(3, 8)
    with pytest.raises(TypeError, match="spec must be a torch.Tensor"):
        si.beamform(np.zeros((2, 3, 8), dtype=np.complex64), m)
    with pytest.raises(TypeError, match="complex64 or complex128"):
        si.beamform(torch.zeros(2, 3, 8), m)
    with pytest.raises(TypeError, match="complex64 or complex128"):
        si.spatial_covariance(torch.zeros(2, 3, 8, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"\(F, T\), \(C, F, T\)"):
        si.beamform(_spec(8), m)
    with pytest.raises(ValueError, match=r"\(F, T\), \(C, F, T\)"):
        si.beamform_apply(_spec(1, 2, 2, 3, 8), torch.zeros(3, 2, dtype=torch.complex128))
    with pytest.raises(NotImplementedError, match="channels must be <= 16"):
        si.beamform(_spec(17, 3, 8), m)
    with pytest.raises(NotImplementedError, match="channels must be <= 16"):
        si.spatial_covariance(_spec(2, 17, 3, 8))
    with pytest.raises(NotImplementedError, match="channels must be <= 16"):
        si.beamform_audio(torch.zeros(17, 4000), 512)
    with pytest.raises(NotImplementedError, match="not differentiable"):
        si.beamform(_spec(2, 3, 8).requires_grad_(), m)
    with pytest.raises(NotImplementedError, match="not differentiable"):
        si.beamform(_spec(2, 3, 8), m.clone().requires_grad_())
    with pytest.raises(NotImplementedError, match="not differentiable"):
        si.beamform_apply(_spec(2, 3, 8), torch.zeros(3, 2, dtype=torch.complex128, requires_grad=True))
    with pytest.raises(NotImplementedError, match="not differentiable"):
        si.beamform_audio(torch.zeros(2, 4000, requires_grad=True), 512)
    with pytest.raises(TypeError, match="mask_target must be a torch.Tensor"):
        si.beamform(_spec(2, 3, 8), None)
    with pytest.raises(TypeError, match="mask_noise must be real"):
        si.beamform(_spec(2, 3, 8), m, torch.ones(3, 8, dtype=torch.complex64))
    with pytest.raises(TypeError, match="mask must be real"):
        si.spatial_covariance(_spec(2, 3, 8), torch.ones(3, 8, dtype=torch.int32))
    with pytest.raises(ValueError, match="does not broadcast"):
        si.beamform(_spec(2, 3, 8), torch.ones(2, 3, 8))                  # (C, F, T): the channel axis is not part of a mask
    with pytest.raises(ValueError, match="does not broadcast"):
        si.beamform(_spec(2, 3, 8), m, torch.ones(4, 8))
    with pytest.raises(ValueError, match="mask_target must be non-negative"):
        si.beamform(_spec(2, 3, 8), -m)
    with pytest.raises(ValueError, match="mask_noise must be non-negative"):
        si.beamform(_spec(2, 3, 8), m, torch.full((3, 1), float("nan")))
    with pytest.raises(ValueError, match="solution must be one of"):
        si.beamform(_spec(2, 3, 8), m, solution="gev")
    with pytest.raises(ValueError, match=r"ref_channel must be in \[0, 2\)"):
        si.beamform(_spec(2, 3, 8), m, ref_channel=2)
    with pytest.raises(ValueError, match=r"ref_channel must be in \[0, 1\)"):
        si.beamform(_spec(3, 8), m, ref_channel=-1)
    with pytest.raises(TypeError, match="ref_channel must be an int"):
        si.beamform(_spec(2, 3, 8), m, ref_channel=torch.tensor([0, 1]))
    with pytest.raises(ValueError, match=r"ref_channel must be in \[0, 2\)"):
        si.beamform_audio(torch.zeros(2, 4000), 512, ref_channel=5)
    with pytest.raises(ValueError, match="n_power_iter must be an int >= 1"):
        si.beamform(_spec(2, 3, 8), m, solution="rtf_power", n_power_iter=0)
    with pytest.raises(NotImplementedError, match="n_power_iter must be <= 64"):
        si.beamform(_spec(2, 3, 8), m, solution="rtf_power", n_power_iter=65)
    with pytest.raises(ValueError, match="diag_load must be"):
        si.beamform(_spec(2, 3, 8), m, diag_load=-1.0)
    with pytest.raises(ValueError, match="mu must be"):
        si.beamform(_spec(2, 3, 8), m, solution="mwf", mu=float("inf"))
    with pytest.raises(TypeError, match="weights must be complex64 or complex128"):
        si.beamform_apply(_spec(2, 3, 8), torch.zeros(3, 2))
    with pytest.raises(ValueError, match="weights must be of shape"):
        si.beamform_apply(_spec(2, 3, 8), torch.zeros(2, 3, dtype=torch.complex128))
    with pytest.raises(ValueError, match=r"\(C, L\)"):
        si.beamform_audio(torch.zeros(4000), 512)


def test_empty_input_needs_no_gpu():
    y, w, ps, pn = si.beamform(_spec(0, 2, 3, 8), torch.ones(3, 8), return_weights=True, return_scm=True)
    assert y.shape == (0, 3, 8) and y.dtype == torch.complex64 and w.shape == (0, 3, 2) and w.dtype == torch.complex128
    assert ps.shape == pn.shape == (0, 3, 2, 2) and ps.dtype == torch.complex128
    y, w = si.beamform(_spec(2, 3, 0, dtype=torch.complex128), torch.ones(3, 0), return_weights=True)      # T = 0: zeros
    assert y.shape == (3, 0) and y.dtype == torch.complex128 and w.shape == (3, 2) and not w.any()
    assert si.spatial_covariance(_spec(3, 0)).shape == (3, 1, 1)
    assert si.beamform_apply(_spec(2, 3, 0), torch.zeros(3, 2, dtype=torch.complex128)).shape == (3, 0)


def test_entry_argument_errors_do_not_need_a_gpu():
    """specinv_beamform's checks, in the header's order, on pointers that are never read"""
    from spectrogram_inversion_amd import _lib, build
    build.build_lib()
    lib = _lib.load()
    p = [0x1000 * (i + 1) for i in range(8)]       # spec, mask_target, mask_noise, weights_in, out, weights_out, scm_target, scm_noise

    def call(ptrs, batch=1, channels=2, n_freq=5, n_frames=7, solution=0, ref=0, n_power=3, load=1e-7, mu=1.0, dtype=_lib.F32):
        return lib.specinv_beamform(*ptrs, batch, channels, n_freq, n_frames, solution, ref, n_power, load, mu, dtype, 0, None)

    def fails(code, word, ptrs, **kw):
        assert call(ptrs, **kw) == code, (word, kw)
        assert word in lib.specinv_last_error(), (word, kw, lib.specinv_last_error())

    estimate = [p[0], p[1], p[2], None, p[4], p[5], p[6], p[7]]
    apply = [p[0], None, None, p[3], p[4], None, None, None]
    # the pointers and the mode rules (each with batch = 0 as well: a later check must not answer first)
    for kw in ({}, {"batch": 0}):
        fails(_lib.EINVAL, b"NULL spec", [None] + estimate[1:], **kw)
        for i in (1, 2, 5, 6, 7):                                # weights_in with a mask, weights_out or a covariance
            fails(_lib.EINVAL, b"with weights_in given nothing is estimated", apply[:i] + [p[i]] + apply[i + 1:], **kw)
        fails(_lib.EINVAL, b"with weights_in given nothing is estimated", apply[:4] + [None] * 4, **kw)      # ... or without out
        fails(_lib.EINVAL, b"no result is asked for", estimate[:4] + [None] * 4, **kw)
        fails(_lib.EINVAL, b"weights need mask_target", [p[0], None, p[2], None, p[4], None, p[6], p[7]], **kw)
        fails(_lib.EINVAL, b"weights need mask_target", [p[0], None, None, None, None, p[5], None, None], **kw)
        fails(_lib.EINVAL, b"out must not alias spec", estimate[:4] + [p[0]] + estimate[5:], **kw)
        fails(_lib.EINVAL, b"out must not alias weights_in", apply[:4] + [p[3]] + apply[5:], **kw)
        fails(_lib.EINVAL, b"weights_out must not alias mask_target", estimate[:5] + [p[1]] + estimate[6:], **kw)
        fails(_lib.EINVAL, b"scm_target must not alias out", estimate[:6] + [p[4], p[7]], **kw)
        fails(_lib.EINVAL, b"scm_noise must not alias scm_target", estimate[:7] + [p[6]], **kw)
    # the numbers, in the header's order; n_power_iter = 65 (the last check, EUNSUPPORTED) rides along and must not answer first
    numbers = (({"batch": 0}, b"must be >= 1"), ({"channels": 0}, b"must be >= 1"), ({"n_freq": 0}, b"must be >= 1"),
               ({"n_frames": 0}, b"must be >= 1"), ({"batch": 1 << 40, "n_freq": 1 << 20}, b"are too many"),
               ({"solution": 3}, b"unknown solution 3"), ({"solution": -1}, b"unknown solution -1"),
               ({"ref": -1}, b"ref_channel must be in [0, 2)"), ({"ref": 2}, b"ref_channel must be in [0, 2)"),
               ({"load": -1.0}, b"diag_load and mu"), ({"load": float("nan")}, b"diag_load and mu"),
               ({"mu": float("inf")}, b"diag_load and mu"), ({"mu": -1e-3}, b"diag_load and mu"), ({"dtype": 7}, b"bad dtype 7"))
    for ptrs in (estimate, apply):
        for kw, word in numbers:
            fails(_lib.EINVAL, word, ptrs, **kw)
            fails(_lib.EINVAL, word, ptrs, **{"n_power": 65, **kw})
        fails(_lib.EINVAL, b"n_power_iter must be >= 1", ptrs, n_power=0)
        fails(_lib.EUNSUPPORTED, b"channels must be <= 16", ptrs, channels=17)
        fails(_lib.EUNSUPPORTED, b"channels must be <= 16", ptrs, channels=17, n_power=65)
        fails(_lib.EUNSUPPORTED, b"n_power_iter must be <= 64", ptrs, n_power=65)


# ------------------------------------------------------------------------------------------------ recorded figures

def test_order_sensitivity_table():
    """Prints d = (d_Y, d_w, d_Phi) for every case and holds _beamform_inputs.D_MEASURED to a fresh measurement from above only:
    a fresh d is at most 4 times the recorded one (LAPACK builds and their threading differ in the last bits, and these are
    rounding-noise quantities), so that the device tolerance never rests on a d understated by more than that.  A fresh d below
    the recorded one is not an error.  No case may exceed 1e-6 in d_Y or d_w."""
    fresh = {}
    for name in bi.NAMES:
        fresh[name] = bi.measure(name)
        print(f'    "{name}": ({fresh[name][0]:.1e}, {fresh[name][1]:.1e}, {fresh[name][2]:.1e}),   # {bi.BY_NAME[name][1]}')
    assert set(bi.D_MEASURED) == set(bi.NAMES)
    for name in bi.NAMES:
        for got, rec in zip(fresh[name], bi.D_MEASURED[name]):
            assert max(got, bi.FLOOR) <= 4 * max(rec, bi.FLOOR), (name, got, rec)
        assert fresh[name][0] <= 1e-6 and fresh[name][1] <= 1e-6, (name, fresh[name])
        assert all(np.isfinite(r).all() for r in bi.oracle(name))


def test_the_cases_cover_the_kernel_edges():
    import importlib
    bf = importlib.import_module("spectrogram_inversion_amd.beamform")       # (the package's `beamform` is the function)
    assert bf.TILE == bi.TILE and bf.MAX_CHANNELS == 16 and set(bf.SOLUTIONS) == set(bo.SOLUTIONS)
    shapes = {c[2]["shape_name"]: c[1] for c in bi.CASES}
    assert {s[3] for s in shapes.values()} >= {1, bi.TILE - 1, bi.TILE, bi.TILE + 1, 2 * bi.TILE + 2}
    assert {s[1] for s in shapes.values()} >= {1, 2, 3, 8, 9, 16}
    assert shapes["c8_t5"][1:] == (8, 2, 5) and shapes["c16_t3"][1:] == (16, 1, 3) and shapes["f1"][2] == 1
    assert bi.make_masks("mask_profile-mwf")[0].shape == (3, 1) and not bi.make_masks("zero_mask-mwf")[0].any()
    assert bi.make_masks("noise_given-mwf")[1] is not None and bi.make_masks("c8-mwf")[1] is None
    assert not bi.make_input("batch3_zero_item-mwf")[1].any() and not bi.make_input("c1-mwf")[:, :, 1].any()


def _array_scene(seed=3):
    """(source image, noise), each (4, L): a voiced source and a white-noise interferer on a line array with whole-sample delays
    between neighbouring microphones (1 and -2 samples), plus spatially white noise"""
    n = 2 * ei.SR
    s = ei.voice(n + 16, seed)
    v = ei.white(n + 16, seed + 1, 0.5)
    src = np.stack([s[8 + 1 * c: 8 + 1 * c + n] for c in range(4)])
    itf = np.stack([v[8 - 2 * c: 8 - 2 * c + n] for c in range(4)])
    amb = np.stack([ei.white(n, seed + 2 + c, 0.25) for c in range(4)])
    return src, itf + amb


def _cov_fast(X, m):
    """Phi(m) (F, C, C) of X (C, F, T) as one contraction (the same definition; the quality figure needs no particular order)"""
    return np.einsum("ft,cft,dft->fcd", m, X, X.conj()) / np.maximum(m.sum(-1), bo.TINY)[:, None, None]


def quality(ref=0):
    """{"ref": SNR of the reference channel, (solution, mask kind): SNR of the result}, in dB"""
    src, noise = _array_scene()
    S = np.stack([ei.stft(c) for c in src])
    N = np.stack([ei.stft(c) for c in noise])
    X = S + N
    snr = lambda Y: float(10 * np.log10(np.sum(np.abs(S[ref]) ** 2) / np.sum(np.abs(Y - S[ref]) ** 2)))      # noqa: E731
    masks = {"ideal": np.abs(S[ref]) ** 2 / np.maximum(np.abs(S[ref]) ** 2 + np.abs(N[ref]) ** 2, bo.TINY),
             "spectral_gain": eo.enhance(eo.power(X[ref]))["gain"]}
    out = {"ref": snr(X[ref])}
    for kind, m in masks.items():
        Ps, Pn = _cov_fast(X, m), _cov_fast(X, 1.0 - m)
        for solution in bo.SOLUTIONS:
            w = np.stack([bo.weights(Ps[f], Pn[f], solution, ref) for f in range(X.shape[1])])
            out[(solution, kind)] = snr(np.einsum("fc,cft->ft", w.conj(), X))
    return out


# SNR in dB, measured by test_quality_figure
QUALITY = {"ref": 3.04, ("souden", "ideal"): 15.92, ("rtf_power", "ideal"): 15.04, ("mwf", "ideal"): 13.24,
           ("souden", "spectral_gain"): 9.17, ("rtf_power", "spectral_gain"): 3.98, ("mwf", "spectral_gain"): 8.68}


def test_quality_figure():
    """Every solution, with the ideal ratio mask and with spectral_gain's mask, must beat the reference channel; the figures are
    printed and recorded in QUALITY and the README, no threshold is taken from elsewhere."""
    q = quality()
    for k, v in q.items():
        print(f"beamform quality, {k}: {v:.2f} dB")
    for k, v in q.items():
        if k != "ref":
            assert v > q["ref"], (k, v, q["ref"])
