"""wpe, wpe_apply and dereverb on the device, against the float64 definition (tests/_wpe_oracle.py) on the cases of
tests/_wpe_inputs.py (listed and motivated there; none is larger than 5 bins x 200 frames).

Tolerances.  complex128: relative L2 per item, 100 x max(d, 2^-53), with d the order sensitivity of the definition itself that
tests/test_wpe_host.py measures for that case and quantity (Y, G, lam; _wpe_inputs.D_MEASURED: from 2e-16 to 3e-9, the latter on
the one-channel prototype shape whose R has a condition number of 3e8).  A tree-shaped float64 sum and a different elimination
order (U D U^H on the device, LU in the oracle) move the result by a small multiple of what a reversed sum does; an indexing or
halo mistake shows at 1e-3 or above.  complex64: every element of Y within one float32 rounding of the oracle's value on the same
float32 input, 2^-23 max(|X|, |Y|) element-wise, plus the float64 bound scaled the same way, element by element (the bound times
max(|X|, |Y|): 2.9e-7 of the element on the one-channel prototype, 1e-11 or less elsewhere); G and lam, float64 from the float32
input, are held to the float64 bounds.

Bit for bit: wpe_apply(X, G, delay) is Y; item b of a batch is the item alone; dereverb is the composition of stft, wpe and istft."""
import importlib

import numpy as np
import pytest
import torch

import _wpe_inputs as wi
import spectrogram_inversion_amd as si

dv = importlib.import_module("spectrogram_inversion_amd.dereverb")      # (the package's `dereverb` is the function)

pytestmark = pytest.mark.gpu

DEV = "cuda"
KINDS = ("complex128", "complex64")


def _options(name):
    opt = wi.BY_NAME[name][2]
    kw = dict(taps=opt["taps"], delay=opt["delay"], n_iter=opt["n_iter"], psd_context=opt["psd_context"])
    p = wi.make_power(name)
    if p is not None:
        kw["power"] = torch.from_numpy(p).to(DEV)
    return kw


def _input(name, kind):
    X = wi.make_input(name)
    return X.astype(np.complex64) if kind == "complex64" else X


def _check(name, kind, Y, G, lam, what=""):
    """device results (B, C, F, T), (B, F, C, K, C), (B, F, T) against the oracle"""
    X = _input(name, kind)
    wY, wG, wlam = wi.oracle(name, single=kind == "complex64")
    tY, tG, tlam = wi.tolerances(name)
    Y, G, lam = Y.cpu().numpy(), G.cpu().numpy(), lam.cpu().numpy()
    assert Y.shape == wY.shape and G.shape == wG.shape and lam.shape == wlam.shape, (name, Y.shape, G.shape, lam.shape)
    assert Y.dtype == X.dtype and G.dtype == np.complex128 and lam.dtype == np.float64
    assert np.isfinite(Y).all() and np.isfinite(G).all() and np.isfinite(lam).all(), name
    for b in range(X.shape[0]):
        eY, eG, el = wi.rel_l2(Y[b], wY[b]), wi.rel_l2(G[b], wG[b]), wi.rel_l2(lam[b], wlam[b])
        print(f"{name}{what} {kind} item {b}: Y {eY:.2e} (tol {tY:.1e}), G {eG:.2e} (tol {tG:.1e}), lam {el:.2e} (tol {tlam:.1e})")
        if kind == "complex128":
            assert eY <= tY, (name, b, eY, tY)
        else:
            allowed = (2.0 ** -23 + tY) * np.maximum(np.abs(X[b]), np.abs(wY[b]))
            err = np.abs(Y[b].astype(np.complex128) - wY[b])
            assert (err <= allowed).all(), (name, b, float((err - allowed).max()))
        assert eG <= tG, (name, b, eG, tG)
        assert el <= tlam, (name, b, el, tlam)


def test_constants():
    assert dv.TILE_FRAMES == wi.TILE and dv.MAX_UNKNOWNS == 64


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", wi.NAMES)
def test_against_the_oracle(name, kind):
    X = torch.from_numpy(_input(name, kind)).to(DEV)
    Y, G, lam = si.wpe(X, return_filter=True, return_power=True, **_options(name))
    _check(name, kind, Y, G, lam)
    # the filter-only mode: the same bits
    assert torch.equal(si.wpe_apply(X, G, wi.BY_NAME[name][2]["delay"]), Y)
    # without the extras: the same Y
    assert torch.equal(si.wpe(X, **_options(name)), Y)


def test_silence_and_zero_items_are_exact_zeros():
    name = "batch3_zero_item"
    X = torch.from_numpy(wi.make_input(name)).to(DEV)
    Y, G, lam = si.wpe(X, return_filter=True, return_power=True, **_options(name))
    assert not Y[1].any() and not G[1].any() and not Y[:, :, 1].any() and not G[:, 1].any()
    assert torch.isfinite(lam).all() and (lam[1] == np.finfo(np.float64).tiny).all()


@pytest.mark.parametrize("kind", KINDS)
def test_an_item_of_a_batch_is_the_item_alone(kind):
    name = "batch3_zero_item"
    X = torch.from_numpy(_input(name, kind)).to(DEV)
    kw = _options(name)
    Y, G, lam = si.wpe(X, return_filter=True, return_power=True, **kw)
    for b in range(X.shape[0]):
        y1, g1, l1 = si.wpe(X[b:b + 1], return_filter=True, return_power=True, **kw)
        assert torch.equal(y1[0], Y[b]) and torch.equal(g1[0], G[b]) and torch.equal(l1[0], lam[b])
        y3, g3, l3 = si.wpe(X[b], return_filter=True, return_power=True, **kw)         # (C, F, T): the channels of one recording
        assert torch.equal(y3, Y[b]) and torch.equal(g3, G[b]) and torch.equal(l3, lam[b])


def test_two_dimensional_input_is_one_channel():
    name = "proto_c1"
    X = torch.from_numpy(wi.make_input(name)).to(DEV)
    kw = _options(name)
    Y, G, lam = si.wpe(X, return_filter=True, return_power=True, **kw)
    y2, g2, l2 = si.wpe(X[0, 0], return_filter=True, return_power=True, **kw)
    assert y2.shape == X.shape[2:] and g2.shape == (X.shape[2], 1, kw["taps"], 1) and l2.shape == X.shape[2:]
    assert torch.equal(y2, Y[0, 0]) and torch.equal(g2, G[0]) and torch.equal(l2, lam[0])
    assert torch.equal(si.wpe_apply(X[0, 0], g2, kw["delay"]), y2)


@pytest.mark.parametrize("kind", KINDS)
def test_strided_offset_and_conjugated_inputs(kind):
    name = "proto_c2"
    x = _input(name, kind)
    X = torch.from_numpy(x).to(DEV)
    kw = _options(name)
    want = si.wpe(X, return_filter=True, return_power=True, **kw)
    _check(name, kind, *want)
    # frames on a stride of 2 with an offset, bins and channels transposed in memory
    big = torch.zeros(x.shape[0], x.shape[2], x.shape[1], 2 * x.shape[3] + 1, dtype=X.dtype, device=DEV)
    big[..., 1::2] = X.transpose(1, 2)
    strided = big[..., 1::2].transpose(1, 2)
    assert not strided.is_contiguous() and strided.storage_offset() == 1
    lazy = torch.from_numpy(x.conj()).to(DEV).conj()
    assert lazy.is_conj()
    for view in (strided, lazy):
        got = si.wpe(view, return_filter=True, return_power=True, **kw)
        assert all(torch.equal(g, w) for g, w in zip(got, want))
        assert torch.equal(si.wpe_apply(view, want[1], kw["delay"]), want[0])


def test_power_broadcasts_and_cpu_tensors_come_back():
    name = "power_given"
    X = torch.from_numpy(wi.make_input(name)).to(DEV)
    kw = _options(name)
    want = si.wpe(X, **kw)
    assert torch.equal(si.wpe(X, **dict(kw, power=kw["power"][None].float().double())),
                       si.wpe(X, **dict(kw, power=kw["power"].float())))      # (1, F, T) float64 and (F, T) float32: the same values
    prof = kw["power"][:, :1]                                       # an (F, 1) profile
    assert torch.equal(si.wpe(X, **dict(kw, power=prof)), si.wpe(X, **dict(kw, power=prof.expand(-1, X.shape[-1]).contiguous())))
    got = si.wpe(X.cpu(), **dict(kw, power=kw["power"].cpu()))
    assert got.device.type == "cpu" and torch.equal(got, want.cpu())


def test_a_delay_beyond_the_frames_and_a_context_beyond_them():
    X = torch.from_numpy(wi.make_input("f1")).to(DEV)
    assert torch.equal(si.wpe(X, taps=4, delay=10 ** 12, n_iter=2), X)
    assert X.shape[-1] < dv.MAX_CONTEXT                   # (every frame's window is then the whole bin)
    assert torch.equal(si.wpe(X, taps=4, delay=3, n_iter=2, psd_context=dv.MAX_CONTEXT),
                       si.wpe(X, taps=4, delay=3, n_iter=2, psd_context=X.shape[-1]))


@pytest.mark.parametrize("dtype", (torch.float32, torch.float64))
def test_dereverb_is_the_composition(dtype):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 4000, generator=g, dtype=dtype).to(DEV)
    kw = dict(hop_length=64, window=torch.hann_window(256, dtype=dtype, device=DEV))
    got = si.dereverb(x, 256, taps=5, delay=2, n_iter=2, **kw)
    X = si.stft(x.reshape(6, -1), 256, **kw)
    Y = si.wpe(X.reshape(2, 3, *X.shape[-2:]), taps=5, delay=2, n_iter=2)
    want = si.istft(Y.reshape(6, *Y.shape[-2:]), **kw).reshape(2, 3, -1)
    assert got.shape == want.shape and got.dtype == dtype and torch.equal(got, want)
    assert not torch.equal(got, x[..., :got.shape[-1]])
    one = si.dereverb(x[0], 256, taps=5, delay=2, n_iter=2, **kw)                    # (C, L): one recording
    assert torch.equal(one, got[0])
    mono = si.dereverb(x[0, 0], 256, taps=5, delay=2, n_iter=2, **kw)
    assert mono.shape == got.shape[-1:] and torch.isfinite(mono).all()
