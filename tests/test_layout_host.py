"""`_ingest.ingest`, the one door between a caller's tensor and a kernel's pointer, on every layout of tests/_layouts.py: no GPU
and no native library needed (the helper is torch alone)."""
import pytest
import torch

import _layouts
from spectrogram_inversion_amd._ingest import ingest

DTYPES = [torch.float32, torch.float64, torch.complex64, torch.complex128]
CASES = [(d, n) for d in DTYPES for n in _layouts.builders(d)]
CPU = torch.device("cpu")


def _dense(dtype, shape=(2, 5, 7)):
    g = torch.Generator().manual_seed(3)
    z = torch.randn(shape, dtype=dtype, generator=g)
    return z


def _is_kernel_ready(t, dtype):
    return (t.dtype == dtype and t.is_contiguous() and not t.is_conj() and not t.is_neg() and not t.requires_grad
            and t.data_ptr() % 16 == 0 and t.device == CPU)


@pytest.mark.parametrize("dtype,name", CASES, ids=[f"{str(d)[6:]}-{n}" for d, n in CASES])
def test_ingest_gives_the_dense_values(dtype, name):
    Z = _dense(dtype)
    if name == "expanded":
        Z = _layouts.repeated(Z)
    view, base = _layouts.build(name, Z)
    before = base.clone()
    out = ingest(view, CPU, dtype)
    assert _is_kernel_ready(out, dtype)
    assert out.shape == Z.shape and torch.equal(out, Z)
    assert torch.equal(base, before) and base.is_conj() == before.is_conj()
    twin = _layouts.dense_twin(view, Z)
    assert ingest(twin, CPU, dtype) is twin


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
def test_dense_aligned_tensor_is_returned_itself(dtype):
    Z = _dense(dtype)
    assert ingest(Z, CPU, dtype) is Z
    flat = Z.reshape(-1)                                           # (a view of the same aligned memory: still no copy)
    assert ingest(flat, CPU, dtype) is flat
    empty = torch.empty((0, 3), dtype=dtype)
    assert ingest(empty, CPU, dtype) is empty


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
def test_requires_grad_comes_back_detached(dtype):
    Z = _dense(dtype).requires_grad_()
    out = ingest(Z, CPU, dtype)
    assert out is not Z and not out.requires_grad and out.grad_fn is None
    assert _is_kernel_ready(out, dtype) and torch.equal(out, Z.detach())
    assert out.data_ptr() == Z.data_ptr()                          # (detached, not copied)
    y = (Z * 2).conj() if dtype.is_complex else Z * 2              # a non-leaf, with the bit where there is one
    out = ingest(y, CPU, dtype)
    assert _is_kernel_ready(out, dtype) and torch.equal(out, y.detach().resolve_conj())


@pytest.mark.parametrize("src,dst", [(torch.float64, torch.float32), (torch.complex128, torch.complex64),
                                     (torch.float16, torch.float32), (torch.complex64, torch.complex128)])
def test_dtype_change_resolves_the_bits_too(src, dst):
    Z = _dense(torch.complex128 if src.is_complex else torch.float64).to(src)
    for name in _layouts.builders(src):
        if src == torch.float16 and name == "neg":
            continue                                               # (no complex32 arithmetic on the CPU to build it from)
        Zn = _layouts.repeated(Z) if name == "expanded" else Z
        view, _ = _layouts.build(name, Zn)
        out = ingest(view, CPU, dst)
        assert _is_kernel_ready(out, dst) and torch.equal(out, Zn.to(dst)), name


def test_the_old_chain_kept_the_conjugate_bit():
    """What the helper replaces, `t.detach().to(device, dtype).contiguous()` behind an `is_contiguous()` test: the bit survives every
    step and `data_ptr()` points at the bytes that are not conjugated.  (If torch ever changes this, the helper is merely cautious.)"""
    Z = _dense(torch.complex64)
    view, base = _layouts.build("conj", Z)
    old = view.detach().reshape(Z.shape)[:].to(device=CPU, dtype=torch.complex64).contiguous()
    assert old.is_conj() and old.data_ptr() == base.data_ptr() and not torch.equal(base, Z)
