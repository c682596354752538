"""Views that hold the values of a dense tensor in the layouts callers really pass: strides (`torch.stft`'s output, a slice with a
step, stride 0), an offset from a 16-byte boundary, the lazy conjugate and negative bits.

Each builder takes the intended dense tensor `Z` (CPU or GPU) and returns `(view, base)`: `view` has `Z`'s values and shape,
`base` is the buffer it looks into (compare it against a clone taken before a call to show the call left it alone).  Each asserts
the property it claims, and that the view really holds `Z`.  `dense_twin(view, Z)` is the freshly made dense tensor of the same
values a layout test compares against.
"""
import torch


def strided(Z):
    """`torch.stft`'s layout: the last two dims transposed from a dense base ((B, L): the transpose of (L, B))."""
    base = Z.transpose(-1, -2).contiguous()
    view = base.transpose(-1, -2)
    assert not view.is_contiguous() and view.stride(-2) == 1
    return view, base


def offset(Z):
    """A contiguous view one element into a larger flat buffer: off the 16-byte boundary for every element narrower than 16
    bytes.  (A complex128 element is 16 bytes, and `view_as_complex` / `view(dtype)` refuse an odd offset in reals: no torch view
    puts one at 8 mod 16.  There the view is one element in, which is all a view can be.)"""
    base = torch.empty(Z.numel() + 5, dtype=Z.dtype, device=Z.device)
    base.copy_(torch.arange(base.numel(), device=Z.device))        # (what surrounds the view is not zeros)
    base[1:1 + Z.numel()] = Z.reshape(-1)
    view = base[1:1 + Z.numel()].view(Z.shape)
    assert view.is_contiguous() and view.storage_offset() == 1
    if Z.element_size() < 16:
        assert view.data_ptr() % 16 != 0
    return view, base


def step_batch(Z):
    """`big[::2]` over the batch."""
    base = torch.zeros((2 * Z.shape[0],) + tuple(Z.shape[1:]), dtype=Z.dtype, device=Z.device)
    base[1::2] = 7
    base[::2] = Z
    view = base[::2]
    assert view.stride(0) == 2 * Z[0].numel() and (Z.shape[0] == 1 or not view.is_contiguous())
    return view, base


def step_last(Z):
    """`big[..., ::2]` over the last dim."""
    base = torch.zeros(tuple(Z.shape[:-1]) + (2 * Z.shape[-1],), dtype=Z.dtype, device=Z.device)
    base[..., 1::2] = 7
    base[..., ::2] = Z
    view = base[..., ::2]
    assert view.stride(-1) == 2 and not view.is_contiguous()
    return view, base


def expanded(Z):
    """One item with stride 0 over the batch (the items of `Z` must be equal: `repeated(Z)` makes such a Z)."""
    base = Z[:1].clone()
    view = base.expand(Z.shape)
    assert view.stride(0) == 0
    return view, base


def conj(Z):
    """`S.conj()`: the conjugate bit on a contiguous tensor whose bytes are the conjugate of its values."""
    base = torch.conj_physical(Z).contiguous()
    view = base.conj()
    assert view.is_conj() and view.is_contiguous() and view.data_ptr() == base.data_ptr()
    return view, base


def conj_strided(Z):
    """`S.mH`: the conjugate bit and transposed strides at once."""
    base = torch.conj_physical(Z.transpose(-1, -2)).contiguous()
    view = base.mH
    assert view.is_conj() and not view.is_contiguous()
    return view, base


def neg(Z):
    """The negative bit: `.imag` of a lazily conjugated complex tensor."""
    base = torch.complex(torch.zeros_like(Z), -Z)
    view = base.conj().imag
    assert view.is_neg()
    return view, base


REAL = {"strided": strided, "offset": offset, "step_batch": step_batch, "step_last": step_last, "expanded": expanded, "neg": neg}
COMPLEX = {"strided": strided, "offset": offset, "step_batch": step_batch, "step_last": step_last, "expanded": expanded,
           "conj": conj, "conj_strided": conj_strided}


def builders(dtype):
    return COMPLEX if dtype.is_complex else REAL


def repeated(Z):
    """`Z` with every item of the batch equal to the first: what `expanded` can represent."""
    return Z[:1].expand(Z.shape).contiguous()


def build(name, Z):
    """`(view, base)` of builder `name`, checked: the view has `Z`'s shape, dtype, device and values."""
    if name == "expanded":
        assert torch.equal(repeated(Z), Z), "expanded needs equal items"
    if name in ("strided", "conj_strided"):
        assert Z.dim() >= 2
    view, base = builders(Z.dtype)[name](Z)
    assert view.shape == Z.shape and view.dtype == Z.dtype and view.device == Z.device
    assert torch.equal(view, Z)
    return view, base


def dense_twin(view, Z):
    twin = torch.empty(view.shape, dtype=view.dtype, device=view.device).copy_(view)
    assert twin.is_contiguous() and not twin.is_conj() and not twin.is_neg() and twin.data_ptr() % 16 == 0
    assert torch.equal(twin, Z)
    return twin
