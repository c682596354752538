"""The one place a caller's tensor becomes something whose `data_ptr()` a kernel may read.

The kernels take a dense buffer: element i of the flattened tensor at byte i * itemsize of a 16-byte aligned pointer.  A torch
tensor promises less - strides (a transpose, a slice with a step, stride 0 from `expand` or from `sum().backward()`), a storage
offset (`batch[1:]`), and two lazy bits: `S.conj()` / `S.mH` / a gradient that flowed back through a `.conj()` carry the
conjugate bit, `.imag` of such a tensor the negative bit; `is_contiguous()` is True for them and the bytes at `data_ptr()` are
the ones that are *not* conjugated / negated.  `detach`, `reshape`, a same-dtype `.to` and `.contiguous()` all keep the bits.
Needs torch only, not the native library.
"""
from __future__ import annotations

import numbers

import torch

ALIGN = 16          # bytes: the vector kernels load 16 bytes per lane, the wave kernels pair elements by index parity


# The predicates the wrappers' argument checks share (each wrapper words its own error).
def is_int(v) -> bool:
    """an int that is no bool"""
    return isinstance(v, int) and not isinstance(v, bool)


def is_real(v) -> bool:
    """a real number that is no bool (NaN and the infinities included)"""
    return isinstance(v, numbers.Real) and not isinstance(v, bool)


def broadcasts_to(shape, want) -> bool:
    want = tuple(want)
    try:
        return torch.broadcast_shapes(tuple(shape), want) == want
    except RuntimeError:
        return False


def ingest(t: torch.Tensor, device, dtype) -> torch.Tensor:
    """`t` as the kernels read it: detached, on `device`, in `dtype`, contiguous, with neither the conjugate nor the negative bit,
    at a 16-byte aligned address.  `t` itself, with no copy, when all of that already holds (attribute tests only: the optimiser
    loops come through here a few hundred thousand times)."""
    if (t.dtype != dtype or t.device != device or t.requires_grad or not t.is_contiguous() or t.is_conj() or t.is_neg()
            or t.data_ptr() % ALIGN):
        t = t.detach().to(device=device, dtype=dtype).resolve_conj().resolve_neg().contiguous()
        if t.data_ptr() % ALIGN:
            t = t.clone()
    return t
