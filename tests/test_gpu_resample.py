"""resample on the device against the definition in NumPy float64 (tests/_resample_oracle.py) on the input's own bits.

Cases meet every corner of k_resample: ratios that raise and lower the rate, 87 taps (7:1), an unbatched call, m * o beyond 2^31
(27781:22050 at L 100000), L = 1 and L = 5 (every tap window clipped on both sides), and output counts around TILE = 256, the
kernel's outputs per workgroup (kResampleTile).  At 2:3 an L_out is 0 or 2 modulo 3, so of 255, 256, 257 only 255 and 257 exist
there: they are taken at 2:3 together with 512 and 513 (two workgroups exactly, and one output more), and 255, 256, 257 at 3:2.
A workgroup stages its span of the row through 16 KiB of LDS when floor(255 o / n) + 2 J + 3 elements fit (J = ceil(W o / base)),
else it reads global memory: 176:23 is the last ratio that fits in float64 (2048 elements), 222:29 the first that does not,
475:31 fits float32 exactly (4096) and 31:2 does not; 20:1 takes the direct path in both dtypes.

Bounds, with K = 2 ceil(W o / base) + 1 taps and A = (base / o) max |x|:
  float64: max |y - y_ref| <= K 2^-45 A + 2^-52 max |y_ref|.  Each weight comes from a sine and a cosine whose arguments reach
    6 pi: an ulp of the argument is 3.5e-15 ~ 2^-48, taken per tap times 8 for the recurrence and the device's sincos.
  float32: that plus 2^-24 max |y_ref|, the single rounding.
"""
import numpy as np
import pytest
import torch

import spectrogram_inversion_amd as si
from _resample_oracle import gain, length_out, resample_ref, taps

pytestmark = pytest.mark.gpu

F16, F32, F64 = torch.float16, torch.float32, torch.float64
DEV = "cuda"
TILE = 256                  # kResampleTile: outputs per workgroup

# (orig, new, batch (None: unbatched), L)
SHAPES = [(3, 2, 3, 1000), (2, 3, 3, 1000), (7, 1, 2, 2000), (1, 5, 2, 300), (160, 147, None, 1500), (27781, 22050, 1, 100000),
          (48000, 44100, 2, 700),
          (3, 2, 1, 1), (3, 2, 1, 5), (2, 3, 1, 1), (2, 3, 1, 5),
          (2, 3, 2, 170), (2, 3, 2, 171), (2, 3, 2, 341), (2, 3, 2, 342),
          (3, 2, 2, 382), (3, 2, 2, 383), (3, 2, 2, 385),
          (176, 23, 2, 2000), (222, 29, 2, 2000), (475, 31, 2, 4000), (31, 2, 2, 4000), (20, 1, 2, 6000)]
CASES = [s + (d,) for s in SHAPES for d in (F32, F64)]


def _id(c):
    return f"{c[0]}:{c[1]}-B{c[2]}-L{c[3]}-{'f32' if c[4] == F32 else 'f64'}"


def _input(batch, length, dtype, seed):
    x = torch.randn(batch or 1, length, generator=torch.Generator().manual_seed(seed), dtype=F64).to(dtype)
    return x[0] if batch is None else x


def _bound(x, ref, orig, new, dtype):
    b = taps(orig, new) * 2.0 ** -45 * gain(orig, new) * float(x.abs().max()) + 2.0 ** -52 * float(np.abs(ref).max())
    return b + (2.0 ** -24 * float(np.abs(ref).max()) if dtype == F32 else 0.0)


def test_the_tile_lengths_are_what_the_docstring_says():
    assert [length_out(n, 2, 3) for n in (170, 171, 341, 342)] == [TILE - 1, TILE + 1, 2 * TILE, 2 * TILE + 1]
    assert [length_out(n, 3, 2) for n in (382, 383, 385)] == [TILE - 1, TILE, TILE + 1]
    assert length_out(100000, 27781, 22050) * 27781 > 2 ** 31


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_parity_with_the_definition(case):
    orig, new, batch, length, dtype = case
    x = _input(batch, length, dtype, seed=orig + new + length)
    ref = resample_ref(x.double().numpy(), orig, new)
    y = si.resample(x.to(DEV), orig, new)
    assert y.device.type == "cuda" and y.dtype == dtype and tuple(y.shape) == ref.shape
    assert y.shape[-1] == length_out(length, orig, new)
    err = float(np.abs(y.cpu().double().numpy() - ref).max())
    bound = _bound(x, ref, orig, new, dtype)
    print(f"{_id(case)}: L_out {y.shape[-1]} K {taps(orig, new)} error {err:.3e} bound {bound:.3e} ({err / bound:.3f})")
    assert err <= bound


@pytest.mark.parametrize("dtype", (F32, F64), ids=("f32", "f64"))
def test_other_filter_parameters(dtype):
    """rolloff 1 (13 taps when raising the rate) and a wider filter"""
    x = _input(2, 777, dtype, seed=5)
    for orig, new, width, rolloff in ((2, 3, 6, 1.0), (5, 4, 16, 0.9475), (4, 5, 1, 0.5)):
        ref = resample_ref(x.double().numpy(), orig, new, width, rolloff)
        y = si.resample(x.to(DEV), orig, new, lowpass_filter_width=width, rolloff=rolloff)
        err = float(np.abs(y.cpu().double().numpy() - ref).max())
        bound = (taps(orig, new, width, rolloff) * 2.0 ** -45 * gain(orig, new, rolloff) * float(x.abs().max())
                 + (2.0 ** -52 + (2.0 ** -24 if dtype == F32 else 0.0)) * float(np.abs(ref).max()))
        print(f"{orig}:{new} W {width} rolloff {rolloff} {dtype}: error {err:.3e} bound {bound:.3e}")
        assert tuple(y.shape) == ref.shape and err <= bound


@pytest.mark.parametrize("dtype", (F32, F64), ids=("f32", "f64"))
def test_only_the_reduced_ratio_matters(dtype):
    x = _input(2, 700, dtype, seed=1).to(DEV)
    assert torch.equal(si.resample(x, 48000, 44100), si.resample(x, 160, 147))


@pytest.mark.parametrize("dtype", (F32, F64), ids=("f32", "f64"))
def test_a_row_of_a_batch_is_the_unbatched_call(dtype):
    x = _input(3, 1000, dtype, seed=2).to(DEV)
    for orig, new in ((3, 2), (2, 3), (20, 1)):
        y = si.resample(x, orig, new)
        for b in range(3):
            assert torch.equal(y[b], si.resample(x[b], orig, new))


def test_equal_rates_copy():
    x = _input(2, 300, F32, seed=3).to(DEV)
    y = si.resample(x, 44100, 44100)
    assert y.data_ptr() != x.data_ptr() and torch.equal(y, x)


def test_the_entry_point_copies_at_equal_rates_too():
    import ctypes as C
    from spectrogram_inversion_amd import _lib
    lib = _lib.load()
    for dtype, code in ((F32, _lib.F32), (F64, _lib.F64)):
        x = _input(2, 300, dtype, seed=9).to(DEV)
        y = torch.zeros_like(x)
        stream = torch.cuda.current_stream()
        _lib.check(lib.specinv_resample(x.data_ptr(), y.data_ptr(), 2, 300, 300, 44100, 44100, 6, 0.99, code, stream.device.index,
                                        C.c_void_p(stream.cuda_stream)))
        torch.cuda.synchronize()
        assert torch.equal(y, x)


def test_a_transposed_view_gives_the_contiguous_inputs_bits():
    xt = _input(500, 3, F32, seed=4).to(DEV)            # (500, 3): its transpose is (3, 500) with strides (1, 3)
    assert not xt.t().is_contiguous()
    assert torch.equal(si.resample(xt.t(), 3, 2), si.resample(xt.t().contiguous(), 3, 2))


def test_a_cpu_tensor_comes_back_to_the_cpu():
    x = _input(2, 400, F64, seed=6)
    y = si.resample(x, 2, 3)
    assert y.device.type == "cpu" and y.dtype == F64
    assert torch.equal(y, si.resample(x.to(DEV), 2, 3).cpu())


def test_float16_is_float32_rounded_back():
    x = _input(2, 400, F16, seed=7).to(DEV)
    y = si.resample(x, 3, 2)
    assert y.dtype == F16 and torch.equal(y, si.resample(x.float(), 3, 2).half())


def test_an_empty_batch():
    y = si.resample(torch.zeros(0, 100, device=DEV), 3, 2)
    assert tuple(y.shape) == (0, length_out(100, 3, 2)) and y.device.type == "cuda"


def test_no_item_bound_is_hidden():
    x = torch.randn(70000, 8, generator=torch.Generator().manual_seed(8), dtype=F32)
    y = si.resample(x.to(DEV), 2, 3)
    assert tuple(y.shape) == (70000, 12)
    rows = [0, 65535, 69999]
    ref = resample_ref(x[rows].double().numpy(), 2, 3)
    err = float(np.abs(y[rows].cpu().double().numpy() - ref).max())
    bound = _bound(x[rows], ref, 2, 3, F32)
    print(f"70000 items: rows {rows} error {err:.3e} bound {bound:.3e}")
    assert err <= bound
