"""Register budgets of k_enhance, read from the code object inside libspecinv.so the way tests/test_build_resources.py reads them
(no GPU needed): all sixteen instantiations - scalar type x real / complex x layout x rule - are there, spill nothing and stay
within their launch bounds.  k_enhance runs at most four waves a workgroup (__launch_bounds__(256)), one per SIMD: 512 registers a lane."""
import itertools

import pytest

from test_build_resources import LIB, READELF, _kernel_table


@pytest.fixture(scope="module")
def kernels():
    import os
    from spectrogram_inversion_amd import build
    build.build_lib()
    assert os.path.exists(LIB) and os.path.exists(READELF), "libspecinv.so / llvm-readelf not available"
    return _kernel_table()


@pytest.mark.parametrize("scalar,cplx,frame_major,rule", list(itertools.product("fd", (0, 1), (0, 1), (0, 1))))
def test_no_enhance_variant_spills(kernels, scalar, cplx, frame_major, rule):
    hits = [k for k in kernels if f"9k_enhanceI{scalar}Lb{cplx}ELb{frame_major}ELi{rule}EE" in k]
    assert len(hits) == 1, hits
    vgprs, spilled, agprs = kernels[hits[0]]
    print(f"k_enhance<{scalar}, {cplx}, {frame_major}, {rule}>: {vgprs} registers ({agprs} accumulation), {spilled} spilled")
    assert spilled == 0 and vgprs + agprs <= 512
