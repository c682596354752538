"""Register budgets of k_wpe, read from the code object inside libspecinv.so the way tests/test_build_resources.py reads them (no
GPU needed): all four instantiations - scalar type x one or two register blocks a thread - are there, spill nothing and stay
within their launch bounds.  k_wpe runs four waves a workgroup (__launch_bounds__(256)), one per SIMD: 512 registers a lane."""
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


@pytest.mark.parametrize("scalar,blocks", list(itertools.product("fd", (1, 2))))
def test_no_wpe_variant_spills(kernels, scalar, blocks):
    hits = [k for k in kernels if f"5k_wpeI{scalar}Li{blocks}EE" in k]
    assert len(hits) == 1, hits
    vgprs, spilled, agprs = kernels[hits[0]]
    print(f"k_wpe<{scalar}, {blocks}>: {vgprs} registers ({agprs} accumulation), {spilled} spilled")
    assert spilled == 0 and vgprs + agprs <= 512
