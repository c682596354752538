"""Register budgets of k_beamform, read from the code object inside libspecinv.so the way tests/test_build_resources.py reads them
(no GPU needed): all four instantiations - scalar type x one or four covariance entries a lane - are there, spill nothing and stay
within their launch bounds.  A workgroup of k_beamform is one wave (__launch_bounds__(64)): up to 512 registers a lane."""
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


@pytest.mark.parametrize("scalar,entries", list(itertools.product("fd", (1, 4))))
def test_no_beamform_variant_spills(kernels, scalar, entries):
    hits = [k for k in kernels if f"10k_beamformI{scalar}Li{entries}EE" in k]
    assert len(hits) == 1, hits
    vgprs, spilled, agprs = kernels[hits[0]]
    print(f"k_beamform<{scalar}, {entries}>: {vgprs} registers ({agprs} accumulation), {spilled} spilled")
    assert spilled == 0 and vgprs + agprs <= 512
