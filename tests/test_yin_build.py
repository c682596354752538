"""Register budgets of k_yin, read from the code object inside libspecinv.so the way tests/test_build_resources.py reads them (no
GPU needed): every variant is within its launch bounds - 256 threads, one wave per SIMD, the 512-entry register file - and
spills nothing."""
import pytest

from test_build_resources import LIB, READELF, _kernel_table


@pytest.fixture(scope="module")
def kernels():
    import os
    from spectrogram_inversion_amd import build
    build.build_lib()
    assert os.path.exists(LIB) and os.path.exists(READELF), "libspecinv.so / llvm-readelf not available"
    return _kernel_table()


@pytest.mark.parametrize("r", (4, 8, 16, 32))
def test_no_variant_spills(kernels, r):
    hits = [k for k in kernels if f"5k_yinILi{r}EE" in k]
    assert len(hits) == 1, hits
    vgprs, spilled, agprs = kernels[hits[0]]
    print(f"k_yin<{r}>: {vgprs} registers ({agprs} accumulation), {spilled} spilled")
    assert spilled == 0 and vgprs <= 512
