"""Register budgets of k_pyin_obs and k_pyin_viterbi, read from the code object inside libspecinv.so the way
tests/test_build_resources.py reads them (no GPU needed): every variant is within its launch bounds and spills nothing.
k_pyin_obs<C> runs 256 threads a workgroup (512 registers a lane at one wave per SIMD); k_pyin_viterbi runs up to 1024, sixteen
waves or four per SIMD, which leaves a lane 128."""
import pytest

from test_build_resources import LIB, READELF, _kernel_table


@pytest.fixture(scope="module")
def kernels():
    import os
    from spectrogram_inversion_amd import build
    build.build_lib()
    assert os.path.exists(LIB) and os.path.exists(READELF), "libspecinv.so / llvm-readelf not available"
    return _kernel_table()


@pytest.mark.parametrize("c", (2, 4, 8, 16))
def test_no_obs_variant_spills(kernels, c):
    hits = [k for k in kernels if f"10k_pyin_obsILi{c}EE" in k]
    assert len(hits) == 1, hits
    vgprs, spilled, agprs = kernels[hits[0]]
    print(f"k_pyin_obs<{c}>: {vgprs} registers ({agprs} accumulation), {spilled} spilled")
    assert spilled == 0 and vgprs <= 512


@pytest.mark.parametrize("ticks", (0, 1))
def test_no_viterbi_variant_spills(kernels, ticks):
    hits = [k for k in kernels if f"14k_pyin_viterbiILb{ticks}EE" in k]
    assert len(hits) == 1, hits
    vgprs, spilled, agprs = kernels[hits[0]]
    print(f"k_pyin_viterbi<{bool(ticks)}>: {vgprs} registers ({agprs} accumulation), {spilled} spilled")
    assert spilled == 0 and vgprs + agprs <= 128
