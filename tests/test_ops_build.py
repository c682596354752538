"""Register budgets of the plan-free ops' kernels - k_enhance, k_wpe, k_beamform, k_yin, k_pyin_obs, k_pyin_viterbi - read from the
code object inside libspecinv.so the way tests/test_build_resources.py reads them (no GPU needed): every instantiation is there,
spills nothing and stays within its launch bounds."""
import itertools
import os

import pytest

from test_build_resources import LIB, READELF, _kernel_table


@pytest.fixture(scope="module")
def kernels():
    from spectrogram_inversion_amd import build
    build.build_lib()
    assert os.path.exists(LIB) and os.path.exists(READELF), "libspecinv.so / llvm-readelf not available"
    return _kernel_table()


def _budget(kernels, mangled, shown):
    """(registers, accumulation registers) of the one kernel whose mangled name holds `mangled`, which spills nothing"""
    hits = [k for k in kernels if mangled in k]
    assert len(hits) == 1, hits
    vgprs, spilled, agprs = kernels[hits[0]]
    print(f"{shown}: {vgprs} registers ({agprs} accumulation), {spilled} spilled")
    assert spilled == 0
    return vgprs, agprs


# k_enhance, all sixteen instantiations - scalar type x real / complex x layout x rule: at most four waves a workgroup
# (__launch_bounds__(256)), one per SIMD: 512 registers a lane
@pytest.mark.parametrize("scalar,cplx,frame_major,rule", list(itertools.product("fd", (0, 1), (0, 1), (0, 1))))
def test_no_enhance_variant_spills(kernels, scalar, cplx, frame_major, rule):
    vgprs, agprs = _budget(kernels, f"9k_enhanceI{scalar}Lb{cplx}ELb{frame_major}ELi{rule}EE",
                           f"k_enhance<{scalar}, {cplx}, {frame_major}, {rule}>")
    assert vgprs + agprs <= 512


# k_wpe, all four instantiations - scalar type x one or two register blocks a thread: four waves a workgroup
# (__launch_bounds__(256)), one per SIMD: 512 registers a lane
@pytest.mark.parametrize("scalar,blocks", list(itertools.product("fd", (1, 2))))
def test_no_wpe_variant_spills(kernels, scalar, blocks):
    vgprs, agprs = _budget(kernels, f"5k_wpeI{scalar}Li{blocks}EE", f"k_wpe<{scalar}, {blocks}>")
    assert vgprs + agprs <= 512


# k_beamform, all four instantiations - scalar type x one or four covariance entries a lane: a workgroup is one wave
# (__launch_bounds__(64)): up to 512 registers a lane
@pytest.mark.parametrize("scalar,entries", list(itertools.product("fd", (1, 4))))
def test_no_beamform_variant_spills(kernels, scalar, entries):
    vgprs, agprs = _budget(kernels, f"10k_beamformI{scalar}Li{entries}EE", f"k_beamform<{scalar}, {entries}>")
    assert vgprs + agprs <= 512


# k_yin: 256 threads, one wave per SIMD, the 512-entry register file
@pytest.mark.parametrize("r", (4, 8, 16, 32))
def test_no_yin_variant_spills(kernels, r):
    vgprs, _ = _budget(kernels, f"5k_yinILi{r}EE", f"k_yin<{r}>")
    assert vgprs <= 512


# k_pyin_obs<C>: 256 threads a workgroup (512 registers a lane at one wave per SIMD)
@pytest.mark.parametrize("c", (2, 4, 8, 16))
def test_no_obs_variant_spills(kernels, c):
    vgprs, _ = _budget(kernels, f"10k_pyin_obsILi{c}EE", f"k_pyin_obs<{c}>")
    assert vgprs <= 512


# k_pyin_viterbi: up to 1024 threads, sixteen waves or four per SIMD, which leaves a lane 128
@pytest.mark.parametrize("ticks", (0, 1))
def test_no_viterbi_variant_spills(kernels, ticks):
    vgprs, agprs = _budget(kernels, f"14k_pyin_viterbiILb{ticks}EE", f"k_pyin_viterbi<{bool(ticks)}>")
    assert vgprs + agprs <= 128
