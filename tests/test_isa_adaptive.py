"""Code-generation guards for the adaptive-supersampling kernels (CPU: reads the gfx950 code object of
librtx_hip.so through tests/isa_tools.py): rtx_adaptive_kernel<DEEP, HSTK> has its three instantiations,
uses no scratch, stays inside the shade kernel's occupancy tier (7 waves per SIMD: at most 72 VGPRs) and
resolves across lanes without LDS traffic of its own; rtx_classify_kernel exists, without scratch or LDS."""
import re

import pytest

import isa_tools

ADAPTIVE = r"_Z19rtx_adaptive_kernelILb([01])ELb([01])E"
SHADE = r"_Z16rtx_shade_kernelILb([01])ELb([01])E"
CLASSIFY = r"_Z19rtx_classify_kernel"
TIER_VGPRS = 72   # 512 / 7 waves, in allocation units of 8


@pytest.fixture(scope="module")
def kernels():
    lib = isa_tools.product_library()
    return {p: isa_tools.kernels(lib, p) for p in (ADAPTIVE, SHADE, CLASSIFY)}


def test_the_three_instantiations_and_the_classifier_exist(kernels):
    assert sorted(kernels[ADAPTIVE]) == [(0, 0), (1, 0), (1, 1)]
    assert kernels[CLASSIFY], "rtx_classify_kernel is missing"


def test_no_scratch_and_the_shade_kernels_tier(kernels):
    shade = kernels[SHADE]
    for key, (_, m) in kernels[ADAPTIVE].items():
        assert m["private_segment_fixed_size"] == 0, (key, m)
        assert m["vgpr_count"] <= TIER_VGPRS, (key, m)
        assert shade[key][1]["vgpr_count"] <= TIER_VGPRS   # (the tier is the shade kernel's)
        assert m["group_segment_fixed_size"] == shade[key][1]["group_segment_fixed_size"], (key, m)
    c = next(iter(kernels[CLASSIFY].values()))[1]
    assert c["private_segment_fixed_size"] == 0 and c["group_segment_fixed_size"] == 0, c


def test_the_resolve_is_cross_lane(kernels):
    """The six butterfly levels of three channels: DPP adds and the two permlane swaps, per variant."""
    for key, (body, _) in kernels[ADAPTIVE].items():
        assert len(re.findall(r"\bv_add_f32_dpp\b|\bv_add_f32\b.*\b(quad_perm|row_half_mirror|row_ror)", body)) >= 12, key
        assert body.count("v_permlane16_swap") >= 3 and body.count("v_permlane32_swap") >= 3, key
