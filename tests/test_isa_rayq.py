"""Code-generation guards for the ray-query kernels (CPU: reads the gfx950 code object in librtx_hip.so,
as tests/test_isa.py does for the render kernel): the six instantiations of rtx_query_kernel<ANY, DEEP,
HSTK> use no scratch, fetch node pairs and triangles through the scalar unit, and stay at 8 waves per
SIMD by their registers (profiles/rayq/resource_usage.txt: 25-33 VGPRs; the next occupancy step is
64)."""
import re

import pytest

import isa_tools

KERNEL = r"_Z16rtx_query_kernelILb([01])ELb([01])ELb([01])E\w+$"   # <ANY, DEEP, HSTK>
VGPR_STEP = 64   # 512 / 64 = 8 waves per SIMD


@pytest.fixture(scope="module")
def kernels():
    return isa_tools.kernels(isa_tools.product_library(), KERNEL)


def test_the_six_instantiations_exist(kernels):
    assert sorted(kernels) == [(0, 0, 0), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 1, 0), (1, 1, 1)]


def test_no_scratch_and_eight_waves_of_registers(kernels):
    for key, (_, meta) in kernels.items():
        assert meta.get("private_segment_fixed_size") == 0, (key, meta)
        assert meta.get("vgpr_count", 999) + meta.get("agpr_count", 0) <= VGPR_STEP, (key, meta)


def test_uniform_records_are_scalar_loads(kernels):
    """Four walks per kernel (octant, fast, fast slab with the exact triangle test, exact), each with one
    64-byte load for a node pair and one for a triangle; the ray itself is the only per-lane read of the
    occlusion kernel besides the HBM stack."""
    for key, (body, _) in kernels.items():
        assert body.count("s_load_dwordx16") >= 8, f"{key}: 64-byte BVH/triangle records are no longer scalar loads"
        n = len(re.findall(r"\bglobal_load_", body))
        assert n <= (14 if key[0] == 0 else 7), f"{key}: {n} vector loads: scene reads fell back to per-lane loads"
