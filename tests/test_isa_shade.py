"""Code-generation guards for the shaded-ray kernels (CPU: reads the gfx950 code object in librtx_hip.so,
as tests/test_isa_rayq.py does for the query kernels): the three instantiations of rtx_shade_kernel<DEEP,
HSTK> exist, use no scratch, stay inside the register bound tests/test_isa.py holds the generic render
kernel to (the body this kernel restates), and fetch node pairs and triangles through the scalar unit;
rtx_query_kernel keeps exactly its six instantiations (the shade kernel is a __global__ of its own, not a
mode of that template)."""
import re

import pytest

import isa_tools

KERNEL = r"_Z16rtx_shade_kernelILb([01])ELb([01])E\w+$"   # <DEEP, HSTK>
QUERY = r"_Z16rtx_query_kernelILb([01])ELb([01])ELb([01])E\w+$"
VGPR_BOUND = 80   # the generic render kernel's (tests/test_isa.py)


@pytest.fixture(scope="module")
def kernels():
    return isa_tools.kernels(isa_tools.product_library(), KERNEL)


def test_the_three_instantiations_exist(kernels):
    assert sorted(kernels) == [(0, 0), (1, 0), (1, 1)]


def test_no_scratch_and_the_generic_kernels_registers(kernels):
    for key, (_, meta) in kernels.items():
        assert meta.get("private_segment_fixed_size") == 0, (key, meta)
        assert meta.get("vgpr_count", 999) + meta.get("agpr_count", 0) <= VGPR_BOUND, (key, meta)


def test_uniform_records_are_scalar_loads(kernels):
    for key, (body, _) in kernels.items():
        assert body.count("s_load_dwordx16") >= 8, f"{key}: 64-byte BVH/triangle records are no longer scalar loads"


def test_the_query_kernel_keeps_its_six_instantiations():
    names = isa_tools.symbols(isa_tools.product_library(), QUERY)
    got = sorted(tuple(int(x) for x in re.match(QUERY, n).groups()) for n in names)
    assert got == [(0, 0, 0), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 1, 0), (1, 1, 1)]
