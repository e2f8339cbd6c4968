"""Code-generation guards for the shaded-ray kernels (CPU: reads the gfx950 code object in librtx_hip.so,
as tests/test_isa_rayq.py does for the query kernels): the three instantiations of rtx_shade_kernel<DEEP,
HSTK> exist, use no scratch, stay inside the register bound tests/test_isa.py holds the generic render
kernel to (the body this kernel restates), and fetch node pairs and triangles through the scalar unit;
rtx_query_kernel keeps exactly its six instantiations (the shade kernel is a __global__ of its own, not a
mode of that template)."""
import os
import re
import subprocess

import pytest

from test_isa import LLVM, _code_object

KERNEL = re.compile(r"^[0-9a-f]+ <(_Z16rtx_shade_kernelILb([01])ELb([01])E\w+)>:", re.M)
QUERY = re.compile(r"^[0-9a-f]+ <_Z16rtx_query_kernelILb([01])ELb([01])ELb([01])E\w+>:", re.M)
VGPR_BOUND = 80   # the generic render kernel's (tests/test_isa.py)


@pytest.fixture(scope="module")
def code(tmp_path_factory):
    if not os.path.exists(f"{LLVM}/clang-offload-bundler"):
        pytest.skip("ROCm LLVM tools not present")
    from gp1_raytracer_2223_amd import build
    lib = os.path.join(os.path.dirname(build.__file__), "lib", "librtx_hip.so")
    if not os.path.exists(lib):
        build.build_hip()
    co = _code_object(tmp_path_factory.mktemp("isa_shade"), lib)
    dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--mcpu=gfx950", str(co)], check=True, capture_output=True,
                         text=True).stdout
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(co)], check=True, capture_output=True,
                           text=True).stdout
    return dis, notes


@pytest.fixture(scope="module")
def kernels(code):
    dis, notes = code
    header = re.compile(r"^[0-9a-f]+ <", re.M)
    out = {}
    for m in KERNEL.finditer(dis):
        nxt = header.search(dis, m.end())   # (the kernel has several s_endpgm: its body runs to the next symbol)
        body = dis[m.end():nxt.start() if nxt else len(dis)]
        meta = {}
        for block in notes.split("  - .")[1:]:
            if re.search(rf"\.name:\s+{m.group(1)}\b", block):
                for key in ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size"):
                    mm = re.search(rf"\.{key}:\s+(\d+)", block)
                    if mm:
                        meta[key] = int(mm.group(1))
        out[tuple(int(m.group(k)) for k in (2, 3))] = (body, meta)
    return out


def test_the_three_instantiations_exist(kernels):
    assert sorted(kernels) == [(0, 0), (1, 0), (1, 1)]


def test_no_scratch_and_the_generic_kernels_registers(kernels):
    for key, (_, meta) in kernels.items():
        assert meta.get("private_segment_fixed_size") == 0, (key, meta)
        assert meta.get("vgpr_count", 999) + meta.get("agpr_count", 0) <= VGPR_BOUND, (key, meta)


def test_uniform_records_are_scalar_loads(kernels):
    for key, (body, _) in kernels.items():
        assert body.count("s_load_dwordx16") >= 8, f"{key}: 64-byte BVH/triangle records are no longer scalar loads"


def test_the_query_kernel_keeps_its_six_instantiations(code):
    got = sorted(tuple(int(x) for x in m.groups()) for m in QUERY.finditer(code[0]))
    assert got == [(0, 0, 0), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 1, 0), (1, 1, 1)]
