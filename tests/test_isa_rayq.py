"""Code-generation guards for the ray-query kernels (CPU: reads the gfx950 code object in librtx_hip.so,
as tests/test_isa.py does for the render kernel): the six instantiations of rtx_query_kernel<ANY, DEEP,
HSTK> use no scratch, fetch node pairs and triangles through the scalar unit, and stay at 8 waves per
SIMD by their registers (profiles/rayq/resource_usage.txt: 25-33 VGPRs; the next occupancy step is
64)."""
import os
import re
import subprocess

import pytest

from test_isa import LLVM, _code_object

KERNEL = re.compile(r"^[0-9a-f]+ <(_Z16rtx_query_kernelILb([01])ELb([01])ELb([01])E\w+)>:", re.M)
VGPR_STEP = 64   # 512 / 64 = 8 waves per SIMD


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(f"{LLVM}/clang-offload-bundler"):
        pytest.skip("ROCm LLVM tools not present")
    from gp1_raytracer_2223_amd import build
    lib = os.path.join(os.path.dirname(build.__file__), "lib", "librtx_hip.so")
    if not os.path.exists(lib):
        build.build_hip()
    co = _code_object(tmp_path_factory.mktemp("isa_rayq"), lib)
    dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--mcpu=gfx950", str(co)], check=True, capture_output=True,
                         text=True).stdout
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(co)], check=True, capture_output=True,
                           text=True).stdout
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
        out[tuple(int(m.group(k)) for k in (2, 3, 4))] = (body, meta)
    return out


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
