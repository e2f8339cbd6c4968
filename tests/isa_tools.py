"""The gfx950 code objects of librtx_hip.so, read once — TEST INFRASTRUCTURE of the tests/test_isa*.py
guards and of the *_cpu.py tests that look at a kernel's metadata.  tools/codeobj_diff.py finds the code
objects (the library holds one offload bundle per device link); the listing here is LLVM's own text."""
import functools
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "tools"))
import codeobj_diff  # noqa: E402

LLVM = "/opt/rocm/lib/llvm/bin"   # fixed: the guards skip only where ROCm's own LLVM tools are absent
META_KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def product_library() -> str:
    """librtx_hip.so, built if missing."""
    from gp1_raytracer_2223_amd import build
    lib = os.path.join(os.path.dirname(build.__file__), "lib", "librtx_hip.so")
    if not os.path.exists(lib):
        build.build_hip()
    return lib


@functools.lru_cache(maxsize=None)
def listing(lib):
    """(disassembly, notes) of `lib`'s gfx950 code objects, as llvm-objdump and llvm-readelf print them;
    skips the calling test where the ROCm LLVM tools are absent."""
    if not os.path.exists(f"{LLVM}/clang-offload-bundler"):
        pytest.skip("ROCm LLVM tools not present")
    dis, notes = [], []
    with tempfile.TemporaryDirectory(prefix="rtx_isa_") as td:
        for co in codeobj_diff.code_objects(Path(lib), Path(td)):
            dis.append(subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--mcpu=gfx950", str(co)], check=True,
                                      capture_output=True, text=True).stdout)
            notes.append(subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(co)], check=True, capture_output=True,
                                        text=True).stdout)
    return "\n".join(dis), "\n".join(notes)


def kernels(lib, pattern):
    """{key: (body, meta)} of the kernels whose symbol matches `pattern` from its start: the key is the
    pattern's groups as ints, or the symbol where it has none; the body runs to the next symbol (a kernel may
    have several s_endpgm); meta holds the META_KEYS its notes state."""
    dis, notes = listing(lib)
    blocks = notes.split("  - .")[1:]
    header = re.compile(r"^[0-9a-f]+ <([^>]+)>:", re.M)
    heads = list(header.finditer(dis))
    out = {}
    for m, nxt in zip(heads, heads[1:] + [None]):
        k = re.match(pattern, m.group(1))
        if not k:
            continue
        body = dis[m.end():nxt.start() if nxt else len(dis)]
        meta = {}
        for block in blocks:
            if re.search(rf"\.name:\s+{re.escape(m.group(1))}\b", block):
                for key in META_KEYS:
                    mm = re.search(rf"\.{key}:\s+(\d+)", block)
                    if mm:
                        meta[key] = int(mm.group(1))
        key = tuple(int(g) for g in k.groups()) if k.groups() else m.group(1)
        assert key not in out, f"two symbols match {pattern} with {key}"
        out[key] = (body, meta)
    return out


def symbols(lib, pattern):
    """Every kernel symbol of the listing that matches `pattern` from its start, duplicates kept."""
    return [s for s in re.findall(r"^[0-9a-f]+ <([^>]+)>:", listing(lib)[0], re.M) if re.match(pattern, s)]
