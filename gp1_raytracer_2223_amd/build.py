"""In-tree native build (no cmake/ninja, no JIT cache): explicit g++/gcc/hipcc lines.

Outputs (git-ignored, travel to the GPU box with the gpurun snapshot):
  gp1_raytracer_2223_amd/lib/librtx_host.so   C++ host scene layer (g++)
  gp1_raytracer_2223_amd/lib/librtx_hip.so    HIP render path for gfx950 (hipcc), linked from one
                                              object per unit under lib/obj/ (only stale units recompile)
  oracle/_build/librtx_oracle.so              C restatement (test infrastructure)
  oracle/_ref/ref_harness                     the reference's own sources (test infra,
                                              only when /root/reference exists)

Every float-producing compile uses -ffp-contract=off and no fast-math: the reference is
MSVC /fp:precise x64 (no FMA contraction) and parity is bit-level.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

PKG = Path(__file__).resolve().parent
REPO = PKG.parent
LIB = PKG / "lib"
CSRC = PKG / "csrc"
INC = REPO / "include"
ORACLE = REPO / "oracle"
REFERENCE = Path("/root/reference")

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = os.environ.get("RTX_OFFLOAD_ARCH", "gfx950")


def _run(cmd: list[str], cwd: Path | None = None) -> None:
    print("+", " ".join(str(c) for c in cmd), flush=True)
    subprocess.run([str(c) for c in cmd], check=True, cwd=cwd)


def _stale(out: Path, deps: list[Path]) -> bool:
    if not out.exists():
        return True
    t = out.stat().st_mtime
    return any(d.stat().st_mtime > t for d in deps if d.exists())


def build_host(force: bool = False) -> Path:
    LIB.mkdir(exist_ok=True)
    out = LIB / "librtx_host.so"
    srcs = [CSRC / "host" / "scene.cpp", CSRC / "host" / "host_api.cpp", CSRC / "host" / "view.cpp"]
    deps = srcs + list((CSRC / "host").glob("*.h")) + [INC / "rtx.h", INC / "rtx_host.h", INC / "rtx_view.h",
                                                         Path(__file__)]
    if force or _stale(out, deps):
        _run(["g++", "-std=c++17", "-O3", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-pthread",
              "-Wall", "-Wextra", f"-I{INC}", *srcs, "-o", out, "-ldl"])
    return out


# The units of librtx_hip.so.  The kernel unit comes first: its object leads the link line, so its
# code object is the first of the library's fat binary (tests/test_isa.py reads that one).
HIP_KERNEL_UNIT = CSRC / "rtx_hip.hip"
HIP_SOURCES = [HIP_KERNEL_UNIT, CSRC / "rtx_cull_records.hip", CSRC / "rtx_sched.hip", CSRC / "rtx_context.hip",
               CSRC / "rtx_pack.cpp", CSRC / "rtx_upload.hip", CSRC / "rtx_frame.hip", CSRC / "rtx_pass.hip", CSRC / "rtx_aov.hip", CSRC / "rtx_deferred.hip", CSRC / "rtx_relight.hip", CSRC / "rtx_edit.hip", CSRC / "rtx_query.hip",
               CSRC / "rtx_adaptive.hip", CSRC / "rtx_diag.hip",
               CSRC / "rtx_policy.hip", CSRC / "rtx_anim.hip", CSRC / "rtx_anim_host.hip", CSRC / "rtx_group.cpp"]
# Every unit gets every flag (the host units compute floats that reach the pixels too).
# -fno-slp-vectorize: the SLP packer turns independent f32 ops into v_pk_* plus
# v_mov shuffles; measured 8 % slower on the render kernel (profiles/r01/ablate_*.txt).
# -structurizecfg-skip-uniform-regions: wave-uniform loops and branches (every loop of
# the BVH walk) stay plain s_cbranch_scc instead of being structurized into SGPR
# lane-mask phis (s_cselect -1/0 + s_and vcc, exec per exit): -6 % SALU per wave.
HIP_FLAGS = [f"--offload-arch={ARCH}", "-std=c++17", "-O3", "-ffp-contract=off",
             "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-slp-vectorize",
             "-mllvm", "-structurizecfg-skip-uniform-regions=true",
             "-DRTX_MIN_WAVES_PER_EU=6", "-fPIC", "-pthread",
             "-Wall", f"-I{INC}", f"-I{CSRC}"]
HIP_JOBS = 8   # units compiled at once (fixed: a shared machine's CPU count says nothing)


def hip_deps() -> list[Path]:
    """What every unit's object depends on besides its own source (the flags live in this file)."""
    return list(CSRC.glob("*.h")) + [INC / "rtx.h", INC / "rtx_diag.h", Path(__file__)]


def build_hip_lib(out: Path, objdir: Path, srcs: list[Path], flags: list[str], force: bool = False) -> Path:
    """Compile the stale units of `srcs` to objects under `objdir`, HIP_JOBS at a time, and link them in
    the order given into `out`."""
    objdir.mkdir(parents=True, exist_ok=True)
    objs = [objdir / (s.stem + ".o") for s in srcs]
    todo = [(s, o) for s, o in zip(srcs, objs) if force or _stale(o, [s] + hip_deps())]
    with ThreadPoolExecutor(max_workers=HIP_JOBS) as pool:
        for f in [pool.submit(_run, [HIPCC, *flags, "-c", s, "-o", o]) for s, o in todo]:
            f.result()
    _run([HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-pthread", *objs, "-o", out])
    return out


def build_hip(force: bool = False) -> Path:
    LIB.mkdir(exist_ok=True)
    out = LIB / "librtx_hip.so"
    if force or _stale(out, HIP_SOURCES + hip_deps()):
        build_hip_lib(out, LIB / "obj", HIP_SOURCES, HIP_FLAGS, force)
    return out


def build_cli(force: bool = False) -> Path:
    """Headless C++ host program over both libraries (lib/rtx_render)."""
    out = LIB / "rtx_render"
    src = CSRC / "cli" / "rtx_render.cpp"
    deps = [src, CSRC / "cli" / "benchmark.h", INC / "rtx_renderer.hpp", INC / "rtx.h", INC / "rtx_host.h", LIB / "librtx_hip.so",
            LIB / "librtx_host.so"]
    if force or _stale(out, deps):
        _run(["g++", "-std=c++17", "-O2", "-Wall", f"-I{INC}", src, "-o", out, f"-L{LIB}", "-lrtx_hip", "-lrtx_host",
              "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,/opt/rocm/lib"])
    return out


def build_view(force: bool = False) -> Path:
    """The SDL viewer (lib/rtx_view): SDL2 is dlopen'ed at run time, nothing links against it."""
    out = LIB / "rtx_view"
    src = CSRC / "cli" / "rtx_view.cpp"
    deps = [src, CSRC / "cli" / "benchmark.h", INC / "rtx.h", INC / "rtx_host.h", INC / "rtx_view.h",
            LIB / "librtx_hip.so", LIB / "librtx_host.so"]
    if force or _stale(out, deps):
        _run(["g++", "-std=c++17", "-O2", "-Wall", f"-I{INC}", src, "-o", out, f"-L{LIB}", "-lrtx_hip", "-lrtx_host",
              "-ldl", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,/opt/rocm/lib"])
    return out


def build_oracle(force: bool = False) -> Path:
    """Test infrastructure: the C restatement used only by tests/, smoke() and bench's
    cpu_baseline leg."""
    bdir = ORACLE / "_build"
    bdir.mkdir(exist_ok=True)
    out = bdir / "librtx_oracle.so"
    src = ORACLE / "rtx_oracle.c"
    if force or _stale(out, [src, INC / "rtx.h"]):
        _run(["gcc", "-std=c11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared",
              "-Wall", "-Wextra", f"-I{INC}", src, "-o", out, "-lm", "-lpthread"])
    return out


def build_checkers(force: bool = False) -> Path:
    """Test infrastructure: the brute-force CPU restatement of the cull records
    (tools/cull_records_ref.c), the checker of tests/test_gpu_cull.py."""
    bdir = REPO / "tools" / "bin"
    bdir.mkdir(exist_ok=True)
    out = bdir / "libcull_records_ref.so"
    src = REPO / "tools" / "cull_records_ref.c"
    if force or _stale(out, [src, CSRC / "rtx_cull.h"]):
        _run(["gcc", "-std=c11", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-Wall", "-Wextra",
              src, "-o", out, "-lm"])
    return out


def have_reference() -> bool:
    """The reference's sources are there and this user may read them."""
    try:
        return (REFERENCE / "source" / "Scene.cpp").exists()
    except OSError:   # a directory on the way is closed to this user: as good as absent
        return False


def build_reference(force: bool = False) -> Path | None:
    """Test infrastructure: the reference's own sources compiled in place (oracle/ref)."""
    out = ORACLE / "_ref" / "ref_harness"
    if not have_reference():
        return out if out.exists() else None
    if force and (ORACLE / "_ref").exists():
        shutil.rmtree(ORACLE / "_ref")
    _run(["make", "-s", "-C", ORACLE / "ref", "-j8"])
    return out


def build_all(force: bool = False) -> None:
    build_host(force)
    build_oracle(force)
    build_checkers(force)
    build_hip(force)
    build_reference(force)   # after librtx_hip.so: oracle/_ref/ref_binding links it
    build_cli(force)
    build_view(force)


if __name__ == "__main__":
    build_all(force="--force" in sys.argv)
