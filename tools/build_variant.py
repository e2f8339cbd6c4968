"""Build an experiment variant of the render library into lib/exp/librtx_hip_<name>.so
(build.py's units and flags, plus extra -D / compiler flags for every unit), optionally with
another source file in place of the kernel unit (rtx_hip.hip).
Usage: python tools/build_variant.py <name> [--src file.hip] [flags...]
Select it at run time with RTX_HIP_LIB (kernel experiments only; tools/ab.sh)."""
import importlib.util
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "gp1_raytracer_2223_amd"


def main() -> int:
    spec = importlib.util.spec_from_file_location("rtx_build", PKG / "build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    name, args = sys.argv[1], sys.argv[2:]
    srcs = list(b.HIP_SOURCES)
    if args[:1] == ["--src"]:
        srcs[srcs.index(b.HIP_KERNEL_UNIT)], args = Path(args[1]).resolve(), args[2:]
    out = PKG / "lib" / "exp" / f"librtx_hip_{name}.so"
    # an extra -DNAME=... replaces the product's -DNAME=...
    flags = [f for f in b.HIP_FLAGS if not (f.startswith("-D") and any(a.startswith(f.split("=")[0]) for a in args))]
    try:   # (every unit again: the extra flags are not part of the objects' staleness check)
        b.build_hip_lib(out, out.parent / f"obj_{name}", srcs, flags + args, force=True)
    except subprocess.CalledProcessError as e:
        return e.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
