"""Resource usage of every rtx_render_kernel instantiation in two builds of librtx_hip.so, read from
the gfx950 code object's notes (no GPU needed):

    python tools/aov_resource_table.py parent/librtx_hip.so this/librtx_hip.so

VGPR, SGPR, scratch (private segment, bytes per lane) and LDS (group segment, bytes per workgroup) are
the notes' own figures.  Occupancy (waves per SIMD) follows from them for the one-wave workgroups the
library launches: min(8, 512 / VGPRs rounded up to the allocation granule of 8, LDS-bound workgroups
per CU / 4 SIMDs with 160 KiB of LDS per CU).  Instantiations are matched by mangled name; those only
the second build has (the hit pass, PHASE 7) are listed after the comparison."""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = "/opt/rocm/lib/llvm/bin"
KEYS = [("vgpr_count", "VGPR"), ("sgpr_count", "SGPR"), ("private_segment_fixed_size", "scratch"),
        ("group_segment_fixed_size", "LDS")]


def notes(lib: str) -> dict:
    with tempfile.TemporaryDirectory() as td:
        fb, co = Path(td) / "fatbin.bin", Path(td) / "gfx950.co"
        subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, str(fb)], check=True)
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fb}", f"--output={co}"], check=True)
        txt = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(co)], check=True, capture_output=True,
                             text=True).stdout
    out = {}
    for block in txt.split("  - .")[1:]:
        m = re.search(r"\.name:\s+(_Z17rtx_render_kernel\w+)", block)
        if not m:
            continue
        rec = {}
        for key, short in KEYS + [("agpr_count", "AGPR")]:
            mm = re.search(rf"\.{key}:\s+(\d+)", block)
            rec[short] = int(mm.group(1)) if mm else 0
        regs = -(-(rec["VGPR"] + rec["AGPR"]) // 8) * 8
        occ = min(8, 512 // max(regs, 8))
        if rec["LDS"]:
            occ = min(occ, -(-(160 * 1024 // rec["LDS"]) // 4))
        rec["occ"] = occ
        out[m.group(1)] = rec
    return out


def label(name: str) -> str:
    m = re.search(r"rtx_render_kernelILb(\d)ELi(\d)ELb(\d)ELi(\d+)ELb(\d)ELb(\d)E(?:Lb(\d)E)?", name)
    if not m:
        return name
    g = m.groups()
    return "COUNT=%s PHASE=%s DEEP=%s SPEC=%s HSTK=%s CULLK=%s SS=%s" % (g[:6] + (g[6] or "0",))


def main() -> int:
    a, b = notes(sys.argv[1]), notes(sys.argv[2])
    cols = [s for _, s in KEYS] + ["occ"]
    print("%-66s %s   (first build -> second; '=' unchanged)" % ("rtx_render_kernel<...>", " ".join("%-11s" % c for c in cols)))
    differ = 0
    for n in a:
        cells = []
        for c in cols:
            x, y = a[n][c], b.get(n, {}).get(c)
            cells.append("%-11s" % (f"{x} =" if x == y else f"{x}->{y}"))
            differ += x != y
        print("%-66s %s" % (label(n), " ".join(cells)))
    print("instantiations of the first build: %d, cells that differ: %d" % (len(a), differ))
    new = [n for n in b if n not in a]
    print()
    print("instantiations only the second build has: %d" % len(new))
    for n in new:
        print("%-66s %s" % (label(n), " ".join("%-11s" % b[n][c] for c in cols)))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
