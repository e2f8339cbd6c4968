"""Resource usage of the adaptive-supersampling kernels (rtx_adaptive_kernel<DEEP, HSTK>, rtx_classify_kernel)
of a librtx_hip.so beside the shade kernel's they restate, read from the gfx950 code objects (no GPU needed):

    python tools/adaptive_resource_table.py this/librtx_hip.so

Per kernel: VGPR, SGPR, scratch (private segment), LDS, the waves per SIMD that follow from them, and the
instruction count of its disassembly."""
import re
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
import codeobj_diff as cd  # noqa: E402

WANTED = re.compile(r"^_Z\d+(rtx_adaptive_kernel|rtx_shade_kernel|rtx_classify_kernel)")


def waves_per_simd(vgpr: int, lds: int, wg_waves: int) -> int:
    regs = -(-vgpr // 8) * 8
    occ = min(8, 512 // max(regs, 8))
    if lds:   # 160 KB per CU over its 4 SIMDs
        occ = min(occ, max(1, (160 * 1024 // lds) * wg_waves // 4))
    return occ


def label(name: str) -> str:
    m = re.match(r"^_Z\d+(\w+?)(?:ILb([01])ELb([01])E|N4rtxd)", name)
    if m and m.group(2) is not None:
        return f"{m.group(1)}<DEEP={m.group(2)}, HSTK={m.group(3)}>"
    return m.group(1) if m else name


def main() -> int:
    if len(sys.argv) != 2:
        print(__doc__)
        return 2
    with tempfile.TemporaryDirectory() as t:
        _, meta, dis = cd.library_kernels(Path(sys.argv[1]), Path(t))
    print(f"{'kernel':44s} VGPR  SGPR  scratch  LDS    waves/SIMD  instructions")
    for name in sorted(k for k in meta if WANTED.match(k)):
        m = meta[name]
        vgpr, sgpr = int(m["vgpr_count"]), int(m["sgpr_count"])
        lds, scratch = int(m["group_segment_fixed_size"]), int(m["private_segment_fixed_size"])
        wg = max(1, int(m["max_flat_workgroup_size"]) // 64)
        print(f"{label(name):44s} {vgpr:<5d} {sgpr:<5d} {scratch:<8d} {lds:<6d} {waves_per_simd(vgpr, lds, wg):<11d} "
              f"{len(dis.get(name, []))}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
