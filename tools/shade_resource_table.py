"""Resource usage of the shaded-ray kernels (rtx_shade_kernel<DEEP, HSTK>) of a librtx_hip.so, read from
the gfx950 code object (no GPU needed), beside the query kernels' (tools/rayq_resource_table.py):

    python tools/shade_resource_table.py this/librtx_hip.so

Per kernel: VGPR, SGPR, scratch, LDS and the waves per SIMD that follow from them, and the
s_load_dwordx16 / global_load / global_store counts of its disassembly."""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
import aov_resource_table as art  # noqa: E402
import rayq_resource_table as rrt  # noqa: E402

LLVM = art.LLVM


def shade_kernels(lib: str) -> dict:
    with tempfile.TemporaryDirectory() as td:
        fb, co = Path(td) / "fatbin.bin", Path(td) / "gfx950.co"
        subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, str(fb)], check=True)
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fb}", f"--output={co}"], check=True)
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", str(co)], check=True, capture_output=True,
                               text=True).stdout
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--mcpu=gfx950", str(co)], check=True, capture_output=True,
                             text=True).stdout
    out = {}
    for m in re.finditer(r"^[0-9a-f]+ <(_Z16rtx_shade_kernelILb([01])ELb([01])E\w+)>:", dis, re.M):
        name = m.group(1)
        nxt = re.compile(r"^[0-9a-f]+ <", re.M).search(dis, m.end())   # (a kernel may end in several places)
        body = dis[m.end():nxt.start() if nxt else len(dis)]
        rec = {"DEEP": int(m.group(2)), "HSTK": int(m.group(3))}
        for block in notes.split("  - .")[1:]:
            if re.search(rf"\.name:\s+{name}\b", block):
                for key, short in art.KEYS + [("agpr_count", "AGPR")]:
                    mm = re.search(rf"\.{key}:\s+(\d+)", block)
                    rec[short] = int(mm.group(1)) if mm else 0
        regs = -(-(rec["VGPR"] + rec["AGPR"]) // 8) * 8
        occ = min(8, 512 // max(regs, 8))
        if rec["LDS"]:
            occ = min(occ, max(1, (160 * 1024 // rec["LDS"]) // 4))
        rec["occ"] = occ
        rec["x16"] = body.count("s_load_dwordx16")
        rec["vload"] = len(re.findall(r"\bglobal_load_", body))
        rec["vstore"] = len(re.findall(r"\bglobal_store_", body))
        rec["insts"] = sum(1 for ln in body.splitlines() if re.match(r"\s+[a-z_0-9]+ ", ln))
        out[name] = rec
    return out


def main() -> int:
    if len(sys.argv) != 2:
        print(__doc__)
        return 2
    head = "VGPR  SGPR  scratch  LDS    occ  s_load_dwordx16  global_load  global_store  instructions"
    print(f"{'rtx_shade_kernel<...>':44s} {head}")
    for name, r in sorted(shade_kernels(sys.argv[1]).items(), key=lambda kv: (kv[1]["DEEP"], kv[1]["HSTK"])):
        label = f"DEEP={r['DEEP']} HSTK={r['HSTK']}"
        print(f"{label:44s} {r['VGPR']:<5d} {r['SGPR']:<5d} {r['scratch']:<8d} {r['LDS']:<6d} {r['occ']:<4d} "
              f"{r['x16']:<16d} {r['vload']:<12d} {r['vstore']:<13d} {r['insts']}")
    print()
    print(f"{'rtx_query_kernel<...>':44s} {head}")
    for name, r in sorted(rrt.query_kernels(sys.argv[1]).items(), key=lambda kv: (kv[1]["ANY"], kv[1]["DEEP"], kv[1]["HSTK"])):
        label = f"ANY={r['ANY']} DEEP={r['DEEP']} HSTK={r['HSTK']}"
        print(f"{label:44s} {r['VGPR']:<5d} {r['SGPR']:<5d} {r['scratch']:<8d} {r['LDS']:<6d} {r['occ']:<4d} "
              f"{r['x16']:<16d} {r['vload']:<12d} {r['vstore']:<13d} {r['insts']}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
