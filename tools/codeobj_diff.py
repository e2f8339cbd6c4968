"""Compare the gfx950 device code of two builds of a HIP library, kernel by kernel.

    python tools/codeobj_diff.py OLD.so NEW.so

Every gfx950 code object of each library's fat binary is extracted (a library linked from several
units carries one per unit) and the kernels of all of them are taken together, so moving a kernel to
another unit is no difference.  Reported: kernels present in one library only; kernels whose
disassembly differs (the address column and the padding after the last instruction stripped); and
kernels whose resource metadata differs (VGPR / SGPR count, LDS size, private segment size, kernarg
size, max flat workgroup size).  Exit status 0 only when nothing differs.
"""
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
META_KEYS = {"vgpr_count": "VGPRs", "sgpr_count": "SGPRs", "group_segment_fixed_size": "LDS bytes",
             "private_segment_fixed_size": "private segment bytes", "kernarg_segment_size": "kernarg bytes",
             "max_flat_workgroup_size": "max flat workgroup size"}
PADDING = re.compile(r"^(\.\.\.|s_nop\b.*|s_code_end)$")


def _tool(name, *args):
    return subprocess.run([f"{LLVM}/{name}", *args], check=True, capture_output=True, text=True).stdout


def code_objects(lib: Path, tmp: Path) -> list[Path]:
    """The gfx950 code objects of every offload bundle in the library's .hip_fatbin section."""
    fb = tmp / (lib.name + ".fatbin")
    _tool("llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", str(lib), str(fb))
    data = fb.read_bytes()
    starts = [m.start() for m in re.finditer(re.escape(BUNDLE_MAGIC), data)] or [0]
    out = []
    for k, (a, b) in enumerate(zip(starts, starts[1:] + [len(data)])):
        piece, co = tmp / f"{lib.name}.{k}.bundle", tmp / f"{lib.name}.{k}.co"
        piece.write_bytes(data[a:b])
        listed = _tool("clang-offload-bundler", "--list", "--type=o", f"--input={piece}")
        if TARGET not in listed.split():
            continue
        _tool("clang-offload-bundler", "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={piece}",
              f"--output={co}")
        if co.stat().st_size:
            out.append(co)
    return out


def kernel_meta(co: Path) -> dict[str, dict[str, str]]:
    """name -> the META_KEYS of each entry of the code object's amdhsa.kernels note."""
    kernels = []
    for line in _tool("llvm-readelf", "--notes", str(co)).splitlines():
        m = re.match(r"^  (- | {2})\.(\w+):\s*(.*)$", line)   # a kernel's own keys start in column 4
        if not m:
            continue
        if m.group(1) == "- ":
            kernels.append({})
        if kernels:
            kernels[-1][m.group(2)] = m.group(3).strip()
    return {k["name"]: {key: k.get(key, "?") for key in META_KEYS} for k in kernels if "name" in k}


def disassembly(co: Path, names: set[str]) -> dict[str, list[str]]:
    """name -> its instructions (mnemonic, operands and encoding; no addresses, no trailing padding)."""
    out, cur = {}, None
    for line in _tool("llvm-objdump", "-d", "--mcpu=gfx950", str(co)).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), []) if m.group(1) in names else None
            continue
        if cur is None or not line.strip():
            continue
        text, _, comment = line.strip().partition("//")
        enc = re.sub(r"^\s*[0-9A-Fa-f]+:\s*", "", comment)        # the address column
        enc = re.sub(r"\s*<[^>]*>\s*$", "", enc)                  # a branch target's symbol + offset
        cur.append((text.strip() + "  " + enc.strip()).strip())
    for body in out.values():
        while body and PADDING.match(body[-1].split("  ")[0].strip()):
            body.pop()
    return out


def library_kernels(lib: Path, tmp: Path):
    meta, dis = {}, {}
    cos = code_objects(lib, tmp)
    for co in cos:
        m = kernel_meta(co)
        meta.update(m)
        dis.update(disassembly(co, set(m)))
    return len(cos), meta, dis


def main() -> int:
    if len(sys.argv) != 3:
        print(__doc__)
        return 2
    old, new = Path(sys.argv[1]), Path(sys.argv[2])
    with tempfile.TemporaryDirectory() as t:
        (Path(t) / "old").mkdir()
        (Path(t) / "new").mkdir()
        n_old, meta_old, dis_old = library_kernels(old, Path(t) / "old")
        n_new, meta_new, dis_new = library_kernels(new, Path(t) / "new")
    print(f"old: {old.name}: {n_old} gfx950 code objects, {len(meta_old)} kernels")
    print(f"new: {new.name}: {n_new} gfx950 code objects, {len(meta_new)} kernels")
    only_old, only_new = sorted(set(meta_old) - set(meta_new)), sorted(set(meta_new) - set(meta_old))
    both = sorted(set(meta_old) & set(meta_new))
    code_diff = [k for k in both if dis_old.get(k) != dis_new.get(k)]
    meta_diff = [k for k in both if meta_old[k] != meta_new[k]]
    for title, names in (("only in old", only_old), ("only in new", only_new)):
        print(f"kernels {title}: {len(names)}")
        for k in names:
            print(f"  {k}")
    print(f"kernels in both: {len(both)}")
    print(f"  disassembly differs: {len(code_diff)}")
    for k in code_diff:
        a, b = dis_old.get(k, []), dis_new.get(k, [])
        first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        print(f"    {k}: {len(a)} -> {len(b)} instructions, first difference at instruction {first}")
    print(f"  metadata differs: {len(meta_diff)}")
    for k in meta_diff:
        what = ", ".join(f"{META_KEYS[key]} {meta_old[k][key]} -> {meta_new[k][key]}" for key in META_KEYS
                         if meta_old[k][key] != meta_new[k][key])
        print(f"    {k}: {what}")
    same = not (only_old or only_new or code_diff or meta_diff)
    if same:
        n_instr = sum(len(dis_new.get(k, [])) for k in both)
        print(f"identical: {len(both)} kernels, {n_instr} instructions, same resource metadata")
    else:
        print("DIFFERENT")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
