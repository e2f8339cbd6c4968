"""Golden data for the adversarial meshes of tests/mesh_fuzz.py (its COMMITTED list), from the
reference built in place (oracle/_ref/ref_harness) — test infrastructure.

Per case the generated OBJ goes to <tmp>/Resources/<stem>.obj and the harness runs with
cwd = <tmp> (`scene file:<scene> t1,...,tk` for every prefix of the case's Update list, `render`
after the whole list).  Written to tests/golden/meshfuzz/<family>_<seed>.npz, data only:

  times                    the Update list
  after<k>                 per mesh, make_seq_goldens.mesh_digest after the first k Updates
  first_*, last_*          per mesh, after the first and after the last Update: nodes (nodesUsed),
                           leaf (triangles of the largest leaf), depth (levels, a lone root = 1),
                           inf (infinite words in the node bounds), negzero (-0 words in the world
                           positions and in the node bounds), triangles
  pixels_m3s1, rgb_m3s1, pixels_m0s1, rgb_m0s1    the reference's 44x28 frames after the list

The OBJ and scene texts are not committed: mesh_fuzz regenerates them at test time.  The files are
written with fixed zip timestamps, so a rerun reproduces them byte for byte.

Usage:  python tests/golden/make_mesh_goldens.py
"""
from __future__ import annotations

import io
import subprocess
import sys
import tempfile
import zipfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path[:0] = [str(HERE), str(HERE.parent)]
import rtxb  # noqa: E402
from make_goldens import HARNESS, ROOT  # noqa: E402
from make_seq_goldens import mesh_digest  # noqa: E402

OUT = HERE / "meshfuzz"
W, H = 44, 28
FRAMES = [(3, 1), (0, 1)]
FACTS = ("nodes", "leaf", "depth", "inf", "negzero", "triangles")


def harness(folder: Path, *args) -> dict:
    out = folder / "o.rtxb"
    subprocess.run([str(HARNESS), *map(str, args), str(out)], cwd=folder, check=True)
    return rtxb.read(out)


def shape_facts(d: dict, i: int) -> dict:
    p = f"mesh{i}_"
    links = d[p + "node_links"].reshape(-1, 3)
    bounds = d[p + "node_bounds"]
    depth, deepest, stack = {0: 1}, 1, [0]
    while stack:
        k = stack.pop()
        if links[k, 1] == 0:
            for c in (int(links[k, 2]), int(links[k, 2]) + 1):
                depth[c] = depth[k] + 1
                deepest = max(deepest, depth[c])
                stack.append(c)
    neg0 = np.uint32(0x80000000)
    return {"nodes": len(links), "leaf": int(links[:, 1].max()) // 3, "depth": deepest,
            "inf": int(np.isinf(bounds).sum()),
            "negzero": int((d[p + "tpositions"].view(np.uint32) == neg0).sum() + (bounds.view(np.uint32) == neg0).sum()),
            "triangles": len(d[p + "indices"]) // 3}


def save(path: Path, arrays: dict) -> None:
    """An .npz np.load reads, with fixed timestamps (np.savez stamps the entries with the clock)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def golden(case) -> dict:
    out = {"times": np.array(case.times, np.float32)}
    with tempfile.TemporaryDirectory() as td:
        folder = Path(td)
        name = f"file:{case.write(folder)}"
        n = len(case.times)
        for k in range(1, n + 1):
            d = harness(folder, "scene", name, case.time_list(k))
            meshes = range(len(d["meshes"]) // 5)
            out[f"after{k}"] = np.array([mesh_digest(d, i) for i in meshes])
            if k in (1, n):
                facts = [shape_facts(d, i) for i in meshes]
                for key in FACTS:
                    out[("first_" if k == 1 else "last_") + key] = np.array([f[key] for f in facts], np.int64)
                if n == 1:
                    for key in FACTS:
                        out["last_" + key] = out["first_" + key]
        for mode, sh in FRAMES:
            d = harness(folder, "render", name, case.time_list(), W, H, mode, sh, 8)
            out[f"pixels_m{mode}s{sh}"] = d["pixels"]
            out[f"rgb_m{mode}s{sh}"] = d["rgb"]
    return out


def main() -> None:
    import mesh_fuzz
    if not HARNESS.exists():
        subprocess.run(["make", "-s", "-C", str(ROOT / "oracle" / "ref"), str(HARNESS)], check=True)
    OUT.mkdir(exist_ok=True)
    for old in OUT.glob("*.npz"):
        old.unlink()
    for family, seed in mesh_fuzz.COMMITTED:
        case = mesh_fuzz.make(family, seed)
        g = golden(case)
        save(OUT / f"{case.name}.npz", g)
        print("meshfuzz", case.name, "T", list(g["first_triangles"]), "nodes", list(g["first_nodes"]),
              list(g["last_nodes"]), "leaf", list(g["first_leaf"]), list(g["last_leaf"]), "depth",
              list(g["first_depth"]), list(g["last_depth"]), "inf", list(g["last_inf"]), "-0",
              list(g["first_negzero"]), list(g["last_negzero"]), flush=True)


if __name__ == "__main__":
    main()
