"""Generate the golden fixtures of tests/golden/ from the REFERENCE ITSELF.

Runs only in the build container: needs /root/reference (the reference's sources are
compiled in place by oracle/ref/Makefile into oracle/_ref/ref_harness; nothing of the
reference is copied here).  The outputs are data only — inputs and expected outputs of
the reference's own functions:

  obj_<stem>.npz        Utils::ParseOBJ results for every Resources/*.obj
  scene_<name>[_t].npz  flattened scenes after Initialize (+ Update(t)): camera, spheres,
                        planes, lights, materials, mesh world positions / permuted indices /
                        normals / BVH nodes (large meshes: SHA-256 of each array)
  frame_<name>_<W>x<H>_m<mode>s<sh>[_t].npz   Renderer::Render output: uint32 pixels and
                        post-MaxToOne float RGB
  config_<name>_<W>x<H>.npz   full-resolution BASELINE configs: SHA-256 of the uint32
                        frame and of the float RGB plane + 4096 seeded sample pixels (index, uint32, rgb)
  prims.npz             primitive / BRDF known-answer vectors (GeometryUtils, Material::Shade)
  prims_domains.npz     the same primitives on the rows of tests/walk_domains.py (prim_rows): operands at the
                        edges of the ray kernels' fast-path domains
  scene_file_<stem>[_t].npz, frame_file_<stem>_128x72_m<mode>s<sh>[_t].npz
                        the same for the scene files in scenes/*.rtxscene, built by the
                        harness with the reference's own classes
  fuzz/<family>_<seed>.rtxscene, .npz   the seeded adversarial scenes of tests/scene_fuzz.py (the
                        generated text) and the reference's 44x28 frames of them, modes (3,1), (2,0)
  meshfuzz/<family>_<seed>.npz   the adversarial meshes of tests/mesh_fuzz.py (written by
                        make_mesh_goldens.py, not by this script): per-mesh digests after every prefix
                        of the case's Update list, shape facts of the reference's trees (nodes, largest
                        leaf, depth, inf and -0 words) and its 44x28 frames, modes (3,1), (0,1)

Usage:  python tests/golden/make_goldens.py [--scene-files-only | --configs-only | --fuzz-only | --prims-domains-only]

"""
from __future__ import annotations

import hashlib
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
sys.path.insert(0, str(HERE))
import rtxb  # noqa: E402

HARNESS = ROOT / "oracle" / "_ref" / "ref_harness"
REF_SRC = Path("/root/reference/source")
SCENES = ["W1", "W2", "W3", "W3_Test", "W4_Reference", "W4_Bunny", "W4_Optional", "Synthetic100k", "Bunny8Lights"]
ANIMATED = ["W4_Reference", "W4_Bunny", "W4_Optional", "Bunny8Lights"]
BIG = {"W4_Optional", "Synthetic100k"}
# BASELINE.json configs, then (round 3) the other two animated catalogue scenes at 1080p for the
# bench's parity_configs block; appended so the seeded sample indices of the first five stay put
CONFIGS = [("W1", 640, 480), ("W3", 1280, 720), ("W4_Bunny", 1920, 1080), ("Synthetic100k", 1920, 1080),
           ("Bunny8Lights", 3840, 2160), ("W4_Reference", 1920, 1080), ("W4_Optional", 1920, 1080)]


def run(*args) -> dict:
    with tempfile.TemporaryDirectory() as td:
        out = Path(td) / "o.rtxb"
        subprocess.run([str(HARNESS), *map(str, args), str(out)], cwd=REF_SRC, check=True)
        return rtxb.read(out)


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def tname(t: float) -> str:
    return "" if t < 0 else f"_t{t:g}"


SCENE_FILES = sorted((HERE.parents[1] / "scenes").glob("*.rtxscene"))
FILE_FRAMES = [(3, 1), (0, 1), (2, 0), (1, 1)]


def scene_files() -> None:
    for f in SCENE_FILES:
        name = f"file:{f}"
        for t in (-1.0, 1.3):
            d = run("scene", name, t)
            np.savez_compressed(HERE / f"scene_file_{f.stem}{tname(t)}.npz", **d)
            for mode, sh in FILE_FRAMES:
                d = run("render", name, t, 128, 72, mode, sh, 8)
                np.savez_compressed(HERE / f"frame_file_{f.stem}_128x72_m{mode}s{sh}{tname(t)}.npz",
                                    pixels=d["pixels"], rgb=d["rgb"])
        print("scene file", f.name, flush=True)


FUZZ_DIR = HERE / "fuzz"
FUZZ_W, FUZZ_H = 44, 28          # five wave tiles and a half across, three and a half down
FUZZ_FRAMES = [(3, 1), (2, 0)]


def fuzz() -> None:
    """The seeded scenes of tests/scene_fuzz.py (its COMMITTED list): the generated text as
    fuzz/<family>_<seed>.rtxscene and the reference's frames of it as fuzz/<family>_<seed>.npz
    (pixels_m<mode>s<sh>, rgb_m<mode>s<sh>).  The harness alone is needed (no HIP library)."""
    sys.path.insert(0, str(HERE.parent))
    import scene_fuzz
    if not HARNESS.exists():
        subprocess.run(["make", "-s", "-C", str(ROOT / "oracle" / "ref"), str(HARNESS)], check=True)
    FUZZ_DIR.mkdir(exist_ok=True)
    for old in list(FUZZ_DIR.glob("*.rtxscene")) + list(FUZZ_DIR.glob("*.npz")):
        old.unlink()
    for family, seed in scene_fuzz.COMMITTED:
        fs = scene_fuzz.make(family, seed)
        f = FUZZ_DIR / f"{fs.name}.rtxscene"
        f.write_text(fs.text)
        out = {}
        for mode, sh in FUZZ_FRAMES:
            d = run("render", f"file:{f}", -1, FUZZ_W, FUZZ_H, mode, sh, 8)
            out[f"pixels_m{mode}s{sh}"] = d["pixels"]
            out[f"rgb_m{mode}s{sh}"] = d["rgb"]
        np.savez_compressed(FUZZ_DIR / f"{fs.name}.npz", **out)
        print("fuzz", fs.name, flush=True)


def prims_domains() -> None:
    """tests/walk_domains.py's rows through the reference's own HitTest_* and SlabTest_BVH."""
    sys.path.insert(0, str(HERE.parent))
    import walk_domains
    with tempfile.TemporaryDirectory() as td:
        rows = Path(td) / "rows.f32"
        walk_domains.prim_rows().tofile(rows)
        d = run("primrows", rows)
    np.savez_compressed(HERE / "prims_domains.npz", **d)


def main() -> None:
    if "--fuzz-only" in sys.argv:
        fuzz()
        return
    assert HARNESS.exists(), "build oracle/_ref first (python -m gp1_raytracer_2223_amd.build)"
    if "--prims-domains-only" in sys.argv:
        prims_domains()
        return
    if "--scene-files-only" in sys.argv:
        scene_files()
        return
    if "--configs-only" in sys.argv:
        configs()
        return
    scene_files()
    fuzz()
    for obj in sorted(REF_SRC.glob("Resources/*.obj")):
        d = run("obj", obj.relative_to(REF_SRC))
        np.savez_compressed(HERE / f"obj_{obj.stem}.npz", **d)

    for name in SCENES:
        for t in ([-1.0, 1.3] if name in ANIMATED else [-1.0]):
            d = run("scene", name, t)
            if name in BIG:
                d = {k: (np.array([sha(v)]) if k.startswith("mesh") and k != "meshes" else v) for k, v in d.items()}
            np.savez_compressed(HERE / f"scene_{name}{tname(t)}.npz", **d)
            d = run("render", name, t, 128, 72, 3, 1, 8)
            np.savez_compressed(HERE / f"frame_{name}_128x72_m3s1{tname(t)}.npz", pixels=d["pixels"], rgb=d["rgb"])

    for name in ["W3", "W3_Test", "W4_Reference", "W2"]:
        for mode in range(4):
            for sh in (0, 1):
                d = run("render", name, -1, 64, 48, mode, sh, 8)
                np.savez_compressed(HERE / f"frame_{name}_64x48_m{mode}s{sh}.npz", pixels=d["pixels"], rgb=d["rgb"])

    configs()

    d = run("prims", 1234, 1500)
    np.savez_compressed(HERE / "prims.npz", **d)
    prims_domains()


def configs() -> None:
    rng = np.random.default_rng(2223)
    for name, W, H in CONFIGS:
        d = run("render", name, -1, W, H, 3, 1, 8)
        px, rgb = d["pixels"], d["rgb"].reshape(-1, 3)
        idx = np.sort(rng.choice(W * H, 4096, replace=False)).astype(np.int64)
        np.savez_compressed(HERE / f"config_{name}_{W}x{H}.npz", sha_pixels=np.array([sha(px)]),
                            sha_rgb=np.array([sha(rgb)]), idx=idx, pixels=px[idx], rgb=rgb[idx])
        print(name, W, H, sha(px)[:16], flush=True)


if __name__ == "__main__":
    main()
