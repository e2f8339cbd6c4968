"""Scenes and cameras at the exact cull's own operand bounds — TEST INFRASTRUCTURE
(tests/test_cull_cases_cpu.py, tests/test_gpu_cull_fuzz.py).

The walks' fast-path bounds have tests/walk_domains.py; these are the bounds only a culling context reads
(rtx_cull_records.hip, cull_ray and cull_pass of rtx_hip.hip):

  coord    cull_domain: a triangle whose v0, e1 or e2 has a component beyond 2^40 gets the box (-inf, +inf), and
           every slot above it the always-pass record.  Twelve right triangles with legs 2^27 stacked 2^22 apart
           in z, as walk_domains' `giant` but 2^40 - 2^27 along x, the fifth (the one the camera looks at) with
           its v0.x exactly 2^40, or one float above.  Legs of 2^27 keep |e1||e2| = 2^54.5 and
           (|v0|_1 + 2^40)(|e1|_1 + |e2|_1) < 2^71: the scene stays tri_fast, so the culled walks run.
  camera   cull_ray's ok: |o_k| <= 2^40.  `giant` seen from x = 2^40 (or one float above), z = 2^24 - 2^40, looking
           back at the stack along (-1, 0, 1) through a frame 3e-4 wide: about a fifth of the pixels hit it.
  bt       cull_pass prunes by t only while sc_t <= bt = 4 R + 1 (R: the camera's distance to the farthest corner
           of the meshes' box).  Twelve small triangles spread over a wide box, a wall behind them whose distance
           along the primary rays runs from 0.97 bt in the middle of the frame to 1.2 bt at its edges, and a
           sphere before a part of the mesh (a small sc_t before the mesh walk).

mag <= cull_T, mag = 0 and mixed waves have test_gpu_cull.test_cull_adversarial_lights; T >= 2^60 has `needle`
(cull_cases.ZERO_T).  |inv_k| <= 2^64 cannot be reached: a direction normalised from a magnitude of at least 2^-30
has |d_k| >= 2^-64 or d_k = 0 exactly, and a zero component makes the wave slow, which never culls.

Lambert only, one point light: no powf, every comparison word for word."""
from __future__ import annotations

from pathlib import Path

import numpy as np

import mesh_fuzz
import walk_domains as WD
from scene_fuzz import fmt

F32 = np.float32
TWO40 = 2.0 ** 40
LEG, DZ, ODD = 2.0 ** 27, 2.0 ** 22, 4      # coord: the legs, the spacing, the triangle at the bound
COORD = ("coord_at", "coord_past")
BT = "bt_straddle"


def coord_x(past: bool) -> float:
    return float(WD.up(TWO40)) if past else TWO40


def coord_texts(past: bool):
    """(OBJ stem, OBJ text, scene text): triangle k = (C, A, B) with A = (S, 0, z), B = (S, LEG, z) and
    C = (S + LEG, 0, z), S = 2^40 - LEG; v0 = C, whose x is 2^40 - 2^20 but for triangle ODD."""
    S = TWO40 - LEG
    verts, faces = [], []
    for k in range(WD.N_TRI):
        z = DZ * k
        cx = coord_x(past) if k == ODD else TWO40 - 2.0 ** 20
        verts += [(S, 0.0, z), (S, LEG, z), (cx, 0.0, z)]
        faces.append((3 * k + 2, 3 * k, 3 * k + 1))
    stem = "cd_coord"
    camera = (S + LEG / 2, LEG / 2 - 2.0 ** 18, DZ * ODD - 2.0 ** 20)
    light = (S + LEG / 2 + 2.0 ** 21, LEG / 2 + 2.0 ** 21, -2.0 ** 26, 2.0 ** 53)
    rows = [f"# cull_domains coord {'past' if past else 'at'}",
            " ".join(["camera"] + [fmt(x) for x in (*camera, 45.0)]),
            "material lambert 0.9 0.75 0.49 1",
            " ".join(["plane", fmt(S - 2.0 ** 30), "0", "0", "1", "0", "0", "1"]),
            f"mesh {stem} 1 none",
            " ".join(["light", "point"] + [fmt(x) for x in light] + ["1", "0.9", "0.75"])]
    return stem, mesh_fuzz.obj_text(np.array(verts, np.float32), faces), "\n".join(rows) + "\n"


BT_CAMERA = (0.0, 2.5, -8.0)
BT_LO, BT_HI = (-4.0, 0.25, 0.0), (4.0, 4.5, 2.0)


def _bt_soup():
    """Twelve triangles of size 0.3 whose corners span BT_LO .. BT_HI exactly (the first two reach the corners)."""
    rng = np.random.default_rng((2223, 40))
    v, f = mesh_fuzz._soup(rng, 12, BT_LO, BT_HI, 0.3)
    v = np.clip(v, BT_LO, BT_HI).astype(np.float32)
    v[0], v[3] = BT_LO, BT_HI
    return v, f


def bt_bound() -> float:
    """bt of the file's camera as frame_shape computes it: 4 x the farthest corner of the meshes' box + 1."""
    lo, hi, o = np.array(BT_LO), np.array(BT_HI), np.array(BT_CAMERA)
    R = max(np.linalg.norm(o - np.where([k & 1, k & 2, k & 4], hi, lo)) for k in range(8))
    return 4.0 * R + 1.0


def bt_texts():
    v, f = _bt_soup()
    wall = float(F32(0.97 * bt_bound() + BT_CAMERA[2]))      # the middle ray meets it at 0.97 bt
    rows = ["# cull_domains bt", " ".join(["camera"] + [fmt(x) for x in (*BT_CAMERA, 45.0)]),
            "material lambert 0.9 0.75 0.49 1",
            " ".join(["plane", "0", "0", fmt(wall), "0", "0", "-1", "1"]),
            "sphere -1.5 2.5 -3 1 1",
            "mesh cd_bt 1 none",
            "light point 2 7 -6 70 1 0.9 0.75"]
    return "cd_bt", mesh_fuzz.obj_text(v, f), "\n".join(rows) + "\n"


def write(name: str, folder) -> Path:
    """Write the scene `name` (COORD or BT) into `folder`/<name>; returns the scene file (its folder holds the OBJ)."""
    stem, obj, text = bt_texts() if name == BT else coord_texts(name == "coord_past")
    d = Path(folder) / name
    d.mkdir(parents=True, exist_ok=True)
    (d / f"{stem}.obj").write_text(obj)
    path = d / f"{name}.rtxscene"
    path.write_text(text)
    return path


def host_scene(name: str, folder):
    """(HostScene, rtx_scene, camera); keep the first alive while the others are in use."""
    from gp1_raytracer_2223_amd.scene import HostScene
    path = write(name, folder)
    hs = HostScene(f"file:{path}", asset_dir=str(path.parent))
    return (hs, *hs.view())


def far_camera(past: bool):
    """The camera of the `camera` bound for walk_domains' `giant`: x = 2^40 or one float above."""
    from gp1_raytracer_2223_amd import abi
    o = np.array([coord_x(past), 2.0 ** 27, 2.0 ** 24 - TWO40])
    f = np.array([2.0 ** 27, 2.0 ** 27, 2.0 ** 24]) - o
    f /= np.linalg.norm(f)
    r = np.cross([0.0, 1.0, 0.0], f)
    r /= np.linalg.norm(r)
    cam = abi.Camera()
    cam.origin[:] = [float(F32(x)) for x in o]
    cam.right[:] = [float(F32(x)) for x in r]
    cam.up[:] = [float(F32(x)) for x in np.cross(f, r)]
    cam.forward[:] = [float(F32(x)) for x in f]
    cam.fov = 1.5e-4
    return cam


def primary_rays(cam, width: int, height: int):
    """(origin, directions (n, 3)) of a frame's primary rays before normalisation, in double: Renderer.cpp's
    cx, cy of the pixel centres times the camera's axes."""
    px, py = np.meshgrid(np.arange(width) + 0.5, np.arange(height) + 0.5)
    cx = (2.0 * px / width - 1.0) * (width / height) * cam.fov
    cy = (1.0 - 2.0 * py / height) * cam.fov
    axes = [np.array(a[:], np.float64) for a in (cam.right, cam.up, cam.forward)]
    d = cx.reshape(-1, 1) * axes[0] + cy.reshape(-1, 1) * axes[1] + axes[2]
    return np.array(cam.origin[:], np.float64), d


def meets_box(o, d, lo, hi) -> np.ndarray:
    """Per ray, whether the half-line o + t d, t > 0, meets the box [lo, hi] (double; no component of d is 0)."""
    t1, t2 = (np.asarray(lo) - o) / d, (np.asarray(hi) - o) / d
    near, far = np.minimum(t1, t2).max(axis=1), np.maximum(t1, t2).min(axis=1)
    return (far > 0) & (far >= near)
