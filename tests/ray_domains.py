"""Rays, scenes and cameras at the edges of the merged ray-domain test — TEST INFRASTRUCTURE
(tests/test_ray_domains_cpu.py, tests/test_gpu_ray_domains.py).

csrc/rtx_fastdiv.h `norm_ray3` computes a ray's square root, normalisation and reciprocals with the fast
forms in every lane and decides with ONE test which lanes take the IEEE forms: with l the direction before
the normalisation, s = (l_x^2 + l_y^2) + l_z^2 in binary32 and d = l / sqrt(s),
    2^-96 <= s <= 2^120   and   min |l_k| >= 2^-60   and   min |d_k| >= 2^-60.
This module builds shadow rays and primary rays on either side of each of these bounds, lane by lane.

Shadow rays.  The scenes have one plane z = -0.0001f with the normal +z, one triangle far to the side and
one point light at (0, 0, Lz).  A caller's ray {(x0, y0, 0), (0, 0, -1), 0, FLT_MAX} hits the plane at
t = 0.0001f, its hit point is (x0, y0, -0.0001f) and its shadow origin (x0, y0, 0) exactly, so the shadow
ray's direction before the normalisation is l = (-x0, -y0, Lz): every lane chooses its own l_x and l_y.
  `low`    Lz = 2^-60: s around 2^-96, the smallest |l_k| at 2^-60 and below, s around 2^120
  `norm`   Lz = 2^-30: the smallest normalised component at 2^-60 and below
  `tiny`   Lz = 2^-70: s a denormal (every ray outside)
  `zero`   Lz = 0:     s = 0, from l = 0 and from squares that underflow (every ray outside)
  `far`    Lz = 2^62:  the light beyond 2^60 (every ray outside)

Primary rays.  `cameras` returns cameras for an 8 x 8 and a 16 x 8 frame whose direction before the
normalisation is (r cx, cy, 1) with r chosen so that the columns next to the centre have |d_x| below 2^-60
(a wave inside but for those lanes), and cameras whose whole frame lies below 2^-96 or above 2^120."""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np
import pytest

import mesh_fuzz
from scene_fuzz import fmt
from gp1_raytracer_2223_amd import abi

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
P2 = lambda e: F32(2.0) ** F32(e)      # noqa: E731  (exact powers of two)
PLANE_Z = -F32(0.0001)
MIXED_LANES = (0, 17, 63)
LAYOUT = ("in", "out") + tuple(f"lane{k}" for k in MIXED_LANES)


@pytest.fixture(scope="module")
def generic_ctx():
    """A context of the generic kernels (RTX_NO_SPEC=1, read once at creation), one per importing module."""
    from gp1_raytracer_2223_amd.renderer import DeviceContext
    from gpu_support import DEV
    os.environ["RTX_NO_SPEC"] = "1"
    try:
        c = DeviceContext(DEV)
    finally:
        os.environ.pop("RTX_NO_SPEC")
    yield c
    c.close()


def dn(x) -> np.float32:
    """One binary32 below x (towards zero for a positive x)."""
    return np.nextafter(F32(x), F32(0))


def up(x) -> np.float32:
    return np.nextafter(F32(x), F32(np.inf))


LZ = {"low": P2(-60), "norm": P2(-30), "tiny": P2(-70), "zero": F32(0), "far": P2(62)}
SCENES = tuple(LZ)


def scene_texts(name: str, mixed: bool = False):
    """(OBJ stem, OBJ text, scene text).  mixed: a solid-colour material on the plane instead (no Lambert-only variant)."""
    verts = np.array([(100, 0, -1), (101, 0, -1), (100, 1, -1)], np.float32)
    rows = [f"# ray_domains {name}", "camera 0 0 1 45",
            "material solid 0.9 0.75 0.49" if mixed else "material lambert 0.9 0.75 0.49 1",
            " ".join(["plane", "0", "0", fmt(PLANE_Z), "0", "0", "1", "1"]),
            "mesh rd_tri 1 none",
            " ".join(["light", "point", "0", "0", fmt(LZ[name]), "3", "1", "0.9", "0.75"])]
    return "rd_tri", mesh_fuzz.obj_text(verts, [(0, 1, 2)]), "\n".join(rows) + "\n"


def host_scene(name: str, folder, mixed: bool = False):
    """(HostScene, rtx_scene, camera); keep the first alive while the others are in use."""
    from gp1_raytracer_2223_amd.scene import HostScene
    d = Path(folder) / (name + ("_mixed" if mixed else ""))
    d.mkdir(parents=True, exist_ok=True)
    stem, obj, text = scene_texts(name, mixed)
    (d / f"{stem}.obj").write_text(obj)
    path = d / f"rd_{name}.rtxscene"
    path.write_text(text)
    hs = HostScene(f"file:{path}", asset_dir=str(path.parent))
    return (hs, *hs.view())


# ----------------------------------------------------------------------------------------------- shadow rays

def _rays(lx, ly):
    """Caller's rays whose shadow rays have l = (lx, ly, Lz)."""
    n = len(lx)
    r = np.zeros((n, 8), np.float32)
    r[:, 0], r[:, 1] = -np.asarray(lx, np.float32), -np.asarray(ly, np.float32)
    r[:, 5] = -1.0
    r[:, 7] = FLT_MAX
    return r


def _spread(rng, n, lo_e, hi_e):
    """Random magnitudes 2^lo_e .. 2^hi_e with random signs, in binary32."""
    return (np.exp2(rng.uniform(lo_e, hi_e, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


# class -> (scene, generator of (lx, ly) for n rays, inside the domain?)
def _const(x, y):
    return lambda rng, n: (np.full(n, x, np.float32) * rng.choice(F32([-1, 1]), n), np.full(n, y, np.float32))


CLASSES = {
    # s: 2^-96 exactly (2^-96 + 2^-120 + 2^-120, both ties to even), two floats below it, far inside
    "low_in": ("low", lambda rng, n: (_spread(rng, n, -47, -40), _spread(rng, n, -47, -40)), True),
    "s_at_2m96": ("low", _const(P2(-48), P2(-60)), True),
    "s_below_2m96": ("low", _const(dn(dn(P2(-48))), P2(-60)), False),
    # the smallest |l_k|: 2^-60 is every `low` ray's l_z; one float below it in l_y
    "l_below_2m60": ("low", lambda rng, n: (_spread(rng, n, -47, -40), np.full(n, dn(P2(-60)), np.float32)), False),
    # s: 2^120 exactly (l_x = 2^60, the others vanish in the sum), the next float's square above it, 2^124
    "s_at_2p120": ("low", _const(P2(60), P2(-50)), False),   # (outside all the same: d_z = 2^-120)
    "s_above_2p120": ("low", _const(up(P2(60)), P2(-50)), False),
    "s_2p124": ("low", _const(P2(62), P2(20)), False),
    # the smallest normalised component: l_y / 2^20 = 2^-60 and one float below
    "norm_in": ("norm", lambda rng, n: (_spread(rng, n, -20, 0), _spread(rng, n, -20, 0)), True),
    "d_at_2m60": ("norm", _const(P2(20), P2(-40)), True),
    "d_below_2m60": ("norm", _const(P2(20), dn(P2(-40))), False),
    "s_at_2p120_in": ("norm", _const(P2(60), P2(30)), False),   # (d_z = 2^-90: outside by the third test only)
    # s a denormal, s zero
    "s_denormal": ("tiny", lambda rng, n: (_spread(rng, n, -69, -65), _spread(rng, n, -69, -65)), False),
    "s_zero_vector": ("zero", _const(F32(0), F32(0)), False),
    "s_zero_underflow": ("zero", lambda rng, n: (_spread(rng, n, -100, -80), _spread(rng, n, -100, -80)), False),
    "light_far": ("far", lambda rng, n: (_spread(rng, n, -3, 3), _spread(rng, n, -3, 3)), False),
}
INSIDE_OF = {"low": "low_in", "norm": "norm_in"}
OUTSIDE_OF = {s: tuple(c for c, (sc, _, ins) in CLASSES.items() if sc == s and not ins) for s in SCENES}
EDGE_INSIDE = {"low": ("s_at_2m96",), "norm": ("d_at_2m60",)}


def waves(scene: str, seed: int = 1):
    """(rays, class name per ray).  `low` and `norm`: five waves as LAYOUT says (the inside wave ends with
    eight rays of each inside edge class; the outside rays cycle through the scene's outside classes).  The
    other scenes: one wave per class, all outside."""
    rng = np.random.default_rng((2223, 31, SCENES.index(scene), seed))
    rays, names = [], []

    def add(cls, n):
        lx, ly = CLASSES[cls][1](rng, n)
        rays.append(_rays(lx, ly))
        names.extend([cls] * n)

    outs = OUTSIDE_OF[scene]
    if scene not in INSIDE_OF:
        for c in outs:
            add(c, 64)
        return np.concatenate(rays), np.array(names)
    ins = INSIDE_OF[scene]
    add(ins, 64 - 8 * len(EDGE_INSIDE[scene]))
    for c in EDGE_INSIDE[scene]:
        add(c, 8)
    for k in range(64):
        add(outs[k % len(outs)], 1)
    for j, lane in enumerate(MIXED_LANES):
        add(ins, lane)
        add(outs[j % len(outs)], 1)
        add(ins, 63 - lane)
    return np.concatenate(rays), np.array(names)


def shadow_l(scene: str, rays: np.ndarray):
    """l = L - originOffset per ray in binary32, from the ray alone, in the reference's order: t = num / den
    of HitTest_Plane, hit.origin = o + d * t, originOffset = hit.origin + n * 0.0001f."""
    r = np.ascontiguousarray(rays, np.float32)
    o, d = r[:, 0:3], r[:, 3:6]
    n = np.array([0, 0, 1], np.float32)
    p0 = np.array([0, 0, PLANE_Z], np.float32)
    with np.errstate(all="ignore"):
        num = (((p0 - o)[:, 0] * n[0] + (p0 - o)[:, 1] * n[1]).astype(np.float32) + (p0 - o)[:, 2] * n[2]).astype(np.float32)
        den = ((d[:, 0] * n[0] + d[:, 1] * n[1]).astype(np.float32) + d[:, 2] * n[2]).astype(np.float32)
        t = (num / den).astype(np.float32)
        h = (o + (d * t[:, None]).astype(np.float32)).astype(np.float32)
        oo = (h + (n * F32(0.0001))[None, :].astype(np.float32)).astype(np.float32)
        L = np.array([0, 0, LZ[scene]], np.float32)
        return (L[None, :] - oo).astype(np.float32), t


def domain_facts(l: np.ndarray) -> dict:
    """The three tests of norm_ray3 per direction l (n, 3), in binary32."""
    l = np.ascontiguousarray(l, np.float32)
    with np.errstate(all="ignore"):
        s = ((l[:, 0] * l[:, 0] + l[:, 1] * l[:, 1]).astype(np.float32) + l[:, 2] * l[:, 2]).astype(np.float32)
        m = np.sqrt(s).astype(np.float32)
        d = (l / m[:, None]).astype(np.float32)
        lo = np.abs(l).min(axis=1)
        dlo = np.where(np.isnan(d).any(axis=1), F32(np.nan), np.abs(d).min(axis=1))
        s_ok = (s >= P2(-96)) & (s <= P2(120))
        l_ok = lo >= P2(-60)
        d_ok = dlo >= P2(-60)
    return {"s": s, "lo": lo, "dlo": dlo, "s_ok": s_ok, "l_ok": l_ok, "d_ok": d_ok, "inside": s_ok & l_ok & d_ok}


# --------------------------------------------------------------------------------------------- primary rays

def _camera(origin, right, up_, forward, fov) -> abi.Camera:
    c = abi.Camera()
    for k in range(3):
        c.origin[k], c.right[k], c.up[k], c.forward[k] = origin[k], right[k], up_[k], forward[k]
    c.fov = fov
    return c


def copy_camera(cam: abi.Camera) -> abi.Camera:
    c = abi.Camera()
    C.memmove(C.byref(c), C.byref(cam), C.sizeof(abi.Camera))
    return c


def cameras(origin=(0.0, 3.0, -9.0)) -> dict:
    """name -> (camera, every lane inside?, some lane inside?): looking down +z from `origin`, fov 1.
    `thin`: right = (2^-58 / aspect, 0, 0) for the widths 8 and 16, so |d_x| = 2^-58 |2 (px + 0.5) / W - 1|
    is below 2^-60 in the columns nearest the centre only; `small` / `huge`: the three axes times 2^-50 /
    2^61, so s lies below 2^-96 / above 2^120 in every pixel."""
    X, Y, Z = (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)
    sc = lambda v, k: tuple(float(F32(a) * F32(k)) for a in v)   # noqa: E731
    return {
        "plain": (_camera(origin, X, Y, Z, 1.0), True, True),
        "thin8": (_camera(origin, sc(X, P2(-58)), Y, Z, 1.0), False, True),       # aspect 1
        "thin16": (_camera(origin, sc(X, P2(-59)), Y, Z, 1.0), False, True),      # aspect 2
        "small": (_camera(origin, sc(X, P2(-50)), sc(Y, P2(-50)), sc(Z, P2(-50)), 1.0), False, False),
        "huge": (_camera(origin, sc(X, P2(61)), sc(Y, P2(61)), sc(Z, P2(61)), 1.0), False, False),
    }


def primary_l(cam: abi.Camera, W: int, H: int) -> np.ndarray:
    """The primary ray's direction before the normalisation per pixel (row-major), in binary32 in the
    reference's order (Renderer.cpp:104-114, Matrix::TransformVector)."""
    px, py = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    fW, fH, two, one, half = F32(W), F32(H), F32(2), F32(1), F32(0.5)
    aspect = F32(fW / fH)
    fov = F32(cam.fov)
    with np.errstate(all="ignore"):
        cx = ((two * ((px + half) / fW).astype(np.float32) - one).astype(np.float32) * aspect).astype(np.float32) * fov
        cy = (one - ((two * (py + half)).astype(np.float32) / fH).astype(np.float32)).astype(np.float32) * fov
        out = []
        for k in range(3):
            r, u, f = F32(cam.right[k]), F32(cam.up[k]), F32(cam.forward[k])
            out.append((((r * cx).astype(np.float32) + (u * cy).astype(np.float32)).astype(np.float32) + f * one).astype(np.float32))
    return np.stack([o.ravel() for o in out], 1)


def wave_lanes(W: int, H: int) -> np.ndarray:
    """(waves, 64) pixel indices of the frame's 8 x 8 wave tiles, lanes row-major (px = lane & 7)."""
    idx = np.arange(W * H).reshape(H, W)
    return np.array([idx[y:y + 8, x:x + 8].ravel() for y in range(0, H, 8) for x in range(0, W, 8)])


# ------------------------------------------------------------------------- the room with one triangle

ROOM = ["plane 0 0 10   0 0 -1  1", "plane 0 0 0    0 1 0   1", "plane 0 10 0   0 -1 0  1",
        "plane 5 0 0   -1 0 0   1", "plane -5 0 0   1 0 0   1"]
ROOM_LIGHTS = ["light point 0 5 5  50 1 0.61 0.45", "light point -2.5 5 -5  70 1 0.8 0.45", "light point 3 2 2  30 0.6 0.8 1"]
ROOM_MATS = {"lambert": ["material lambert 0.49 0.57 0.57 1", "material lambert 1 1 1 1"],
             "mixed": ["material lambert 0.49 0.57 0.57 1", "material cook_torrance 0.75 0.75 0.75 0 0.6"]}
# camera name -> (origin, fov degrees, pitch, yaw) for HostScene.set_camera: the triangle in a part of the
# view, filling it, and behind the camera
ROOM_CAMERAS = {"mix": ((0.0, 3.0, -9.0), 45.0, 0.0, 0.0), "tri": ((0.0, 3.0, 3.0), 20.0, 0.0, 0.0),
                "planes": ((0.0, 3.0, 6.0), 45.0, 0.0, 0.0)}


def room_scene(folder, kind: str, lights=None):
    """HostScene of the five-plane room with one triangle (material 2, back-face culled, facing -z at
    z = 5) and three point lights; kind: `lambert` (the Lambert-only kernel variant) or `mixed` (Lambert
    walls, a Cook-Torrance triangle)."""
    from gp1_raytracer_2223_amd.scene import HostScene
    d = Path(folder) / f"room_{kind}"
    d.mkdir(parents=True, exist_ok=True)
    verts = np.array([(-3, 0.5, 5), (0, 6.5, 5), (3, 0.5, 5)], np.float32)
    (d / "fp_tri.obj").write_text(mesh_fuzz.obj_text(verts, [(0, 1, 2)]))
    path = d / f"room_{kind}.rtxscene"
    path.write_text("\n".join(["camera 0 3 -9 45", *ROOM_MATS[kind], *ROOM, "mesh fp_tri 2 back",
                               *(ROOM_LIGHTS if lights is None else lights)]) + "\n")
    return HostScene(f"file:{path}", asset_dir=str(path.parent))
