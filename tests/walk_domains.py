"""Rays, scenes and a model of the per-wave walk choice at the edges of the ray kernels' fast-path
domains — TEST INFRASTRUCTURE (tests/test_walk_domains_cpu.py, tests/test_gpu_walk_domains.py,
tests/golden/make_goldens.py).

DESIGN.md, *Fast-path domains* (1)-(5), names the operand bounds inside which a wave of the ray kernels
takes a shortcut: every |d_k| in [2^-60, 2^60] (tested as min |d_k| >= 2^-60 and the binary32 sum of the
magnitudes <= 2^60), a finite origin, |d_k| <= 1 and |o_k| <= 2^40 on a scene with |e1||e2| <= 2^56 for
the reduced triangle test, |a| > 2^60 for the IEEE reciprocal of the full one, and tmin > 0 with a
finite tmax for the any-hit plane shortcut.  This module builds, for every bound, seeded rays exactly
at it and one float past it, on scenes whose triangles sit exactly at the |e1||e2| bound and one float
past it, in waves that are wholly inside, wholly outside, and inside but for one lane; and `walk_of`
restates the choice in numpy, from the text of DESIGN.md, so that the tests can prove which walk each
wave is meant to take.

Scenes: twelve right triangles (0, 0, z), (0, b, z), (a, 0, z) stacked in z (normal -z, towards the
file's camera), one Lambert material, one plane x = const beside the stack that only a ray travelling in -x can
reach (far beyond the triangles), a point light and a directional light.  No powf anywhere: every
comparison is word for word.  A fifth scene, `needle` (below), has thin triangles 2^90 away: the bound on
v0 that tri_fast needs beside the one on |e1||e2|."""
from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path

import numpy as np

import mesh_fuzz
from scene_fuzz import fmt

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
INF = F32(np.inf)
N_TRI = 12


def up(x) -> np.float32:
    """One binary32 above x."""
    return np.nextafter(F32(x), INF)


@dataclass(frozen=True)
class Geo:
    """A scene's geometry and the scales its rays are built with."""
    name: str
    a: float            # leg along x
    b: float            # leg along y
    dz: float           # spacing of the stack
    xcap: float         # targets have x <= 0.45 min(a, xcap)
    back: float         # an ordinary ray starts `back` .. 6 `back` from its target
    rho: tuple          # lateral offsets (x, y) of the rays built along the z axis
    plane_x: float      # the plane x = plane_x, normal +x, beside the stack
    camera: tuple       # the file's camera (it looks down +z)
    point: tuple        # point light: x, y, z, intensity
    direct: tuple       # directional light: dx, dy, dz, intensity
    fov: float = 45.0   # the camera's, degrees

    @property
    def tri_fast(self) -> bool:
        return float(F32(self.a)) * float(F32(self.b)) <= 2.0 ** 56


_G28 = 2.0 ** 28
# The file's camera stands between the fourth and the fifth triangle (2^20 before the fifth on the large
# scenes), looks down +z and sees the fifth's hypotenuse: some pixels hit it, the others pass every
# triangle.  The point light lies below the stack, past the hypotenuse: a shadow ray leaves the stack's
# footprint before or after it crosses the fourth triangle, depending on the pixel.
_BIG_CAMERA = (2.0 ** 27, 2.0 ** 27 - 2.0 ** 18, 2.0 ** 24 - 2.0 ** 20)
_BIG_LIGHT = (2.0 ** 27 + 2.0 ** 21, 2.0 ** 27 + 2.0 ** 21, -2.0 ** 26, 2.0 ** 53)
_DIRECT = (0.25, 0.5, -1.0, 1.0)
GEO = {
    "unit": Geo("unit", 4.0, 4.0, 0.5, 4.0, 1.0, (1.0, 1.0), -8.0, (2.0, 1.9, 1.75), (2.3, 2.3, -6.0, 60.0), _DIRECT),
    "giant": Geo("giant", _G28, _G28, 2.0 ** 22, _G28, 2.0 ** 22, (2.0 ** 26, 2.0 ** 26), -2.0 ** 30, _BIG_CAMERA,
                 _BIG_LIGHT, _DIRECT),
    "over": Geo("over", _G28, float(up(_G28)), 2.0 ** 22, _G28, 2.0 ** 22, (2.0 ** 26, 2.0 ** 26), -2.0 ** 30,
                _BIG_CAMERA, _BIG_LIGHT, _DIRECT),
    "sliver": Geo("sliver", 2.0 ** 55, 2.0, 0.25, 2.0 ** 38, 1.0, (2.0 ** 30, 0.25), -8.0, (2.0 ** 36, 1.97, 0.875),
                  (2.0 ** 36, 2.2, -0.5, 2.0), _DIRECT),
}
CULLS = ("none", "back")
SCENES = tuple((g, c) for g in GEO for c in CULLS)


def scene_texts(geo: Geo, cull: str):
    """(OBJ stem, OBJ text, scene text) of a scene: every float through scene_fuzz.fmt, so that strtof
    reads the same binary32 on every side."""
    verts, faces = [], []
    for k in range(N_TRI):
        z = geo.dz * k
        verts += [(0.0, 0.0, z), (0.0, geo.b, z), (geo.a, 0.0, z)]
        faces.append((3 * k, 3 * k + 1, 3 * k + 2))
    stem = f"wd_{geo.name}"
    rows = [f"# walk_domains {geo.name} {cull}",
            " ".join(["camera"] + [fmt(x) for x in (*geo.camera, geo.fov)]),
            "material lambert 0.9 0.75 0.49 1",
            " ".join(["plane", fmt(geo.plane_x), "0", "0", "1", "0", "0", "1"]),
            f"mesh {stem} 1 {cull}",
            " ".join(["light", "point"] + [fmt(x) for x in geo.point] + ["1", "0.9", "0.75"]),
            " ".join(["light", "directional"] + [fmt(x) for x in geo.direct] + ["0.5", "0.75", "1"])]
    return stem, mesh_fuzz.obj_text(np.array(verts, np.float32), faces), "\n".join(rows) + "\n"


def write_scene(geo: Geo, cull: str, folder) -> Path:
    """Write the OBJ and the scene file into `folder`/<name>_<cull>; returns the scene file's path (its
    folder is the asset folder)."""
    d = Path(folder) / f"{geo.name}_{cull}"
    d.mkdir(parents=True, exist_ok=True)
    stem, obj, text = scene_texts(geo, cull)
    (d / f"{stem}.obj").write_text(obj)
    path = d / f"wd_{geo.name}_{cull}.rtxscene"
    path.write_text(text)
    return path


def host_scene(geo: Geo, cull: str, folder):
    """(HostScene, rtx_scene, camera); keep the first alive while the others are in use."""
    from gp1_raytracer_2223_amd.scene import HostScene
    path = write_scene(geo, cull, folder)
    hs = HostScene(f"file:{path}", asset_dir=str(path.parent))
    return (hs, *hs.view())


# ---------------------------------------------------------------------------------------------------- rays

def _rows(o, d, tmin, tmax):
    n = o.shape[0]
    r = np.zeros((n, 8), np.float32)
    with np.errstate(over="ignore"):
        r[:, 0:3], r[:, 3:6] = o, d
    r[:, 6], r[:, 7] = tmin, tmax
    return r


MISS = 0.45      # the share of rays aimed past the hypotenuse: inside the boxes, outside every triangle


def _targets(rng, geo: Geo, n):
    """Points in the planes of random triangles of the stack: well inside the triangle (x / a + y / b <=
    0.9), or for a share of MISS well past its hypotenuse (on the sliver: past its short leg)."""
    k = rng.integers(0, N_TRI, n)
    miss = rng.uniform(0.0, 1.0, n) < MISS
    x = rng.uniform(0.05, 0.45, n) * min(geo.a, geo.xcap)
    y = np.where(miss, rng.uniform(1.1, 3.0, n), rng.uniform(0.05, 0.45, n)) * geo.b
    return np.stack([x, y, geo.dz * k], 1)


def _signs(rng, n, octant):
    """Direction signs: octant None = random per ray (two in three travel up, against the triangles'
    normals: the rays a back-culling mesh keeps in closest hit), else bit a set = negative on axis a."""
    if octant is None:
        sg = rng.choice(np.array([-1.0, 1.0]), size=(n, 3))
        sg[:, 2] = np.where(rng.uniform(0.0, 1.0, n) < 2.0 / 3.0, 1.0, -1.0)
        return sg
    return np.tile(np.array([[-1.0 if (octant >> a) & 1 else 1.0 for a in range(3)]]), (n, 1))


def _mags(rng, n):
    """Direction magnitudes: every component in [0.05, 0.9], z at least 0.4 (no grazing ray: the
    reference refuses |n . d| and |a| below FLT_EPSILON)."""
    m = rng.uniform(0.05, 0.6, (n, 3))
    m[:, 2] = rng.uniform(0.4, 0.9, n)
    return m


def plain(rng, geo: Geo, n, octant=None, tmin=1e-4, tmax=FLT_MAX):
    """Ordinary rays into the triangles, inside every domain."""
    p, d = _targets(rng, geo, n), _mags(rng, n) * _signs(rng, n, octant)
    s = rng.uniform(1.0, 6.0, (n, 1)) * geo.back
    return _rows(p - s * d, d, tmin, tmax)


def _scaled(rng, geo, n, octant, scale, tmin):
    """`plain` with the direction times a power of two (the origin stays, t shrinks by it)."""
    r = plain(rng, geo, n, octant, tmin)
    with np.errstate(over="ignore"):
        r[:, 3:6] = r[:, 3:6] * F32(scale)
    return r


def dmax(rng, geo, n, octant=None, outside=False):
    """max |d_k| = 1 exactly, or one float above."""
    p, m = _targets(rng, geo, n), _mags(rng, n)
    m = m / m.max(axis=1, keepdims=True)
    d = (m * _signs(rng, n, octant)).astype(np.float32)
    top = np.abs(d).argmax(axis=1)
    rows = np.arange(n)
    d[rows, top] = np.sign(d[rows, top]) * (up(1.0) if outside else F32(1.0))
    s = rng.uniform(1.0, 6.0, (n, 1)) * geo.back
    return _rows(p - s * d.astype(np.float64), d, 1e-4, FLT_MAX)


def dsum(rng, geo, n, octant=None, outside=False):
    """|d| = (2^59, small, 2^59): the binary32 sum of the magnitudes is 2^60 exactly; outside, x is
    2^59 + 2^37 and the sum one float above 2^60.  t is tiny, so tmin = 0."""
    p = _targets(rng, geo, n)
    m = np.stack([np.full(n, 2.0 ** 59 + (2.0 ** 37 if outside else 0.0)), rng.uniform(1.0, 16.0, n) * 2.0 ** 30,
                  np.full(n, 2.0 ** 59)], 1)
    d = m * _signs(rng, n, octant)
    s = rng.uniform(1.0, 6.0, (n, 1)) * geo.back * 2.0 ** -59.5
    return _rows(p - s * d, d, 0.0, FLT_MAX)


def dsingle(rng, geo, n, octant=None, outside=False):
    """d_z = 2^60; inside, x and y are below 2^34 and the sum rounds to 2^60; outside, they are of
    its size (each still <= 2^60) and the sum is beyond."""
    p = _targets(rng, geo, n)
    xy = rng.uniform(0.05, 0.6, (n, 2)) * (2.0 ** 60 if outside else 2.0 ** 34)
    d = np.concatenate([xy, np.full((n, 1), 2.0 ** 60)], 1) * _signs(rng, n, octant)
    s = rng.uniform(1.0, 6.0, (n, 1)) * geo.back * 2.0 ** -60
    return _rows(p - s * d, d, 0.0, FLT_MAX)


def dmin(rng, geo, n, octant=None, outside=False):
    """min |d_k| = 2^-60 (x or y in turn), or 2^-61."""
    p, d = _targets(rng, geo, n), _mags(rng, n) * _signs(rng, n, octant)
    ax = np.arange(n) & 1
    rows = np.arange(n)
    d[rows, ax] = np.sign(d[rows, ax]) * (2.0 ** -61 if outside else 2.0 ** -60)
    s = rng.uniform(1.0, 6.0, (n, 1)) * geo.back
    return _rows(p - s * d, d, 1e-4, FLT_MAX)


def along_z(rng, geo, n, dist, octant=None, down=None, tmin=1e-4, tmax=FLT_MAX):
    """Rays that start at z = +-dist exactly (dist a binary32, the largest origin magnitude) beside the
    stack's axis and are aimed into a triangle: d_z = -+1 up to rounding, |d_x|, |d_y| = offset / dist.
    down: per ray, whether it starts above the stack and travels down (None = as the octant says, or
    random)."""
    p = _targets(rng, geo, n)
    sg = _signs(rng, n, octant)
    if down is not None:
        sg[:, 2] = np.where(down, -1.0, 1.0)
    off = rng.uniform(0.1, 1.0, (n, 2)) * np.array(geo.rho) * sg[:, 0:2]
    o = np.concatenate([p[:, 0:2] - off, (-sg[:, 2:3]) * float(dist)], 1)
    o32 = o.astype(np.float32).astype(np.float64)
    d = (p - o32) / np.abs(p[:, 2:3] - o32[:, 2:3])
    return _rows(o32, d, tmin, tmax)


def far(rng, geo, n, octant=None):
    """The NaN-occluder class: origins 2^70, 2^100, 2^120 and 2^100 away in turn, tmax finite (twice the
    distance).  Three in four start below the stack and travel up, where the plane cannot be hit: on
    the large scenes `s x e1` overflows for the two larger distances, Vector3::Cross's `0 *` terms make
    every component NaN, no comparison rejects the NaN t and DoesHit reports an occluder that
    GetClosestHit cannot keep."""
    out = np.zeros((n, 8), np.float32)
    for k, e in enumerate((70, 100, 120, 100)):
        idx = np.arange(k, n, 4)
        down = (np.arange(idx.size) & 3) == 3
        out[idx] = along_z(rng, geo, idx.size, 2.0 ** e, octant, down, 1e-4, 2.0 ** (e + 1))
    return out


def big_a(rng, geo, n, octant=None):
    """Directions times 2^6, 2^30, 2^58 (the fast slab still holds), 2^66, 2^71 and 2^74 in turn: on the
    2^56 scenes |a| = |d_z| a b lies in (2^60, 2^126], in (2^126, FLT_MAX] (a denormal 1 / a) and
    overflows to inf.  t shrinks with the scale: tmin is 0 and, in turn, negative (as far behind the
    origin as the nearest an ordinary ray starts from its target)."""
    out = np.zeros((n, 8), np.float32)
    for k, e in enumerate((6, 30, 58, 66, 71, 74)):
        idx = np.arange(k, n, 6)
        out[idx] = _scaled(rng, geo, idx.size, octant, 2.0 ** e, 0.0)
        out[idx[1::2], 6] = -geo.back * 2.0 ** -e
    return out


PLANE_FORMS = tuple((tmin, fin) for tmin in (0.0, -1.0, 1e-4) for fin in (True, False))


def plane_rays(rng, geo, n, octant=None, outside=False):
    """Ordinary rays with tmin in {0, -1, 1e-4} x tmax in {a few times the distance to the target, inf}.
    Inside: tmin = 1e-4 and the finite tmax only.  The direction's z sign puts the plane in front of the
    ray or behind it."""
    r = plain(rng, geo, n, octant)
    reach = rng.uniform(0.5, 8.0, n) * 6.0 * geo.back
    forms = [f for f in PLANE_FORMS if f != (1e-4, True)] if outside else [(1e-4, True)]
    for i in range(n):
        tmin, fin = forms[i % len(forms)]
        r[i, 6], r[i, 7] = tmin, (reach[i] if fin else INF)
    return r


def _twin(fn):
    return (lambda rng, geo, n, o=None: fn(rng, geo, n, o, False)), (lambda rng, geo, n, o=None: fn(rng, geo, n, o, True))


def _omax(rng, geo, n, o=None, outside=False):
    return along_z(rng, geo, n, up(2.0 ** 40) if outside else F32(2.0 ** 40), o)


def onto_plane(rng, geo, n, octant=None, outside=False):
    """Rays travelling in -x onto the plane beside the stack, 2^20 from it.  The hit point's larger
    coordinate of y and z has the magnitude 2^40 (1 - 2^-20), or 2^40 (1 + 2^-20): the origins of the
    shadow rays lie on either side of the 2^40 bound (and so do these rays' own).  Half of the hit points
    lie at -y, +z, from where the way to the point light crosses the stack; the others see it freely."""
    big = 2.0 ** 40 * (1 + 2.0 ** -20 if outside else 1 - 2.0 ** -20)
    sg = _signs(rng, n, octant)[:, 1:3]
    if octant is None:
        sg[::2] = (-1.0, 1.0)
    yz = rng.uniform(0.3, 1.0, (n, 2))
    top = rng.integers(0, 2, n)
    yz[np.arange(n), top] = 1.0
    o = np.concatenate([np.full((n, 1), geo.plane_x + 2.0 ** 20), yz * sg * big], 1)
    d = np.concatenate([np.full((n, 1), -1.0), rng.uniform(1.0, 2.0, (n, 2)) * 2.0 ** -30 * sg], 1)
    return _rows(o, d, 1e-4, FLT_MAX)


# class -> (inside generator, outside generator): both sides of one threshold.  `far` and `big_a` have
# ordinary rays as their inside.
CLASSES = {
    "dmax": _twin(dmax), "dsum": _twin(dsum), "dsingle": _twin(dsingle), "dmin": _twin(dmin), "omax": _twin(_omax),
    "far": (plain, far), "big_a": (plain, big_a), "plane": _twin(plane_rays),
}
SHADE_CLASSES = {"onto_plane": _twin(onto_plane)}     # for the shaded rays: not aimed at the triangles
_ALL = {**CLASSES, **SHADE_CLASSES}
# The scenes a class is for.  The classes of the triangle domain (3) need a tri_fast scene for their inside
# to be fast at all; the NaN occluder needs `s x e1` to overflow, which the 2^28 legs do.  Every class
# still runs on every scene.
INTENDED = {"dmax": ("unit", "giant", "sliver"), "dsum": tuple(GEO), "dsingle": tuple(GEO), "dmin": tuple(GEO),
            "omax": ("unit", "giant", "sliver"), "far": ("giant",), "big_a": ("unit", "giant", "sliver"),
            "plane": tuple(GEO)}
MIXED_LANES = (0, 17, 63)
LAYOUT = ("in", "out") + tuple(f"lane{k}" for k in MIXED_LANES)     # the waves of `waves`, in order


def waves(geo: Geo, cls: str, seed: int = 1) -> np.ndarray:
    """Five waves of a class: all inside (one octant), all outside, and 63 inside rays with one outside
    ray at lane 0, 17 and 63."""
    inside, outside = _ALL[cls]
    rng = np.random.default_rng((2223, sorted(GEO).index(geo.name), sorted(_ALL).index(cls), seed))
    octant = (3 * sorted(_ALL).index(cls) + 1) & 7
    blocks = [inside(rng, geo, 64, octant), outside(rng, geo, 64, None)]
    odd = outside(rng, geo, 6, None)
    for j, lane in enumerate(MIXED_LANES):
        b = inside(rng, geo, 64, octant if j == 1 else None)
        b[lane] = odd[1 + j]
        blocks.append(b)
    return np.concatenate(blocks)


def tail(geo: Geo, cls: str, seed: int = 2) -> np.ndarray:
    """130 inside rays whose only outside rays are rays 63 and 64: a prefix of 63 leaves the first in an
    inactive tail lane, a prefix of 64 the second in a wave that is not launched."""
    inside, outside = _ALL[cls]
    rng = np.random.default_rng((2223, sorted(GEO).index(geo.name), sorted(_ALL).index(cls), seed))
    r = inside(rng, geo, 130, None)
    r[63:65] = outside(rng, geo, 8, None)[2:4]
    return r


def outside_of(cls: str):
    """(indices into `waves`, indices into `tail`) of the outside rays."""
    return np.concatenate([np.arange(64, 128), [128 + 64 * j + lane for j, lane in enumerate(MIXED_LANES)]]), np.array([63, 64])


def all_sets(geo: Geo) -> dict:
    """{set name: rays} of a scene: `waves` and `tail` of every class."""
    out = {}
    for cls in CLASSES:
        out[f"{cls}/waves"] = waves(geo, cls)
        out[f"{cls}/tail"] = tail(geo, cls)
    return out


# ------------------------------------------------------------- thin triangles far away: beyond the bound on v0

# Twelve triangles (0, y, Z), (a, y, Z), (0, y + b, Z) with a b = 2^56 exactly, 2^30 apart in y, in the plane
# z = Z = 2^90.  |e1||e2| is at its bound, but for any origin `(o - v0) x e1` has the term Z a = 2^130: it
# overflows, Vector3::Cross's `0 *` terms make every component NaN, and DoesHit accepts the triangle for
# every ray that crosses the plane z = Z between x = 0 and x = a, while the reduced cross products keep an
# infinite component that rejects it.  The packer therefore refuses tri_fast to a scene whose
# (|v0|_1 + 2^40) (|e1|_1 + |e2|_1) exceeds 2^126, and rays inside every ray domain take the cross
# products as written on it.
NEEDLE_A, NEEDLE_B, NEEDLE_Z, NEEDLE_DY = 2.0 ** 40, 2.0 ** 16, 2.0 ** 90, 2.0 ** 30
NEEDLE_FACTS = {"tri_fast": False, "oct": True}


def needle_texts(cull: str, frame: bool = False):
    """(OBJ stem, OBJ text, scene text) of the `needle` scene.  frame: the variant a frame shows the
    overflow in: a plane z = 5 before the file's camera, a point light 2^60 beyond it (a shadow ray of
    that length still has a direction) whose shadow rays cross z = 2^90 between x = 0 and x = 2^40 for
    about a quarter of the pixels, where DoesHit accepts the NaN t although the triangle lies beyond the
    light; and a near point light that varies the colour."""
    verts, faces = [], []
    for k in range(N_TRI):
        y = NEEDLE_DY * k
        verts += [(0.0, y, NEEDLE_Z), (NEEDLE_A, y, NEEDLE_Z), (0.0, y + NEEDLE_B, NEEDLE_Z)]
        faces.append((3 * k, 3 * k + 1, 3 * k + 2))
    rows = [f"# walk_domains needle {cull}", "camera 0 0 0 45", "material lambert 0.9 0.75 0.49 1",
            f"mesh wd_needle 1 {cull}", "light point 0 0 -10 1 1 0.9 0.75", "light directional 0.25 0.5 -1 1 0.5 0.75 1"]
    if frame:
        rows = rows[:3] + ["plane 0 0 5 0 0 1 1", rows[3], " ".join(["light point 8 8", fmt(2.0 ** 60), "1e36 1 0.9 0.75"]),
                           "light point 3 4 9 20 0.5 0.75 1"]
    return "wd_needle", mesh_fuzz.obj_text(np.array(verts, np.float32), faces), "\n".join(rows) + "\n"


def write_needle(cull: str, folder, frame: bool = False) -> Path:
    d = Path(folder) / (f"needle_{cull}" + ("_frame" if frame else ""))
    d.mkdir(parents=True, exist_ok=True)
    stem, obj, text = needle_texts(cull, frame)
    (d / f"{stem}.obj").write_text(obj)
    path = d / f"wd_needle_{cull}.rtxscene"
    path.write_text(text)
    return path


def needle_scene(cull: str, folder, frame: bool = False):
    """(HostScene, rtx_scene, camera) of the `needle` scene, or of its frame variant."""
    from gp1_raytracer_2223_amd.scene import HostScene
    path = write_needle(cull, folder, frame)
    hs = HostScene(f"file:{path}", asset_dir=str(path.parent))
    return (hs, *hs.view())


def needle_rays(seed: int = 3, n: int = 320) -> np.ndarray:
    """Rays inside every ray domain (|o_k| <= 2^39, max |d_k| = 1, no component below 2^-60) aimed at
    the plane z = Z, four in five between x = 0 and x = a; the first wave in one octant."""
    rng = np.random.default_rng((2223, 99, seed))
    x = np.where(rng.uniform(0, 1, n) < 0.8, rng.uniform(0.1, 0.9, n), rng.uniform(1.5, 3.0, n)) * NEEDLE_A
    p = np.stack([x, rng.uniform(0.0, N_TRI - 1, n) * NEEDLE_DY, np.full(n, NEEDLE_Z)], 1)
    o = rng.uniform(-1.0, 1.0, (n, 3)) * 2.0 ** 39
    o[:64, 0:2] = -np.abs(o[:64, 0:2])
    d = p - o
    d /= np.abs(d).max(axis=1, keepdims=True)
    return _rows(o, d, 1e-4, FLT_MAX)


# ------------------------------------------------------------------------------ rows for the primitive pins

PRIM_ROW = 34       # ray 8, triangle v0 v1 v2 9, cull mode 1, box 6, plane 6, sphere 4
PRIM_RAYS = 5       # inside and outside rays of every class on every scene (24 outside rays of `far`)


def _nearest_triangle(geo: Geo, ray) -> int:
    """The triangle of the stack the ray's line passes through (the first found), else the one whose plane
    it meets nearest its origin; in double."""
    o, d = ray[0:3].astype(np.float64), ray[3:6].astype(np.float64)
    best, best_t = 0, np.inf
    for k in range(N_TRI):
        if d[2] == 0 or not np.isfinite(d[2]):
            break
        t = (geo.dz * k - o[2]) / d[2]
        x, y = o[0] + t * d[0], o[1] + t * d[1]
        if x >= 0 and y >= 0 and x / geo.a + y / geo.b <= 1:
            return k
        if abs(t) < best_t:
            best, best_t = k, abs(t)
    return best


def prim_rows() -> np.ndarray:
    """(n, PRIM_ROW) float32: rays of every class (SHADE_CLASSES too), inside and outside, on every scene,
    each with the triangle of the stack it is aimed at (cull modes 0, 1, 2 in turn), that triangle's box
    or the stack's, the scene's plane or the triangle's, and a sphere around the triangle's middle: the
    operands of tests/golden/prims_domains.npz, on which the reference's own HitTest_* and SlabTest_BVH
    pin the oracle's."""
    rows = []
    for name, geo in GEO.items():
        for cls in _ALL:
            w = waves(geo, cls)
            picks = np.concatenate([w[:PRIM_RAYS], w[64:64 + (24 if cls == "far" else PRIM_RAYS)]])
            for ray in picks:
                i = len(rows)
                k = _nearest_triangle(geo, ray)
                z = geo.dz * k
                tri = [0.0, 0.0, z, 0.0, geo.b, z, geo.a, 0.0, z]
                box = [0.0, 0.0, z, geo.a, geo.b, z] if i & 1 else [0.0, 0.0, 0.0, geo.a, geo.b, geo.dz * (N_TRI - 1)]
                plane = [geo.plane_x, 0.0, 0.0, 1.0, 0.0, 0.0] if i & 2 else [0.0, 0.0, z, 0.0, 0.0, -1.0]
                sphere = [min(geo.a, geo.xcap) / 4, geo.b / 4, z, min(geo.a, geo.xcap, geo.b) / 4]
                rows.append(np.array([*ray, *tri, float(i % 3), *box, *plane, *sphere], np.float32))
    return np.array(rows, np.float32)


# --------------------------------------------------------------------------------------------------- model

def facts(geo: Geo) -> dict:
    """What the packer derives from a scene and the chooser reads: tri_fast, and that the node array
    has octant copies (tests/test_walk_domains_cpu.py holds the packer to both)."""
    return {"tri_fast": geo.tri_fast, "oct": True}


def lane_facts(rays: np.ndarray) -> dict:
    """Per ray, the domain tests of DESIGN.md (1)-(5) in binary32."""
    r = np.ascontiguousarray(rays, np.float32)
    o, d = r[:, 0:3], r[:, 3:6]
    ad = np.abs(d)
    with np.errstate(all="ignore"):
        s = (ad[:, 0] + ad[:, 1]).astype(np.float32) + ad[:, 2]      # binary32, in this order
        lo = np.where(np.isnan(ad).any(axis=1), F32(np.nan), ad.min(axis=1))
        rcp_dom = (lo >= F32(2.0 ** -60)) & (s.astype(np.float32) <= F32(2.0 ** 60))          # (1); NaN fails
        slow = ~rcp_dom | ~np.isfinite(o).all(axis=1)                                       # (2)
        tri_dom = (ad.max(axis=1) <= 1) & (np.abs(o).max(axis=1) <= F32(2.0 ** 40))           # (3)
        plane_dom = (r[:, 6] > 0) & (np.abs(r[:, 7]) < INF)                                 # (5)
    octant = (np.signbit(d[:, 0]).astype(int) | (np.signbit(d[:, 1]).astype(int) << 1) |
              (np.signbit(d[:, 2]).astype(int) << 2))
    return {"slow": slow, "tri_dom": tri_dom & ~slow, "plane_dom": plane_dom, "octant": octant}


WALKS = ("octant", "fast", "xc", "exact")


def walk_of(scene_facts: dict, rays: np.ndarray, active=None):
    """[(walk, plane form)] per wave of 64 rays: the walk is `octant`, `fast`, `xc` (the fast slab with
    Vector3::Cross as written and the |a| check) or `exact`; the plane form `cand` (the shortcut) or
    `divide`.  active: bool per ray (default: all); a wave without an active lane is skipped.  A wave
    takes a shortcut when every ACTIVE lane is inside its domain."""
    n = rays.shape[0]
    act = np.ones(n, bool) if active is None else np.asarray(active, bool)
    f = lane_facts(rays)
    out = []
    for w0 in range(0, n, 64):
        a = act[w0:w0 + 64]
        if not a.any():
            continue
        sl = slice(w0, w0 + 64)
        slab_fast = not f["slow"][sl][a].any()
        fast = slab_fast and scene_facts["tri_fast"] and f["tri_dom"][sl][a].all()
        same = len(set(f["octant"][sl][a].tolist())) == 1
        walk = ("octant" if scene_facts["oct"] and same else "fast") if fast else ("xc" if slab_fast else "exact")
        out.append((walk, "cand" if f["plane_dom"][sl][a].all() else "divide"))
    return out


def shadow_rays(scene, rays: np.ndarray, planes: dict, light: int):
    """(rays, hit): the shadow ray Ray{hit + normal * 0.0001, l / |l|, 0.0001, |l|} towards `light` of
    every ray from the checker's hit record, in binary32 as the renderer computes it, and which rays
    hit (the shadow ray's active lanes)."""
    r = np.ascontiguousarray(rays, np.float32)
    n = r.shape[0]
    hit = (np.asarray(planes["primitive"]) >> 30) != 0
    with np.errstate(all="ignore"):
        t = planes["depth"].astype(np.float32)[:, None]
        h = r[:, 0:3] + (r[:, 3:6] * t).astype(np.float32)
        oo = h + (planes["normal"].reshape(n, 3) * F32(0.0001)).astype(np.float32)
        l = np.array(scene.lights[light].origin[:], np.float32)[None, :] - oo
        mag = np.sqrt(((l[:, 0] * l[:, 0]).astype(np.float32) + l[:, 1] * l[:, 1]).astype(np.float32) + l[:, 2] * l[:, 2])
        l = (l / mag[:, None]).astype(np.float32)
    return _rows(oo, l, 1e-4, mag.astype(np.float32)), hit
