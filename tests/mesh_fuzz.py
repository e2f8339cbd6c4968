"""Seeded adversarial MESHES for the animated BVH rebuild — TEST INFRASTRUCTURE
(tests/test_mesh_fuzz_golden.py, tests/test_gpu_anim_fuzz.py, golden/make_mesh_goldens.py,
tools/anim_stress.py).

tests/scene_fuzz.py varies everything around the bundled meshes; this varies the mesh data, aimed
at the corners of the reference's TriangleMesh::BuildBVH / Subdivide / FindBestSplitPlane that the
bundled meshes never reach (DESIGN.md §7a has the table).  `make(family, seed)` returns the OBJ
text(s), the scene text and the Update times of one case.  The OBJ is `v x y z` / `f a b c`
(1-based); every float is printed with scene_fuzz.fmt, so strtof reads the same binary32 on every
side.  The scene is one Lambert material, a floor plane, a point light and the spinning mesh(es):
no powf anywhere, so frames are bit-exact.  No position is NaN (rtx_anim_create refuses those) and
no degenerate triangle appears (its normal would be NaN).

Every Update list starts with 3.1415927: cosf gives exactly -1 there, the yaw is 0 and the rotation
is the identity, so axis-aligned ties and flat axes survive into the first rebuild.  Four more
times follow: each rebuild permutes the triangles in place and the next one starts from that order.

Families (the seed picks the variant, modulo their number, and seeds the random numbers):
  tiny        T = 1, 2, 3, 4, 9 (seeds 0-4): the `idxCount <= 8` threshold counts indices
  negative    random soup translated so that every centroid is negative on all three axes: the
              centroid maximum starts at FLT_MIN, the bin scale is wrong and almost nothing splits.
              Seeds 0, 2: T = 200 and 3,300, wide enough on x and z to reach a second bin (a few
              nodes, a leaf of thousands); seeds 1, 3: T = 233 and 3,200, compact (the root is the
              only leaf).  Seed 4: negative on y only, eight thin slabs of 128 triangles that the
              x axis separates (128 is the most a one-wave node of the device builder holds)
  negative_x  the same on one axis only (seed 0: x, seed 1: z)
  dup         one triangle many times plus a few others.  Seed 0: 5,000 copies and 2 others (all
              axes skipped below the root: a leaf above every LDS capacity); seed 1: 40 copies
              among 20 others
  flat_grid   an 8 x 8 integer grid in a y = const plane (seed 0 centred, seed 1 with a corner at the
              origin, seed 2 away from it): a skipped axis and exact SAH ties between planes and
              between x and z
  dup_grid    a bumpy grid with every face twice (seed 0) or twelve times (seed 1), off-centre:
              ties inside leaves, medium leaves
  epsilon     the centroid spread of one axis is non-zero but below FLT_EPSILON at yaw 0
              (seed 0: y, which the spin keeps; seed 1: x, which the spin widens)
  overflow    soup scaled by 1e19: node areas overflow to inf, `splitCost >= noSplitCost` is false
              and the partition runs on axis 0 at the zero-initialised splitPos
  geometric   triangles shrinking geometrically towards the origin: skewed bins, a large leaf beside
              single triangles (seed 0: 120 triangles, ratio 0.5; seed 1: 600, ratio 0.9)
  caps        centred soup of T = 3,136, 3,137, 4,096, 4,097 (seeds 0-3): the device builder's LDS
              capacity and its frontier histogram's, exactly at and one past
  mixed       seven of the above spinning in one scene (one above 3,136 triangles, one `tiny`) and
              a static mesh
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from scene_fuzz import fmt

FAMILIES = ("tiny", "negative", "negative_x", "dup", "flat_grid", "dup_grid", "epsilon", "overflow", "geometric",
            "caps", "mixed")
TINY_T = (1, 2, 3, 4, 9)
CAPS_T = (3136, 3137, 4096, 4097)
FIRST_TIME = 3.1415927      # cosf(t) == -1: yaw 0

# The committed set (tests/golden/meshfuzz/).  Seeds chosen so that the coverage conditions of
# tests/test_mesh_fuzz_golden.py hold.
COMMITTED = ([("tiny", s) for s in range(5)] + [("negative", s) for s in (0, 1, 2, 3, 4)] +
             [("negative_x", 0), ("negative_x", 1), ("dup", 0), ("dup", 1), ("flat_grid", 0), ("flat_grid", 1),
              ("flat_grid", 2), ("dup_grid", 0), ("dup_grid", 1), ("epsilon", 0), ("epsilon", 1), ("overflow", 0), ("overflow", 1),
              ("geometric", 0), ("geometric", 1)] + [("caps", s) for s in range(4)] + [("mixed", 0)])


@dataclass(frozen=True)
class MeshCase:
    family: str
    seed: int
    objs: dict                      # stem -> OBJ text
    text: str                       # the .rtxscene file
    times: tuple                    # Update times (binary32 values)
    triangles: dict = field(default_factory=dict)   # stem -> T

    @property
    def name(self) -> str:
        return f"{self.family}_{self.seed}"

    @property
    def obj(self) -> str:
        """The OBJ text of a single-mesh case."""
        (text,) = self.objs.values()
        return text

    def time_list(self, n=None) -> str:
        """The first n times as the reference harness reads them (t1,t2,...)."""
        return ",".join(fmt(t) for t in self.times[:n])

    def write(self, folder):
        """Write the OBJ files into `folder` and `folder`/Resources (the reference harness reads
        Resources/<stem>.obj below its working directory) and the scene file; returns its path."""
        res = folder / "Resources"
        res.mkdir(exist_ok=True)
        for stem, text in self.objs.items():
            (folder / f"{stem}.obj").write_text(text)
            (res / f"{stem}.obj").write_text(text)
        scene = folder / f"{self.name}.rtxscene"
        scene.write_text(self.text)
        return scene


def obj_text(verts, faces) -> str:
    rows = ["v " + " ".join(fmt(c) for c in v) for v in verts]
    rows += ["f %d %d %d" % (a + 1, b + 1, c + 1) for a, b, c in faces]
    return "\n".join(rows) + "\n"


def _soup(rng, T, lo=(-1.5, -1.5, -1.5), hi=(1.5, 1.5, 1.5), size=0.3):
    """T triangles with their own vertices: a centre in the box, corners within `size` of it."""
    c = rng.uniform(lo, hi, (T, 1, 3))
    v = (c + rng.uniform(-size, size, (T, 3, 3))).astype(np.float32).reshape(-1, 3)
    return v, [(3 * t, 3 * t + 1, 3 * t + 2) for t in range(T)]


def _grid(n, height, copies=1):
    """n x n cells over integer x, z; two triangles per cell (normals up), each `copies` times."""
    v = [(float(i), float(height(i, j)), float(j)) for j in range(n + 1) for i in range(n + 1)]
    f = []
    for j in range(n):
        for i in range(n):
            a, b, c, d = j * (n + 1) + i, j * (n + 1) + i + 1, (j + 1) * (n + 1) + i, (j + 1) * (n + 1) + i + 1
            for tri in ((a, c, b), (b, c, d)):
                f.extend([tri] * copies)
    return np.array(v, np.float32), f


def _times(rng, last=None):
    """FIRST_TIME, then four multiples of 1/8 in [0.125, 8) (exact in binary32)."""
    t = [FIRST_TIME] + [0.125 * int(k) for k in rng.integers(1, 64, 4)]
    if last is not None:
        t[-1] = last
    return tuple(float(np.float32(x)) for x in t)


_CULLS = ("none", "back", "front")


def _mesh_line(stem, cull, scale=None, at=None, spin=True) -> str:
    t = ["mesh", stem, "1", cull]
    if scale is not None:
        t += ["scale"] + [fmt(x) for x in scale]
    if at is not None:
        t += ["translate"] + [fmt(x) for x in at]
    if spin:
        t.append("spin")
    return " ".join(t)


def _scene(name, camera, floor, light, mesh_lines, fov=45.0) -> str:
    """The camera (it looks down +z), a floor plane at height `floor`, the meshes, a point light."""
    rows = [f"# mesh_fuzz {name}",
            " ".join(["camera"] + [fmt(x) for x in (*camera, fov)]),
            "material lambert 0.9 0.75 0.49 1",
            " ".join(["plane", "0", fmt(floor), "0", "0 1 0 1"])]
    rows += mesh_lines
    rows.append(" ".join(["light", "point"] + [fmt(x) for x in light] + ["1 0.9 0.75"]))
    return "\n".join(rows) + "\n"


def _frame(v, scale, at, t_last):
    """Camera, floor and light (position, intensity) that show the mesh as the last Update leaves it:
    slightly above it, far enough back for its box to fit the 45 degree frame.  Quarter units."""
    q = lambda x: float(np.round(x * 4) / 4)    # noqa: E731
    yaw = (np.cos(t_last) + 1.0) / 2.0 * 2.0 * np.pi
    p = v.astype(np.float64) * (1.0 if scale is None else np.array(scale, np.float64))
    w = np.stack([p[:, 0] * np.cos(yaw) + p[:, 2] * np.sin(yaw), p[:, 1],
                  -p[:, 0] * np.sin(yaw) + p[:, 2] * np.cos(yaw)], 1) + np.array(at, np.float64)
    lo, hi = w.min(0), w.max(0)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    back = half[2] + 1.05 * max(half[0] / 0.62, half[1] / 0.3, 0.75)
    up = max(0.1 * back, min(0.35 * back, 0.4 * (back - half[2]) - half[1]))    # the flatter, the higher
    camera = (q(mid[0]), q(mid[1] + up), q(mid[2] - back))
    light = (q(mid[0] + 0.5 * back), q(mid[1] + back), q(mid[2] - 0.75 * back), q(1.25 * back * back))
    return camera, q(lo[1] - 0.5), light


def _part(family: str, seed: int, rng):
    """One mesh of a family: (verts, faces, cull, scale, translate, last time or None)."""
    scale = at = last = None
    cull = _CULLS[seed % 3]
    if family == "tiny":
        T = TINY_T[seed % 5]
        # spaced along x, so that whatever may split does
        v, f = _soup(rng, T, (0, -0.5, -0.5), (0, 0.5, 0.5), 0.4)
        v[:, 0] += np.repeat(np.linspace(-2, 2, T) if T > 1 else [0.0], 3).astype(np.float32)
        at, cull = (0.0, 0.0, 0.0), "none"
    elif family == "negative":
        if seed % 5 == 4:
            # eight slabs of 128 triangles along x, thin in x, every y negative: at yaw 0 the x axis
            # cuts the mesh into the slabs (eight nodes of exactly 128 on one level: a one-wave
            # node with every lane pair taken), whose y axis then has the FLT_MIN maximum
            v, f = _soup(rng, 8 * 128, (-0.1, -3.0, -0.4), (0.1, -1.0, 0.4), 0.15)
            v[:, 0] = (v[:, 0] * 0.04 + np.repeat(np.arange(8) * 2.0 - 7.0, 3 * 128)).astype(np.float32)
            at, cull, last = (0.0, 0.0, 0.0), "none", 2.125     # yaw 85 degrees at the end: the slabs face the camera
        else:
            # wide: a spread above an eighth of the distance reaches a second bin
            T, wide = ((200, True), (233, False), (3300, True), (3200, False))[seed % 5]
            half = (4.5, 1.5, 3.5) if wide else (1.5, 1.5, 1.5)
            v, f = _soup(rng, T, tuple(-h for h in half), half)
            at = (-50.0, -40.0, -60.0)
    elif family == "negative_x":
        v, f = _soup(rng, 220 + 37 * (seed % 4))
        at = (-30.0, 4.0, 9.0) if seed % 2 == 0 else (7.0, 3.0, -45.0)
    elif family == "dup":
        big = seed % 2 == 0
        v, f = _soup(rng, 3 if big else 21, size=0.5)
        one, rest = f[0], f[1:]
        copies = 5000 if big else 40
        # the copies first (big) or spread among the others (small)
        f = [one] * copies + rest if big else [x for k, r in enumerate(rest) for x in ([one] * 2 + [r])]
        at, cull = (0.5, 0.25, 1.0), "none"
    elif family == "flat_grid":
        v, f = _grid(8, lambda i, j: 0.0)
        v += np.float32(((-4, 0, -4), (0, 2, 0), (3, 2, 1))[seed % 3])
        at, cull = (0.0, -1.0, 0.0), ("back", "none", "none")[seed % 3]
    elif family == "dup_grid":
        n, copies = ((12, 2), (6, 12))[seed % 2]
        bump = rng.integers(0, 4, (n + 1, n + 1)) * 0.125
        v, f = _grid(n, lambda i, j: bump[j, i], copies)
        v *= np.float32([4.0 / n, 1, 4.0 / n])
        at = (3.5, 0.5, -2.25)
    elif family == "epsilon":
        v, f = _soup(rng, 150, size=0.4)
        axis = (1, 0)[seed % 2]
        # every coordinate of the axis is a small multiple of 2^-30: the centroid spread is far
        # below FLT_EPSILON and still not zero
        v[:, axis] = (rng.integers(1, 64, len(v)) * 2.0 ** -30).astype(np.float32)
        at, cull = (0.0, 0.0, 0.0), "none"      # a zero translation keeps the tiny values
    elif family == "overflow":
        v, f = _soup(rng, 120 + 60 * (seed % 2), (-1.5, 0.5, 3.0), (1.5, 3.0, 6.0))
        scale, cull, last = (1e19, 1e19, 1e19), "none", 3.25     # yaw 0.018 at the end: still in view
    elif family == "geometric":
        # triangle k is a unit-box triangle shrunk by r^k towards the origin (corner offsets no
        # smaller than 1e-9, so that no normal underflows): once 4 r^k is below FLT_EPSILON the
        # rest of the progression is one leaf
        T, r = ((120, 0.5), (600, 0.9))[seed % 2]
        s = r ** np.arange(T)
        c = rng.uniform((3.0, -1.0, -1.0), (4.0, 1.0, 1.0), (T, 1, 3)) * s[:, None, None]
        v = (c + rng.uniform(-0.3, 0.3, (T, 3, 3)) * np.maximum(s, 1e-9)[:, None, None]).astype(np.float32)
        v, f = v.reshape(-1, 3), [(3 * t, 3 * t + 1, 3 * t + 2) for t in range(T)]
        at, cull = (0.0, 0.0, 0.0), "none"      # a zero translation keeps the tiny values
    elif family == "caps":
        v, f = _soup(rng, CAPS_T[seed % 4], size=0.1)
        at = (0.0, 0.5, 0.0)
    else:
        raise ValueError(family)
    return v, f, cull, scale, at, last


# mixed: (family, seed, where in the scene)
_MIXED = (("caps", 1, (-3.0, 0.0, 2.0)), ("tiny", 2, (3.0, 2.0, 0.0)), ("dup", 1, (0.0, 0.0, 0.0)),
          ("flat_grid", 1, (-6.0, -2.0, -3.0)), ("geometric", 0, (-4.0, 2.5, 0.0)), ("epsilon", 1, (3.0, -0.5, -1.0)),
          ("dup_grid", 0, (1.0, -1.5, -3.0)))


def make(family: str, seed: int) -> MeshCase:
    fid = FAMILIES.index(family)
    rng = np.random.default_rng((77, fid, seed))
    name = f"{family}_{seed}"
    if family == "mixed":
        objs, lines, tris = {}, [], {}
        for k, (fam, s, at) in enumerate(_MIXED):
            v, f, cull, scale, _, _ = _part(fam, s, np.random.default_rng((77, FAMILIES.index(fam), s)))
            stem = f"mf_{name}_{k}"
            objs[stem], tris[stem] = obj_text(v, f), len(f)
            lines.append(_mesh_line(stem, cull, scale, at))
        v, f = _soup(rng, 30)
        objs[f"mf_{name}_static"], tris[f"mf_{name}_static"] = obj_text(v, f), len(f)
        lines.append(_mesh_line(f"mf_{name}_static", "back", None, (0.0, 3.0, 3.0), spin=False))
        scene = _scene(name, (0.0, 2.0, -11.0), -2.5, (1.0, 5.0, -4.0, 50.0), lines, fov=60.0)
        return MeshCase(family, seed, objs, scene, _times(rng), tris)
    v, f, cull, scale, at, last = _part(family, seed, rng)
    times = _times(rng, last)
    stem = f"mf_{name}"
    if family == "overflow":    # the camera stays at the origin, below the mesh
        camera, floor, light = (0.0, 1.0, 0.0), -2.5, (1.0, 5.0, -4.0, 50.0)
    else:
        camera, floor, light = _frame(v, scale, at, times[-1])
    text = _scene(name, camera, floor, light, [_mesh_line(stem, cull, scale, at)])
    return MeshCase(family, seed, {stem: obj_text(v, f)}, text, times, {stem: len(f)})
