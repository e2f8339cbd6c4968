"""Ray sets for the ray-query tests — TEST INFRASTRUCTURE.  Seeded numpy, (n, 8) float32 rows
{origin, direction, tmin, tmax}.  The sets are the ones the queries can go wrong on: rays the renderer
never makes (unnormalised, tmin <= 0, infinite tmax, non-finite fields), waves that take each walk
(octant copies, mixed octants, an axis-parallel lane), and the short lengths around a wave boundary."""
from __future__ import annotations

import numpy as np

FLT_MAX = np.finfo(np.float32).max
INF = np.float32(np.inf)
LENGTHS = (1, 63, 64, 65)       # the tail mask and the wave boundary
DEFAULT_BOX = (np.array([-1.0, 0.0, -1.0], np.float32), np.array([1.0, 2.0, 1.0], np.float32))


def mesh_box(scene):
    """The meshes' joint bounding box (the union of their root nodes' boxes), or DEFAULT_BOX."""
    lo, hi = None, None
    for i in range(scene.n_meshes):
        m = scene.meshes[i]
        if m.n_nodes == 0:
            continue
        a, b = np.array(m.nodes[0].min[:], np.float32), np.array(m.nodes[0].max[:], np.float32)
        if not (np.isfinite(a).all() and np.isfinite(b).all()):
            continue
        lo = a if lo is None else np.minimum(lo, a)
        hi = b if hi is None else np.maximum(hi, b)
    return DEFAULT_BOX if lo is None else (lo, hi)


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _rows(o, d, tmin, tmax):
    n = o.shape[0]
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3], r[:, 3:6] = o, d
    r[:, 6], r[:, 7] = tmin, tmax
    return r


def scatter(seed: int, n: int = 1024) -> np.ndarray:
    """Origins uniform in (-6, -1, -3)..(6, 11, 12); unit directions times one of {1e-3, 0.5, 1, 1, 3,
    1e3}; tmin from {1e-4, 0, -1, 0.5}; tmax from {FLT_MAX, inf, 2, 6}."""
    rng = np.random.default_rng(seed)
    o = rng.uniform((-6, -1, -3), (6, 11, 12), size=(n, 3)).astype(np.float32)
    d = _unit(rng, n) * rng.choice(np.array([1e-3, 0.5, 1, 1, 3, 1e3], np.float32), size=(n, 1))
    tmin = rng.choice(np.array([1e-4, 0, -1, 0.5], np.float32), size=n)
    tmax = rng.choice(np.array([FLT_MAX, INF, 2, 6], np.float32), size=n)
    return _rows(o, d.astype(np.float32), tmin, tmax)


def aimed(scene, seed: int, n: int = 1024) -> np.ndarray:
    """Origin uniform in (-4, 0.5, -4)..(4, 8, 8); direction = (a uniform point of the meshes' joint
    bounding box) - origin, unnormalised; tmin 1e-4; tmax from {FLT_MAX, 1.0, 1.5}."""
    rng = np.random.default_rng(seed)
    lo, hi = mesh_box(scene)
    o = rng.uniform((-4, 0.5, -4), (4, 8, 8), size=(n, 3)).astype(np.float32)
    p = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    tmax = rng.choice(np.array([FLT_MAX, 1.0, 1.5], np.float32), size=n)
    return _rows(o, p - o, np.float32(1e-4), tmax)


def octant(scene, seed: int) -> np.ndarray:
    """Ten 64-ray blocks through the meshes' box: block k < 8 has every direction in octant k (bit a set
    = negative on axis a), so its wave walks that octant's node copies; block 8 mixes octants; block 9 is
    block 0 with one axis-parallel lane (a -0 and a +0 component: infinite inverses of both signs), so
    the whole wave takes the exact slab."""
    rng = np.random.default_rng(seed)
    lo, hi = mesh_box(scene)
    blocks = []
    for k in range(10):
        mag = np.abs(_unit(rng, 64)) + np.float32(1e-3)
        if k == 8:
            sign = rng.choice(np.array([-1.0, 1.0], np.float32), size=(64, 3))
        else:
            kk = 0 if k == 9 else k
            sign = np.array([[-1.0 if (kk >> a) & 1 else 1.0 for a in range(3)]], np.float32)
        d = (mag * sign).astype(np.float32)
        p = rng.uniform(lo, hi, size=(64, 3)).astype(np.float32)
        o = (p - d * rng.uniform(1.0, 6.0, size=(64, 1)).astype(np.float32)).astype(np.float32)
        r = _rows(o, d, np.float32(1e-4), FLT_MAX)
        if k == 9:
            c = (lo + hi) / 2
            r[17, 0:3] = (c[0], c[1], lo[2] - 2.0)
            r[17, 3:6] = (-0.0, 0.0, 1.0)
        blocks.append(r)
    return np.concatenate(blocks)


def nonfinite(scene, seed: int) -> np.ndarray:
    """NaN, +inf and -inf in each of the eight fields in turn of a ray aimed at the meshes' box; a zero
    direction; tmax < tmin; and origins exactly on a face of the box with a zero direction component on
    that axis (0 * inf in the slab test).  Each special ray is followed by three plain aimed rays, so
    that its wave holds ordinary rays too."""
    rng = np.random.default_rng(seed)
    lo, hi = mesh_box(scene)
    c = (lo + hi) / 2
    base = np.array([c[0] + 0.3, c[1] + 0.2, lo[2] - 3.0, -0.05, -0.03, 1.0, 1e-4, FLT_MAX], np.float32)
    special = []
    for f in range(8):
        for v in (np.float32(np.nan), INF, -INF):
            r = base.copy()
            r[f] = v
            special.append(r)
    z = base.copy(); z[3:6] = 0.0; special.append(z)
    z = base.copy(); z[6], z[7] = 5.0, 1.0; special.append(z)
    for face in (lo[0], hi[0]):
        z = base.copy(); z[0] = face; z[3] = 0.0; special.append(z)
        z = base.copy(); z[0] = face; z[3] = -0.0; special.append(z)
    z = base.copy(); z[1] = lo[1]; z[4] = 0.0; special.append(z)
    fill = aimed(scene, seed + 1, 3 * len(special))
    out = np.zeros((4 * len(special), 8), np.float32)
    out[0::4] = np.array(special, np.float32)
    out[1::4], out[2::4], out[3::4] = fill[0::3], fill[1::3], fill[2::3]
    return out


def wave_tiles(width: int, height: int) -> np.ndarray:
    """The permutation that puts a row-major width x height frame's pixels into the hit pass's order:
    64 consecutive entries are one 8 x 8 tile (row-major inside it); width and height multiples of 8."""
    assert width % 8 == 0 and height % 8 == 0
    idx = np.arange(width * height, dtype=np.int64).reshape(height // 8, 8, width // 8, 8)
    return idx.transpose(0, 2, 1, 3).reshape(-1)
