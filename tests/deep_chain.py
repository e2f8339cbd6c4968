"""Left-deep chain BVHs that fill the per-wave DFS stack, and a model of how full it gets — TEST
INFRASTRUCTURE of tests/test_deep_chain_cpu.py and tests/test_gpu_deep_stack_fill.py (plain Python,
no device).

Every walk keeps a stack of pending right siblings per wave: 64 entries in LDS, 1024 in LDS (DEEP) or
max_depth + 1 in HBM (HSTK), chosen from the tree's level depth.  bvh_walk pushes the right child only
while it descends into the left one, so on tests/test_gpu_deep_bvh.py's chain (left = a leaf, right =
the rest) the stack never holds more than one entry, however deep the tree.  `left_deep_scene` mirrors
that chain: inner node j has left = inner node j + 1 and right = the leaf of triangle T - 1 - j, the
deepest inner node has the leaves of triangles 0 and 1, and a wave whose lanes pass both children all
the way down holds T - 1 entries, the tree's level depth, before it tests its first triangle.

`high_water` and `high_water_any` restate the walks' push and pop rules on lane masks (slab tests in
float32 numpy, pinned to the oracle's by the CPU test; triangle tests are the oracle's own), so a test
can demand the fill it relies on before a device is involved."""
from __future__ import annotations

import ctypes as C

import numpy as np

import oracle_bind
from gp1_raytracer_2223_amd import abi
from gp1_raytracer_2223_amd.scene import HostScene

FLT_MAX = np.finfo(np.float32).max
LAYOUTS = ("centred", "corner")
W, H = 160, 96            # the frames of the stack-fill tests: 20 x 12 wave tiles
AIM, FOV = 9.5, 0.04      # the chain starts 9.5 along the camera's forward axis; rtx_camera::fov is tan(half-angle)
# the rim point of a triangle, in units of its half-size from the axis: the direction in which the chain's
# projected triangles grow strictly with k (the bottom edge's midpoint; the right-angle corner)
RIM_DIR = {"centred": (0.0, -1.0), "corner": (1.5, -1.5)}
AXIS_TMAX = 13.0          # beyond the farthest triangle (11.875), before the room's back wall


def _dist(k: int, T: int) -> float:
    return AIM * (1.0 + 0.25 * k / T)


def _half(k: int, T: int) -> float:
    return 0.15 + 1.2 * k / T


def left_deep_mesh(T: int, layout: str, origin=(0.0, 3.0, -9.0)):
    """(positions, indices, normals, nodes) of T triangles facing -z on the axis origin + t (0, 0, 1), the
    nearest the smallest, under the left-deep chain.  Node 0 is the root; inner node j's children are the
    adjacent nodes 2j + 1 (inner node j + 1, or triangle 0's leaf under the deepest) and 2j + 2 (the leaf
    of triangle T - 1 - j), so left-then-right DFS meets the triangles in the order 0, 1, ..., T - 1."""
    assert T >= 2 and layout in LAYOUTS
    ox, oy, oz = origin
    pos, idx, nrm = [], [], []
    for k in range(T):
        s, z = _half(k, T), oz + _dist(k, T)
        if layout == "centred":
            v = [(ox - s, oy - s, z), (ox + s, oy - s, z), (ox, oy + s, z)]
        else:   # the lower-right half of the box [-s/2, 3s/2] x [-3s/2, s/2] about the axis, which it misses
            x0, x1, y0, y1 = ox - 0.5 * s, ox + 1.5 * s, oy - 1.5 * s, oy + 0.5 * s
            v = [(x0, y0, z), (x1, y0, z), (x1, y1, z)]
        b = len(pos)
        pos += v
        idx += [b, b + 2, b + 1]
        nrm.append((0.0, 0.0, -1.0))
    pos = np.array(pos, np.float32)
    idx = np.array(idx, np.int32)
    nrm = np.array(nrm, np.float32)
    tri_lo = pos[idx.reshape(-1, 3)].min(axis=1)
    tri_hi = pos[idx.reshape(-1, 3)].max(axis=1)
    if layout == "corner":   # a leaf's box is the whole shifted box, not the triangle's own: the same here
        assert np.array_equal(tri_lo, pos[0::3]) and np.array_equal(tri_hi[:, :2], pos[2::3, :2])
    pre_lo = np.minimum.accumulate(tri_lo, axis=0)   # the box of triangles 0..k
    pre_hi = np.maximum.accumulate(tri_hi, axis=0)
    nodes = (abi.BVHNode * (2 * T - 1))()

    def put(n, lo, hi, first, count, left):
        for a in range(3):
            nodes[n].min[a] = float(lo[a])
            nodes[n].max[a] = float(hi[a])
        nodes[n].first_idx, nodes[n].idx_count, nodes[n].left_node = first, count, left

    for j in range(T - 1):
        inner = 0 if j == 0 else 2 * j - 1
        put(inner, pre_lo[T - 1 - j], pre_hi[T - 1 - j], 0, 0, 2 * j + 1)
        k = T - 1 - j
        put(2 * j + 2, tri_lo[k], tri_hi[k], 3 * k, 3, 0)
    put(2 * (T - 2) + 1, tri_lo[0], tri_hi[0], 0, 3, 0)
    return pos, idx, nrm, nodes


def scene_with_mesh(pos, idx, nrm, nodes):
    """The Bunny scene's room, lights and camera with one hand-built mesh in the bunny's place (as
    test_gpu_deep_bvh.deep_scene): (scene, camera, whatever the pointers refer to)."""
    hs = HostScene("W4_Bunny")
    base, cam = hs.view()
    m = abi.Mesh()
    m.positions = pos.ctypes.data_as(C.POINTER(C.c_float))
    m.n_positions = len(pos)
    m.indices = idx.ctypes.data_as(C.POINTER(C.c_int32))
    m.n_indices = len(idx)
    m.normals = nrm.ctypes.data_as(C.POINTER(C.c_float))
    m.nodes = nodes
    m.n_nodes = len(nodes)
    m.cull_mode = abi.RTX_CULL_NONE
    m.material = 2
    meshes = (abi.Mesh * 1)(m)
    s = abi.Scene()
    s.spheres, s.n_spheres = base.spheres, base.n_spheres
    s.planes, s.n_planes = base.planes, base.n_planes
    s.lights, s.n_lights = base.lights, base.n_lights
    s.materials, s.n_materials = base.materials, base.n_materials
    s.meshes, s.n_meshes = meshes, 1
    return s, cam, (hs, pos, idx, nrm, nodes, meshes)


def left_deep_scene(T: int, layout: str):
    """(scene, camera, keep-alive): the left-deep chain of T triangles in the Bunny room, seen through
    a narrow camera (fov 0.04) so that a 160 x 96 frame's central tiles pass every box of the chain."""
    hs = HostScene("W4_Bunny")
    _, cam0 = hs.view()
    origin = tuple(float(x) for x in cam0.origin)
    assert (tuple(cam0.right), tuple(cam0.up), tuple(cam0.forward)) == ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
    s, cam, keep = scene_with_mesh(*left_deep_mesh(T, layout, origin))
    cam.fov = FOV
    s._chain = (T, layout)   # (read by rim_rays and axis_waves)
    return s, cam, keep


_views = {}


def view(T: int, layout: str):
    """(scene, camera) of left_deep_scene(T, layout), built once and kept alive; read-only."""
    if (T, layout) not in _views:
        _views[(T, layout)] = left_deep_scene(T, layout)
    return _views[(T, layout)][:2]


def write_mesh(path, pos, idx, nrm, nodes) -> None:
    """The mesh as tests/deep_chain_pack.cpp reads it: int32 T, then positions, indices, normals and the
    nodes (rtx_bvh_node, 36 bytes each), raw."""
    with open(path, "wb") as f:
        f.write(np.array([len(nrm)], np.int32).tobytes())
        f.write(pos.tobytes())
        f.write(idx.tobytes())
        f.write(nrm.tobytes())
        f.write(bytes(nodes))


# ---------------------------------------------------------------- rays

def _rows(o, d, tmin, tmax) -> np.ndarray:
    r = np.zeros((len(d), 8), np.float32)
    r[:, 0:3], r[:, 3:6] = o, d
    r[:, 6], r[:, 7] = tmin, tmax
    return r


def camera_tile_rays(cam: abi.Camera, params: abi.RenderParams, tile: int) -> np.ndarray:
    """The 64 primary rays of wave tile `tile` (8 x 8 pixels, tiles and pixels row-major; of a tile that
    overhangs the frame, the rays of its pixels inside): render_pixel's statements (oracle/rtx_oracle.c)
    in float32, one rounding per operation in its order."""
    f = np.float32
    Wp, Hp = int(params.width), int(params.height)
    cols = -(-Wp // 8)
    assert 0 <= tile < cols * -(-Hp // 8)
    ix, iy = 8 * (tile % cols) + np.arange(64) % 8, 8 * (tile // cols) + np.arange(64) // 8
    inside = (ix < Wp) & (iy < Hp)
    px, py = ix[inside].astype(np.float32), iy[inside].astype(np.float32)
    aspect = f(Wp) / f(Hp)
    fov = f(cam.fov)
    cx = (f(2) * ((px + f(0.5)) / f(Wp)) - f(1)) * aspect * fov
    cy = (f(1) - (f(2) * (py + f(0.5))) / f(Hp)) * fov
    r, u, w = (np.array(v[:], np.float32) for v in (cam.right, cam.up, cam.forward))
    d = np.stack([(r[a] * cx + u[a] * cy) + w[a] * f(1) for a in range(3)], axis=1)
    assert d.dtype == np.float32
    m = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    d = d / m[:, None]
    return _rows(np.array(cam.origin[:], np.float32), d, f(0.0001), FLT_MAX)


def axis_ray(cam: abi.Camera, tmax=FLT_MAX) -> np.ndarray:
    return _rows(np.array(cam.origin[:], np.float32), np.array([cam.forward[:]], np.float32), np.float32(1e-4), tmax)


def rim_rays(scene: abi.Scene, cam: abi.Camera):
    """(rays, tri): for every triangle k one ray from the camera's origin to a point of k that no nearer
    triangle covers, in waves of 64: lane 0 of every wave is the axis ray (tri = -1), lanes 1..63 the rim
    rays of 63 consecutive triangles.  Seen from the origin triangle k is the layout's shape scaled by
    half(k) / dist(k) about the axis, which grows with k: the point half way between k - 1's and k's
    extent along RIM_DIR lies inside k and beyond every nearer triangle.  Directions are not normalised
    (the hit is at t = 1); tmin 1e-4, tmax FLT_MAX."""
    T, layout = scene._chain
    ux, uy = RIM_DIR[layout]
    ratio = [_half(k, T) / _dist(k, T) for k in range(T)]
    assert all(b > a for a, b in zip(ratio, ratio[1:]))
    o = np.array(cam.origin[:], np.float32)
    rows, tri = [], []
    for k in range(T):
        if k % 63 == 0:
            rows.append(axis_ray(cam)[0])
            tri.append(-1)
        rho = 0.5 * ratio[0] if k == 0 else 0.5 * (ratio[k] + ratio[k - 1])
        d = _dist(k, T)
        rows.append(_rows(o, np.array([[ux * rho * d, uy * rho * d, d]], np.float32), np.float32(1e-4), FLT_MAX)[0])
        tri.append(k)
    rays = np.array(rows, np.float32)
    assert rays.shape[0] == T + -(-T // 63) and rays.shape[0] % 64 != 0
    return rays, np.array(tri, np.int64)


def axis_waves(scene: abi.Scene, cam: abi.Camera) -> np.ndarray:
    """130 rays that end before the room's back wall (tmax 13): a wave of 64 axis rays, a wave whose
    lane 0 is the axis ray beside 63 rays that leave the chain's boxes behind at once, and two more axis
    rays.  On the corner layout the axis crosses every box and misses every triangle: nothing occludes
    it, so an any-hit walk pops its whole stack."""
    a = axis_ray(cam, np.float32(AXIS_TMAX))
    away = a.repeat(63, axis=0)
    away[:, 3] = np.float32(1.0) + np.arange(63, dtype=np.float32) / np.float32(64)   # x / z >= 1: outside every box
    return np.concatenate([a.repeat(64, axis=0), a, away, a, a])


# ---------------------------------------------------------------- the occupancy model

def _smin(a, b):
    return np.where(b < a, b, a)   # std::min: (b < a) ? b : a


def _smax(a, b):
    return np.where(a < b, b, a)   # std::max: (a < b) ? b : a


def slab_pass(rays: np.ndarray, lo: np.ndarray, hi: np.ndarray) -> np.ndarray:
    """bool (rays, boxes): GeometryUtils::SlabTest_BVH (the oracle's `slab`) in float32, NaNs included."""
    rays = np.ascontiguousarray(rays, np.float32)
    with np.errstate(all="ignore"):
        inv = np.float32(1) / rays[:, 3:6]
        t_min = t_max = None
        for a in range(3):
            t1 = (lo[None, :, a] - rays[:, None, a]) * inv[:, None, a]
            t2 = (hi[None, :, a] - rays[:, None, a]) * inv[:, None, a]
            n, x = _smin(t1, t2), _smax(t1, t2)
            t_min, t_max = (n, x) if a == 0 else (_smax(t_min, n), _smin(t_max, x))
        return (t_max > 0) & (t_max >= t_min)


def node_arrays(mesh: abi.Mesh):
    """(lo, hi, idx_count, left_node, first_idx) of a mesh's nodes as numpy arrays."""
    raw = np.frombuffer(C.string_at(mesh.nodes, mesh.n_nodes * C.sizeof(abi.BVHNode)), np.uint32).reshape(-1, 9)
    box = raw[:, :6].copy().view(np.float32)
    return box[:, :3], box[:, 3:], raw[:, 7].tolist(), raw[:, 8].tolist(), raw[:, 6].tolist()


def _lane_bits(passed: np.ndarray) -> list:
    """One Python int per box: bit l set when ray l passed it (up to 64 rays)."""
    n = passed.shape[0]
    full = np.zeros((64, passed.shape[1]), bool)
    full[:n] = passed
    packed = np.ascontiguousarray(np.packbits(full.T, axis=1, bitorder="little"))   # (boxes, 8) bytes, lane 0 first
    return packed.view("<u8").reshape(-1).tolist()


class _Tri:
    """Scene::DoesHit's triangle test per (lane, triangle): the oracle's, on the wave's distinct rays."""

    def __init__(self, mesh: abi.Mesh, rays: np.ndarray):
        self.mesh, self.lib = mesh, oracle_bind.lib()
        self.uniq, self.of = np.unique(np.ascontiguousarray(rays, np.float32).view(np.uint32), axis=0, return_inverse=True)
        self.uniq = np.ascontiguousarray(self.uniq).view(np.float32)
        self.of = np.asarray(self.of).reshape(-1).tolist()
        self.seen = {}
        self.out = np.zeros(8, np.float32)

    def occludes(self, lane: int, k: int) -> bool:
        key = (self.of[lane], k)
        if key not in self.seen:
            m = self.mesh
            tri = np.zeros(12, np.float32)
            for v in range(3):
                i = m.indices[3 * k + v]
                tri[3 * v:3 * v + 3] = [m.positions[3 * i + a] for a in range(3)]
            tri[9:12] = [m.normals[3 * k + a] for a in range(3)]
            ray = np.ascontiguousarray(self.uniq[key[0]])
            self.seen[key] = bool(self.lib.rtx_oracle_hit_triangle(oracle_bind.fptr(ray), oracle_bind.fptr(tri), int(m.cull_mode),
                                                                   1, oracle_bind.fptr(self.out)))
        return self.seen[key]


def _walk(mesh: abi.Mesh, rays64: np.ndarray, any_hit: bool):
    """bvh_walk on lane masks: (the largest number of pending entries, pops made while more than 64
    entries were pending, pops in all)."""
    rays64 = np.ascontiguousarray(rays64, np.float32)
    n = rays64.shape[0]
    assert 1 <= n <= 64 and mesh.n_nodes
    lo, hi, count, left, first = node_arrays(mesh)
    bits = _lane_bits(slab_pass(rays64, lo, hi))
    tri = _Tri(mesh, rays64) if any_hit else None
    live = (1 << n) - 1
    node, m = 0, bits[0] & live
    stack, high, deep_pops, pops = [], 0, 0, 0
    if m == 0:
        return 0, 0, 0
    while True:
        descend = False
        if count[node]:
            if any_hit:
                for k in range(first[node] // 3, (first[node] + count[node]) // 3):
                    for lane in range(n):
                        if (m & live) >> lane & 1 and tri.occludes(lane, k):
                            live &= ~(1 << lane)
                if live == 0:
                    return high, deep_pops, pops
        else:
            l = left[node]
            ml, mr = bits[l] & m, bits[l + 1] & m
            if ml:
                if mr:
                    stack.append((l + 1, mr))
                    high = max(high, len(stack))
                node, m, descend = l, ml, True
            elif mr:
                node, m, descend = l + 1, mr, True
        while not descend:
            if not stack:
                return high, deep_pops, pops
            deep_pops += len(stack) > 64
            pops += 1
            node, m = stack.pop()
            if any_hit:
                m &= live
            descend = m != 0


def high_water(scene: abi.Scene, rays64) -> int:
    """The most pending entries one wave of up to 64 rays holds on the scene's mesh in a closest-hit walk:
    a node is entered with the mask of lanes that passed its slab test, both children are tested for those
    lanes, and the right child is pushed when some lane passes the left and some lane the right."""
    return _walk(scene.meshes[0], rays64, False)[0]


def high_water_any(scene: abi.Scene, rays64):
    """The any-hit walk (Scene::DoesHit): a lane leaves at its first occluder, a popped entry keeps its live
    lanes only, and the wave leaves when none is live.  (high-water mark, pops made while more than 64
    entries were pending, pops in all)."""
    return _walk(scene.meshes[0], rays64, True)


def frame_high_water(scene: abi.Scene, cam: abi.Camera, width: int = W, height: int = H) -> np.ndarray:
    """high_water of every wave tile of a frame, in tile order."""
    p = abi.make_params(width, height)
    return np.array([high_water(scene, camera_tile_rays(cam, p, t)) for t in range(-(-width // 8) * -(-height // 8))])
