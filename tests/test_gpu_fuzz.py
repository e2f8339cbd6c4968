"""The device against the oracle on the seeded adversarial scenes of tests/scene_fuzz.py — the
scene-content axes the catalogue never varies: kd != 1, Phong exponents 0 and 200, roughness 0,
metalness 0.5, non-unit plane normals, mirrored and front- / no-cull meshes, ties between
primitive kinds, zero lights, and frames that contain NaN and inf.  The oracle is pinned to the
reference on the committed part of the set (tests/test_fuzz_golden.py); here the committed scenes
and further seeds render on the device in the default, the generic (RTX_NO_SPEC=1) and the split
(RTX_SPLIT=force) contexts, supersampled, and through the work counters; the specialised variant
each family is built for is checked with rtx_spec_info.  Records no scene file can express
(unknown material kinds and light types, no lights, no primitives, material 255 of 256, other
pixel formats, frames below one wave tile) are built through the ABI structs.

Comparison (_compare_nf): NaN positions identical; where the oracle's colour holds a NaN the uint32
pixel is equal too; every other value bit-equal when no powf ran (modes 0 and 1, or no Phong /
Cook-Torrance shade in the oracle's counters), else within the project's 1e-4 per channel and
1 LSB.  No pixel is excluded."""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_bind
import scene_fuzz
import ss_ref
from gp1_raytracer_2223_amd import abi
from gp1_raytracer_2223_amd.renderer import DeviceContext
from gpu_support import DEV

pytestmark = pytest.mark.gpu

TOL = 1e-4
W, H = 44, 28                    # five wave tiles and a half across, three and a half down
TILES = 6 * 4

COMMITTED = list(scene_fuzz.COMMITTED)
# further seeds generated at test time; the odd ones with a seeded pitch, yaw and fov
EXTRA = [(f, s) for f in scene_fuzz.FAMILIES for s in (10, 11, 12)] + [(f, 13) for f in ("open", "nonfinite", "ties", "room2")]
ALL = COMMITTED + EXTRA
FIRST = [next(c for c in COMMITTED if c[0] == f) for f in scene_fuzz.FAMILIES]   # one scene per family
MODES_COMMITTED = [(3, 1), (3, 0), (2, 1), (1, 1), (0, 1)]
MODES_EXTRA = [(3, 1), (2, 0)]


def _id(c):
    return f"{c[0]}_{c[1]}"


def _modes(case):
    return MODES_COMMITTED if case in COMMITTED else MODES_EXTRA


# ---- contexts, scenes and oracle frames: built once per module --------------------------------

def _env_ctx(name, value):
    os.environ[name] = value   # read once, at context creation
    try:
        return DeviceContext(DEV)
    finally:
        del os.environ[name]


@pytest.fixture(scope="module")
def generic_ctx():
    ctx = _env_ctx("RTX_NO_SPEC", "1")
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def split_ctx():
    ctx = _env_ctx("RTX_SPLIT", "force")
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def ss_ctx():
    ctx = DeviceContext(DEV)
    ctx.set_supersample(2)
    yield ctx
    ctx.close()


_dir = None
_scenes = {}
_oracle = {}
_counts = {}


@pytest.fixture(scope="module", autouse=True)
def _scene_dir(tmp_path_factory):
    global _dir
    _dir = tmp_path_factory.mktemp("fuzz")
    yield
    _scenes.clear()


def _scene(case):
    """(FuzzScene, rtx_scene, camera) of (family, seed); the host scene stays alive in the cache."""
    if case not in _scenes:
        family, seed = case
        fs = scene_fuzz.make(family, seed, camera=case in EXTRA and seed % 2 == 1)
        hs = scene_fuzz.host_scene(fs, _dir / f"{fs.name}.rtxscene")
        _scenes[case] = (fs, hs, *hs.view())
    fs, _, s, cam = _scenes[case]
    return fs, s, cam


def _ref(case, mode, sh, w=W, h=H):
    """The oracle's frame (computed once, never written to)."""
    key = (case, mode, sh, w, h)
    if key not in _oracle:
        _, s, cam = _scene(case)
        px, rgb = oracle_bind.render(s, cam, abi.make_params(w, h, mode, sh))
        px.setflags(write=False)
        rgb.setflags(write=False)
        _oracle[key] = (px, rgb)
    return _oracle[key]


def _exact(case, mode, sh, w=W, h=H):
    """No powf ran: modes 0 and 1 never shade, else by the oracle's counters of this very frame."""
    if mode in (0, 1):
        return True
    key = (case, mode, sh, w, h)
    if key not in _counts:
        _, s, cam = _scene(case)
        _counts[key] = oracle_bind.count(s, cam, abi.make_params(w, h, mode, sh))
    c = dict(zip(oracle_bind.COUNTER_NAMES, _counts[key].tolist()))
    return c["shade_phong"] == 0 and c["shade_ct"] == 0


def _channels(px, fmt=abi.XRGB8888):
    return np.stack([(px >> fmt[0]) & 255, (px >> fmt[1]) & 255, (px >> fmt[2]) & 255], -1).astype(np.int32)


def _compare_nf(name, gpu, ref, exact, fmt=abi.XRGB8888):
    gpx, grgb = gpu
    rpx, rrgb = ref
    assert gpx.shape == rpx.shape and grgb.shape == rrgb.shape, name
    gn, rn = np.isnan(grgb), np.isnan(rrgb)
    assert np.array_equal(gn, rn), f"{name}: NaN positions differ at {np.flatnonzero(gn != rn)[:8]} " \
                                   f"(device {int(gn.sum())}, oracle {int(rn.sum())})"
    nan_px = rn.reshape(-1, 3).any(axis=1)
    assert np.array_equal(gpx[nan_px], rpx[nan_px]), f"{name}: pixels of NaN colours differ"
    gw, rw = grgb.view(np.uint32), rrgb.view(np.uint32)
    if exact:
        bad = (gw != rw) & ~rn
        assert not bad.any(), f"{name}: {int(bad.sum())} colour words differ, first at {int(np.argmax(bad))}: " \
                              f"{grgb[np.argmax(bad)]!r} vs {rrgb[np.argmax(bad)]!r}"
        assert np.array_equal(gpx, rpx), f"{name}: {int((gpx != rpx).sum())} pixels differ"
        return
    inf = np.isinf(grgb) | np.isinf(rrgb)
    assert np.array_equal(gw[inf], rw[inf]), f"{name}: infinite values differ"
    fin = ~rn & ~inf
    d = np.abs(grgb[fin] - rrgb[fin])
    assert float(d.max(initial=0.0)) <= TOL, f"{name}: max-abs {d.max()}"
    lsb = int(np.abs(_channels(gpx, fmt) - _channels(rpx, fmt)).max(initial=0))
    assert lsb <= 1, f"{name}: {lsb} LSB"
    other = ~np.uint32((255 << fmt[0]) | (255 << fmt[1]) | (255 << fmt[2]))
    assert np.array_equal(gpx & other, rpx & other), f"{name}: bits outside the channels differ"


def _same_nf(name, a, b):
    """Two device frames: NaN positions equal, every other word and every pixel bit-equal."""
    an, bn = np.isnan(a[1]), np.isnan(b[1])
    assert np.array_equal(an, bn), f"{name}: NaN positions differ"
    assert np.array_equal(a[1].view(np.uint32)[~an], b[1].view(np.uint32)[~bn]), f"{name}: colour words differ"
    assert np.array_equal(a[0], b[0]), f"{name}: {int((a[0] != b[0]).sum())} pixels differ"


# ---- scene files -------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ALL, ids=_id)
def test_default_context_two_frames(gpu_ctx, case):
    """The first frame after an upload runs in identity tile order, the second in cost order."""
    fs, s, cam = _scene(case)
    for mode, sh in _modes(case):
        p = abi.make_params(W, H, mode, sh)
        gpu_ctx.upload(s)
        for k in range(2):
            _compare_nf(f"{fs.name}/m{mode}s{sh}/frame{k}", gpu_ctx.render(cam, p), _ref(case, mode, sh),
                        _exact(case, mode, sh))


@pytest.mark.parametrize("case", ALL, ids=_id)
def test_generic_equals_default(gpu_ctx, generic_ctx, case):
    fs, s, cam = _scene(case)
    gpu_ctx.upload(s)
    generic_ctx.upload(s)
    for mode, sh in MODES_EXTRA:
        p = abi.make_params(W, H, mode, sh)
        _same_nf(f"{fs.name}/m{mode}s{sh}", gpu_ctx.render(cam, p), generic_ctx.render(cam, p))
        assert generic_ctx.spec_info()[1] == -1


_parts = {}


def _split_case(split_ctx, gpu_ctx, case):
    fs, s, cam = _scene(case)
    split_ctx.upload(s)
    gpu_ctx.upload(s)
    for mode, sh in MODES_EXTRA:
        p = abi.make_params(W, H, mode, sh)
        split_ctx.render(cam, p)                      # measured frame: selects the heavy set
        heavy, parts = split_ctx.split_info()
        if parts > 1:                                 # (a tree of one part renders unsplit)
            assert heavy == TILES, (heavy, parts)     # every 8x8 wave tile
        _parts[case] = parts
        got = split_ctx.render(cam, p)                # rendered by the split launches
        _same_nf(f"{fs.name}/m{mode}s{sh}/split vs one piece", got, gpu_ctx.render(cam, p))
        _compare_nf(f"{fs.name}/m{mode}s{sh}/split", got, _ref(case, mode, sh), _exact(case, mode, sh))
    return _parts[case]


def _has_mesh(case):
    return "\nmesh " in scene_fuzz.make(*case).text


WITH_MESH = [c for c in ALL if _has_mesh(c)]


@pytest.mark.parametrize("case", WITH_MESH, ids=_id)
def test_split_context(split_ctx, gpu_ctx, case):
    _split_case(split_ctx, gpu_ctx, case)


def test_split_context_did_split(split_ctx, gpu_ctx):
    """The family set is not vacuous for the split path: committed scenes of several families render
    with more than one BVH frontier part."""
    for case in [c for c in COMMITTED if c in WITH_MESH and c not in _parts]:
        _split_case(split_ctx, gpu_ctx, case)
    split = {c[0] for c in COMMITTED if _parts.get(c, 0) > 1}
    assert len(split) >= 3, _parts


@pytest.mark.parametrize("case", FIRST, ids=_id)
def test_supersample_2(ss_ctx, case):
    """Each sample is the reference's pixel of the 2W x 2H frame, the mean in tree order: a NaN or
    inf sample propagates through the sums like any float."""
    fs, s, cam = _scene(case)
    _, hi = _ref(case, 3, 1, 2 * W, 2 * H)
    with np.errstate(invalid="ignore", over="ignore"):
        rgb = ss_ref.resolve(hi, W, H, 2)
        px = ss_ref.quantize(rgb)
    ss_ctx.upload(s)
    _compare_nf(f"{fs.name}/ss2", ss_ctx.render(cam, abi.make_params(W, H)), (px, rgb),
                _exact(case, 3, 1, 2 * W, 2 * H))


@pytest.mark.parametrize("case", FIRST, ids=_id)
def test_work_counters_match_oracle(gpu_ctx, case):
    _, s, cam = _scene(case)
    p = abi.make_params(W, H)
    gpu_ctx.upload(s)
    g = gpu_ctx.count_work(cam, p)
    o = oracle_bind.count(s, cam, p)
    assert np.array_equal(g, o), dict(zip(oracle_bind.COUNTER_NAMES, zip(g.tolist(), o.tolist())))


K_COMB_SHADOWS = 64   # kSpecCombShadows (csrc/rtx_kernels.h)


@pytest.mark.parametrize("case", [c for c in ALL if c[0].startswith("room") or c[0] == "open"], ids=_id)
def test_family_takes_its_variant(gpu_ctx, case):
    """roomN is built for kSpecVariants[N], open for the generic kernel (-1); without Combined
    lighting and shadows every scene takes the generic kernel."""
    family = case[0]
    want = int(family[4:]) if family.startswith("room") else -1
    _, s, cam = _scene(case)
    gpu_ctx.upload(s)
    assert gpu_ctx.spec_info()[1] == -1               # nothing launched yet
    gpu_ctx.render(cam, abi.make_params(W, H, 3, 1))
    facts, variant = gpu_ctx.spec_info()
    assert variant == want, (family, variant, hex(facts))
    assert facts & K_COMB_SHADOWS
    gpu_ctx.render(cam, abi.make_params(W, H, 2, 1))
    facts, variant = gpu_ctx.spec_info()
    assert variant == -1 and not facts & K_COMB_SHADOWS, (family, variant, hex(facts))


# ---- records no scene file can express ---------------------------------------------------------

class _Arrays:
    """Keeps the ctypes arrays of a hand-built scene alive."""


LAMBERT, SOLID = abi.RTX_MAT_LAMBERT, abi.RTX_MAT_SOLID_COLOR
_POINT = (abi.RTX_LIGHT_POINT, (1.0, 4.0, -1.0), (1.0, 0.9, 0.8), 30.0)


def _camera(origin=(0.0, 1.5, -6.0), fov=0.5):
    cam = abi.Camera()
    cam.origin[:] = origin
    cam.right[:] = (1.0, 0.0, 0.0)
    cam.up[:] = (0.0, 1.0, 0.0)
    cam.forward[:] = (0.0, 0.0, 1.0)
    cam.fov = fov
    return cam


def _records(materials, spheres=(), planes=(), mesh_material=None, lights=(_POINT,)):
    """materials: (kind, colour, kd); spheres: (origin, radius, material); planes: (origin, normal,
    material); mesh_material: a no-cull quad (x in +-1, y in [0.5, 2.5], z = 3) in one leaf;
    lights: (type, origin, colour, intensity)."""
    keep = _Arrays()
    s = abi.Scene()
    keep.mat = (abi.Material * len(materials))()
    for k, (kind, colour, kd) in enumerate(materials):
        keep.mat[k].kind = kind
        keep.mat[k].color[:] = colour
        keep.mat[k].kd = kd
    s.materials, s.n_materials = keep.mat, len(materials)
    if spheres:
        keep.sph = (abi.Sphere * len(spheres))()
        for k, (o, r, m) in enumerate(spheres):
            keep.sph[k].origin[:] = o
            keep.sph[k].radius, keep.sph[k].material = r, m
        s.spheres, s.n_spheres = keep.sph, len(spheres)
    if planes:
        keep.pl = (abi.Plane * len(planes))()
        for k, (o, n, m) in enumerate(planes):
            keep.pl[k].origin[:] = o
            keep.pl[k].normal[:] = n
            keep.pl[k].material = m
        s.planes, s.n_planes = keep.pl, len(planes)
    if mesh_material is not None:
        pos = [-1, 0.5, 3, 1, 0.5, 3, 1, 2.5, 3, -1, 2.5, 3]
        idx = [0, 2, 1, 0, 3, 2]
        keep.pos = (C.c_float * len(pos))(*pos)
        keep.idx = (C.c_int32 * len(idx))(*idx)
        keep.nrm = (C.c_float * 6)(0.0, 0.0, -1.0, 0.0, 0.0, -1.0)
        keep.nodes = (abi.BVHNode * 1)()
        keep.nodes[0].min[:] = (-1.0, 0.5, 3.0)
        keep.nodes[0].max[:] = (1.0, 2.5, 3.0)
        keep.nodes[0].first_idx, keep.nodes[0].idx_count, keep.nodes[0].left_node = 0, 6, 0
        keep.mesh = (abi.Mesh * 1)()
        m = keep.mesh[0]
        m.positions, m.n_positions = keep.pos, 4
        m.indices, m.n_indices = keep.idx, 6
        m.normals = keep.nrm
        m.nodes, m.n_nodes = keep.nodes, 1
        m.cull_mode, m.material = abi.RTX_CULL_NONE, mesh_material
        s.meshes, s.n_meshes = keep.mesh, 1
    if lights:
        keep.light = (abi.Light * len(lights))()
        for k, (t, o, c, i) in enumerate(lights):
            keep.light[k].type = t
            keep.light[k].origin[:] = o
            keep.light[k].color[:] = c
            keep.light[k].intensity = i
        s.lights, s.n_lights = keep.light, len(lights)
    s._keep = keep
    return s


_MATS = [(LAMBERT, (0.49, 0.57, 0.57), 1.0), (LAMBERT, (1.0, 0.6, 0.2), 0.35), (SOLID, (0.2, 0.9, 0.4), 0.0),
         (LAMBERT, (0.3, 0.4, 1.0), 2.5)]


def _standard(materials=_MATS, sphere=1, plane=0, mesh=3, lights=(_POINT,)):
    """A floor, a sphere and the quad, lit from the upper right."""
    return _records(materials, spheres=[((-1.5, 1.0, 2.0), 1.0, sphere)], planes=[((0, 0, 0), (0, 1, 0), plane)],
                    mesh_material=mesh, lights=lights)


def _check_records(ctx, s, cam, p, name, fmt=abi.XRGB8888):
    """Lambert and Solid materials only: bit for bit, both frames."""
    ctx.upload(s)
    ref = oracle_bind.render(s, cam, p)
    for k in range(2):
        _compare_nf(f"{name}/frame{k}", ctx.render(cam, p), ref, True, fmt)
    return ref


@pytest.mark.parametrize("kind", [4, -1, 0x7fffffff])
@pytest.mark.parametrize("where", ["sphere", "plane", "mesh"])
def test_unknown_material_kind(gpu_ctx, kind, where):
    """An out-of-catalogue kind shades as colour 0 and keeps the scene off the specialised variants."""
    mats = _MATS + [(kind, (1.0, 1.0, 1.0), 1.0)]
    s = _standard(mats, **{where: 4})
    for mode, sh in [(3, 1), (2, 0)]:
        ref = _check_records(gpu_ctx, s, _camera(), abi.make_params(W, H, mode, sh), f"kind {kind} on the {where}/m{mode}")
        assert gpu_ctx.spec_info()[1] == -1
    assert (ref[0] == 0).any() and (ref[0] != 0).any()   # the unknown material is in view, and others are


@pytest.mark.parametrize("ltype", [2, -1])
@pytest.mark.parametrize("sh", [1, 0])
def test_unknown_light_type(gpu_ctx, ltype, sh):
    """An out-of-catalogue light type has direction 0 (so the normalised direction is 0/0) and
    radiance 0: the Combined frame holds NaN where such a light is not occluded."""
    lights = (_POINT, (ltype, (-2.0, 3.0, 0.0), (1.0, 1.0, 1.0), 20.0), (abi.RTX_LIGHT_POINT, (-3.0, 2.0, -2.0), (0.5, 0.5, 1.0), 15.0))
    s = _standard(lights=lights)
    for mode in (3, 2, 1, 0):
        ref = _check_records(gpu_ctx, s, _camera(), abi.make_params(W, H, mode, sh), f"light type {ltype}/m{mode}s{sh}")
        if mode == 3 and not sh:
            # the case is what it claims (with shadows the NaN shadow ray fails no test of the
            # sphere's, so the light counts as occluded)
            assert np.isnan(ref[1]).any() and not np.isnan(ref[1]).all()
    assert gpu_ctx.spec_info()[1] == -1


@pytest.mark.parametrize("mode,sh", [(3, 1), (3, 0), (1, 1)])
def test_no_lights(gpu_ctx, mode, sh):
    ref = _check_records(gpu_ctx, _standard(lights=()), _camera(), abi.make_params(W, H, mode, sh), "no lights")
    assert not ref[0].any()   # the reference's frame without a light is black


def test_material_255_of_256(gpu_ctx):
    mats = [(LAMBERT, (0.49, 0.57, 0.57), 1.0)] * 255 + [(SOLID, (0.25, 0.5, 0.75), 0.0)]
    s = _standard(mats, sphere=255, plane=0, mesh=254)
    _check_records(gpu_ctx, s, _camera(), abi.make_params(W, H), "material 255/m3s1")
    ref = _check_records(gpu_ctx, s, _camera(), abi.make_params(W, H, 2, 0), "material 255/m2s0")
    # BRDF mode, one light: a pixel of the sphere is its Solid colour itself
    assert (ref[1].reshape(-1, 3) == np.float32([0.25, 0.5, 0.75])).all(axis=1).any()


def test_no_primitives(gpu_ctx):
    """A scene of materials and a light only: every ray misses."""
    s = _records(_MATS[:1])
    ref = _check_records(gpu_ctx, s, _camera(), abi.make_params(W, H), "no primitives")
    assert not ref[0].any()


FORMATS = [(0, 8, 16, 0xFF000000), (24, 16, 8, 0x000000FF), (24, 24, 24, 0)]


@pytest.mark.parametrize("fmt", FORMATS, ids=lambda f: "-".join(map(str, f[:3])))
def test_pixel_formats(gpu_ctx, fmt):
    s = _standard()
    ref = _check_records(gpu_ctx, s, _camera(), abi.make_params(W, H, fmt=fmt), f"format {fmt}", fmt)
    assert ((ref[0] & fmt[3]) == fmt[3]).all()
    if len(set(fmt[:3])) == 3:   # the same channels as XRGB8888 packs
        x = oracle_bind.render(s, _camera(), abi.make_params(W, H))[0]
        assert np.array_equal(_channels(ref[0], fmt), _channels(x))


@pytest.mark.parametrize("w,h", [(1, 1), (1, 9), (9, 1), (7, 9)])
def test_frames_below_one_wave_tile(gpu_ctx, w, h):
    ref = _check_records(gpu_ctx, _standard(), _camera(), abi.make_params(w, h), f"{w}x{h}")
    assert ref[0].any()


def test_two_views_below_one_wave_tile(gpu_ctx):
    w, h, n = 7, 9, 2
    s = _standard()
    p = abi.make_params(w, h)
    views = (abi.Camera * n)()
    cams = [_camera(), _camera(origin=(1.0, 2.0, -5.0), fov=0.7)]
    for v in range(n):
        C.memmove(C.byref(views[v]), C.byref(cams[v]), C.sizeof(abi.Camera))
    gpu_ctx.upload(s)
    for k in range(2):
        abi.check(gpu_ctx.lib.rtx_render_views_async(gpu_ctx.h, views, n, C.byref(p), 1), "views", gpu_ctx.h)
        px = np.full(n * w * h, 0xDEADBEEF, np.uint32)
        rgb = np.full(3 * n * w * h, -1.0, np.float32)
        abi.check(gpu_ctx.lib.rtx_download(gpu_ctx.h, px.ctypes.data_as(C.POINTER(C.c_uint32)),
                                           rgb.ctypes.data_as(C.POINTER(C.c_float))), "download", gpu_ctx.h)
        for v in range(n):
            got = (px[v * w * h:(v + 1) * w * h], rgb[3 * v * w * h:3 * (v + 1) * w * h])
            _compare_nf(f"view {v}/frame{k}", got, oracle_bind.render(s, cams[v], p), True)
