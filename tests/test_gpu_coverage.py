"""Every frame after a shape's first proves that it writes every pixel: the device frame buffer is
filled with words no frame can contain (tests/devbuf.py) right before the frame under test, and read
back raw afterwards.  Every word of a row the frame owns must equal the oracle's frame bit for bit and
every other word must still hold the sentinel — so a tile missing from the dispatch order, a heavy tile
no split launch renders, or a launch that writes a row it does not own cannot hide behind the previous
frame's pixels, as it can in a test that only downloads a repeated frame.

The paths that run from the second frame of a shape on: the cost-ordered dispatch (one view, views with
stripes), its XCD-affine re-deal (RTX_XCD_ORDER=1), split rendering of every tile (RTX_SPLIT=force)
with the deferred join, with more heavy tiles than kMaxHeavyTiles and with a moving camera (the motion
schedule), light-major frames, supersampled frames, two contexts in flight, and the hit pass's planes.
The light-count limits (kMaxSplitLights = kMaxCullLights = kMaxLmLights = 32) are crossed with scenes
of 31, 32 and 33 lights built through the ABI structs.

Each case renders warm-up frames to reach the state under test, asserts through the diagnostics that
it was reached, poisons, renders one frame and checks both planes.  Scenes are pow-free and finite
(Lambert only), so every comparison is bit-exact and no colour word is a NaN."""
import ctypes as C
import os

import numpy as np
import pytest

import aov_ref
import checkers
import devbuf
import gpu_support as gs
import oracle_bind
import ss_ref
from gp1_raytracer_2223_amd import abi
from gp1_raytracer_2223_amd.renderer import AOV_ALL, AOV_DEPTH, AOV_NORMAL, AOV_PRIMITIVE, DeviceContext
from gp1_raytracer_2223_amd.scene import HostScene
from gpu_support import DEV
from test_gpu_aov import SENTINEL as AOV_SENTINEL

pytestmark = pytest.mark.gpu

K_MAX_HEAVY_TILES = 8192   # kMaxHeavyTiles (csrc/rtx_kernels.h)
K_MAX_LIGHTS = 32          # kMaxSplitLights, kMaxCullLights, kMaxLmLights
KNOBS = ("RTX_XCD_ORDER", "RTX_SPLIT", "RTX_SPLIT_PARTS", "RTX_DEFER_JOIN", "RTX_LIGHT_MAJOR", "RTX_CULL_MIN_SA",
         "RTX_CULL_RATIO", "RTX_CULL_ANIMATED")
SPLIT_FORCE = dict(RTX_SPLIT="force", RTX_SPLIT_PARTS="4")   # (4 parts: a short split chain)


def _ctx(**env):
    """A context created under exactly the knobs of `env` (read once, at creation)."""
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update(env)
    try:
        return DeviceContext(DEV)
    finally:
        for k in KNOBS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def _fixture(**env):
    @pytest.fixture(scope="module")
    def f():
        c = _ctx(**env)
        yield c
        c.close()
    return f


plain_ctx = _fixture()
xcd_ctx = _fixture(RTX_XCD_ORDER="1")
split_ctx = _fixture(**SPLIT_FORCE)
split_nodefer_ctx = _fixture(RTX_DEFER_JOIN="0", **SPLIT_FORCE)
lm_ctx = _fixture(RTX_LIGHT_MAJOR="1")
cull_ctx = _fixture(RTX_CULL_MIN_SA="0", RTX_CULL_RATIO="0", RTX_CULL_ANIMATED="1")   # test_gpu_cull's: culls every scene


# ---- scenes, cameras and expected frames: built once per module, never written to ----------------

_oracle = {}


def _moved(cam, dx):
    c = abi.Camera()
    C.memmove(C.byref(c), C.byref(cam), C.sizeof(abi.Camera))
    c.origin[0] = np.float32(cam.origin[0]) + np.float32(dx)
    return c


def _frozen(px, rgb):
    devbuf.assert_legal(px, rgb)   # the sentinels cannot be output
    px.setflags(write=False)
    rgb.setflags(write=False)
    return px, rgb


def _want(name, W, H, mode=3, sh=1, dx=0.0, k=1):
    """The oracle's whole frame of scene `name` with the camera moved by dx along x, supersampled k x k."""
    key = (name, W, H, mode, sh, float(np.float32(dx)), k)
    if key not in _oracle:
        s, cam = gs.view(name)
        px, rgb = oracle_bind.render(s, _moved(cam, dx), abi.make_params(k * W, k * H, mode, sh))
        if k > 1:
            rgb = ss_ref.resolve(rgb, W, H, k)
            px = ss_ref.quantize(rgb)
        _oracle[key] = _frozen(px, rgb)
    return _oracle[key]


def _views(cam, n):
    """n cameras 0.05 apart along x (view 0 = cam) as the array rtx_render_views_async takes."""
    arr = (abi.Camera * n)()
    for v in range(n):
        m = _moved(cam, 0.05 * v)
        C.memmove(C.byref(arr[v]), C.byref(m), C.sizeof(abi.Camera))
    return arr


def _queue(ctx, cams, p, frames=1):
    """Queue `frames` frames of one camera or an array of them, both planes, without waiting."""
    arr = (abi.Camera * 1)(cams) if isinstance(cams, abi.Camera) else cams
    for _ in range(frames):
        abi.check(ctx.lib.rtx_render_views_async(ctx.h, arr, len(arr), C.byref(p), 1), "rtx_render_views_async", ctx.h)
    return len(arr)


def _poisoned(ctx, cams, p, want, what, frames=1):
    """Poison both planes, queue `frames` frames without a sync between them, check."""
    n = 1 if isinstance(cams, abi.Camera) else len(cams)
    devbuf.poison(ctx, n * p.width * p.height, rgb=True)
    _queue(ctx, cams, p, frames)
    devbuf.check(ctx, p, n, [w[0] for w in want], [w[1] for w in want], what)


def _schedule_tiles(ctx):
    """Tiles of the context's current schedule, 0 = none measured yet (rtx_schedule_state)."""
    n = C.c_uint32()
    abi.check(ctx.lib.rtx_schedule_state(ctx.h, None, None, 0, C.byref(n)), "rtx_schedule_state", ctx.h)
    return n.value


def _assert_ordered(ctx, ntiles):
    """The next frame runs in a measured order: a permutation of its tiles (on an XCD-order context the
    re-deal the kernel consumes, too)."""
    assert _schedule_tiles(ctx) >= ntiles
    up = C.POINTER(C.c_uint32)
    order, cost = np.zeros(ntiles, np.uint32), np.zeros(ntiles, np.uint32)
    n = C.c_uint32()
    abi.check(ctx.lib.rtx_schedule_state(ctx.h, order.ctypes.data_as(up), cost.ctypes.data_as(up), ntiles, C.byref(n)),
              "rtx_schedule_state", ctx.h)
    assert np.array_equal(np.sort(order), np.arange(ntiles, dtype=np.uint32))
    rc = ctx.lib.rtx_schedule_xcd_order(ctx.h, order.ctypes.data_as(up), ntiles)
    if rc != abi.RTX_E_STATE:   # RTX_E_STATE: the context has no XCD order
        abi.check(rc, "rtx_schedule_xcd_order", ctx.h)
        assert np.array_equal(np.sort(order), np.arange(ntiles, dtype=np.uint32))
    return rc == abi.RTX_OK


def _tiles(W, H, views=1):
    return ((W + 7) // 8) * ((H + 7) // 8) * views


# ---- cost-ordered dispatch and its XCD-affine re-deal --------------------------------------------

# 41 x 33 = 1353 tiles: two kSchedChunk chunks, the second partial; 41 x 25 = 1025: one tile past a
# chunk; 6 x 4 with partial tiles on both sides; one tile; 5 x 4: fewer than 8 tile columns and rows
ORDER_SHAPES = [(328, 264), (328, 200), (44, 28), (8, 8), (40, 32)]


@pytest.mark.parametrize("W,H", ORDER_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("which", ["plain", "xcd"])
def test_cost_order_one_view(plain_ctx, xcd_ctx, which, W, H):
    ctx = {"plain": plain_ctx, "xcd": xcd_ctx}[which]
    s, cam = gs.view("W4_Bunny")
    want = [_want("W4_Bunny", W, H)]
    p = abi.make_params(W, H)
    ctx.upload(s)
    _queue(ctx, cam, p)                       # frame 1 measures
    assert _assert_ordered(ctx, _tiles(W, H)) == (which == "xcd")
    for f in (2, 3, 4):
        _poisoned(ctx, cam, p, want, f"{which} {W}x{H} frame {f}")


# (views, stripe_rows, stripe_step) at H = 200: 13 stripes of 16 rows, 7 of 32, 5 of 48, the last one
# partial (8 rows) every time; a step of 9 exceeds 7 and 5, so some stripe_first owns no row of a view
STRIPE_CASES = [(3, 16, 2), (3, 32, 3), (3, 48, 9), (8, 16, 3), (8, 32, 9), (8, 48, 2)]


@pytest.mark.parametrize("views,rows,step", STRIPE_CASES)
@pytest.mark.parametrize("which", ["plain", "xcd"])
def test_cost_order_views_and_stripes(plain_ctx, xcd_ctx, which, views, rows, step):
    ctx = {"plain": plain_ctx, "xcd": xcd_ctx}[which]
    W, H = 72, 200
    s, cam = gs.view("W4_Bunny")
    cams = _views(cam, views)
    want = [_want("W4_Bunny", W, H, dx=0.05 * v) for v in range(views)]
    ctx.upload(s)
    empty = 0
    for first in range(step):
        p = abi.make_params(W, H, stripe_rows=rows, stripe_first=first, stripe_step=step)
        empty += sum(not devbuf.owned_rows(p, v).any() for v in range(views))
        _queue(ctx, cams, p)                  # frame 1 of this share measures
        n_stripes = (H + rows - 1) // rows
        owned = (n_stripes + step - 1) // step   # stripes of the largest owner: the launch's tile rows
        assert _assert_ordered(ctx, (W + 7) // 8 * owned * (rows // 8) * views) == (which == "xcd")
        for f in (2, 3):
            _poisoned(ctx, cams, p, want, f"{which} {views} views, {rows}-row stripes {first}/{step}, frame {f}")
    assert (empty > 0) == (step == 9), "a step above the stripe count leaves some view of some share without a row"


# ---- split rendering: every tile heavy ------------------------------------------------------------

@pytest.mark.parametrize("mode,sh", [(3, 1), (3, 0), (0, 1)])
@pytest.mark.parametrize("name", ["W4_Bunny", "Bunny8Lights"])
@pytest.mark.parametrize("W,H", [(256, 144), (44, 28)], ids=lambda v: str(v))
@pytest.mark.parametrize("which", ["defer", "nodefer"])
def test_split_force(split_ctx, split_nodefer_ctx, which, W, H, name, mode, sh):
    """Frame 2 is the first one the split launches render; frames 3.. repeat it, and a repeated frame's
    main kernel starts beside the previous frame's chain (the deferred join; RTX_DEFER_JOIN=0: never)."""
    ctx = {"defer": split_ctx, "nodefer": split_nodefer_ctx}[which]
    s, cam = gs.view(name)
    want = [_want(name, W, H, mode, sh)]
    p = abi.make_params(W, H, mode, sh)
    ctx.upload(s)
    _queue(ctx, cam, p)                       # the measured frame: selects the heavy set
    heavy, parts = ctx.split_info()
    assert parts > 1 and heavy == _tiles(W, H), (heavy, parts)
    for f in (2, 3):
        _poisoned(ctx, cam, p, want, f"{name} m{mode}s{sh} {W}x{H} frame {f}")
    assert ctx.split_info()[0] == _tiles(W, H)
    # three repeats queued back to back: every owned word written by one of them
    _poisoned(ctx, cam, p, want, f"{name} m{mode}s{sh} {W}x{H} three repeats", frames=3)


def test_split_more_heavy_tiles_than_the_cap(split_ctx):
    """128 x 65 = 8320 tiles, all heavy: the heavy set is clamped to kMaxHeavyTiles; the split launches
    render those and the main kernel the 128 tiles past the cap."""
    W, H = 1024, 520
    assert _tiles(W, H) == K_MAX_HEAVY_TILES + 128
    s, cam = gs.view("W4_Bunny")
    want = [_want("W4_Bunny", W, H)]
    p = abi.make_params(W, H)
    split_ctx.upload(s)
    _queue(split_ctx, cam, p)
    heavy, parts = split_ctx.split_info()
    assert parts > 1 and heavy == K_MAX_HEAVY_TILES, (heavy, parts)
    _poisoned(split_ctx, cam, p, want, "8320 heavy tiles, frame 2")
    assert split_ctx.split_info()[0] == K_MAX_HEAVY_TILES


def test_split_with_a_moving_camera(split_ctx):
    """The motion schedule: every frame is measured and split, and PHASE 3 must hand every hit-key and
    occlusion slot back reset (hit_key = ~0, occ_bits = 0) for the next frame's other rays."""
    W, H = 256, 144
    s, cam = gs.view("W4_Bunny")
    p = abi.make_params(W, H)
    split_ctx.upload(s)
    _queue(split_ctx, cam, p, 2)              # measured frame, first split frame
    for f, k in enumerate([1, 2, 3, 4, 5, 6, 7, 0]):
        heavy, parts = split_ctx.split_info()
        assert parts > 1 and heavy == _tiles(W, H), (f, heavy, parts)
        _poisoned(split_ctx, _moved(cam, 0.05 * k), p, [_want("W4_Bunny", W, H, dx=0.05 * k)],
                  f"moving camera, frame {f} at +{0.05 * k:.2f}")


# ---- light-major frames ---------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", [(192, 128), (44, 28)], ids=lambda v: str(v))
def test_light_major(lm_ctx, W, H):
    s, cam = gs.view("Bunny8Lights")
    want = [_want("Bunny8Lights", W, H)]
    lm_ctx.upload(s)
    # the warm-up at this shape is a BRDF-mode frame: it allocates the buffers, and the Combined frames
    # after it start a schedule of their own, so the first of them is a shape's first frame
    _queue(lm_ctx, cam, abi.make_params(W, H, 2, 1))
    assert lm_ctx.light_major_info() == (True, 0xFFFFFFFF)
    p = abi.make_params(W, H)
    for f in (1, 2, 3):
        _poisoned(lm_ctx, cam, p, want, f"light-major {W}x{H} frame {f}")
        assert lm_ctx.light_major_info()[0]


# ---- supersampled frames --------------------------------------------------------------------------

@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("W,H", [(37, 23), (80, 60)], ids=lambda v: str(v))
@pytest.mark.parametrize("which", ["plain", "split"])
def test_supersampled(plain_ctx, split_ctx, which, W, H, k):
    ctx = {"plain": plain_ctx, "split": split_ctx}[which]
    s, cam = gs.view("W4_Bunny")
    want = [_want("W4_Bunny", W, H, k=k)]
    p = abi.make_params(W, H)
    ctx.upload(s)
    ctx.set_supersample(k)
    try:
        _queue(ctx, cam, p)
        if which == "split":
            heavy, parts = ctx.split_info()
            assert parts > 1 and heavy == _tiles(k * W, k * H), (heavy, parts)
        else:
            _assert_ordered(ctx, _tiles(k * W, k * H))
        for f in (2, 3):
            _poisoned(ctx, cam, p, want, f"{which} {W}x{H} k={k} frame {f}")
    finally:
        ctx.set_supersample(1)


# ---- two contexts in flight -----------------------------------------------------------------------

def test_two_contexts_in_flight(plain_ctx):
    W, H = 320, 180
    s, cam = gs.view("Synthetic100k")
    want = [_want("Synthetic100k", W, H)]
    p = abi.make_params(W, H)
    other = _ctx()
    try:
        pair = (plain_ctx, other)
        for c in pair:
            c.upload(s)
            _queue(c, cam, p, 2)
        for c in pair:
            _assert_ordered(c, _tiles(W, H))
            devbuf.poison(c, W * H, rgb=True)
        for i in range(12):   # enqueued without waiting: the two contexts' launches overlap
            _queue(pair[i % 2], cam, p)
        for i, c in enumerate(pair):
            devbuf.check(c, p, 1, [want[0][0]], [want[0][1]], f"context {i} of two in flight")
    finally:
        other.close()


# ---- the hit pass ---------------------------------------------------------------------------------

def _word(x):
    return int(np.asarray(x).reshape(1).view(np.uint32)[0])


@pytest.fixture(scope="module")
def aov_want():
    """The checker's planes of the pass below (tests/aov_ref.py), computed once."""
    s, cam = gs.view("W4_Bunny")
    want = aov_ref.planes(checkers.lib(), s, cam, 37, 53)
    for a in want.values():
        a.setflags(write=False)
    return want


@pytest.mark.parametrize("mask", [AOV_DEPTH, AOV_NORMAL | AOV_PRIMITIVE, AOV_ALL], ids=["depth", "normal_primitive", "all"])
def test_hit_pass_writes_its_planes_rows_only(plain_ctx, aov_want, mask):
    """On the device: the planes a mask names hold the checker's values in the rows the pass owns, and
    everything else — unnamed planes, rows it does not own, the colour frame buffer — keeps its sentinel."""
    W, H, step = 37, 53, 3
    ctx = plain_ctx
    s, cam = gs.view("W4_Bunny")
    want = aov_want
    elems ={"depth": 1, "normal": 3, "material": 1, "primitive": 1}
    for k in aov_ref.NAMES:   # the sentinels cannot be output
        assert not (want[k].view(np.uint32) == _word(AOV_SENTINEL[k])).any(), k
    ctx.upload(s)
    full = abi.make_params(W, H)
    _queue(ctx, cam, full)                        # a colour frame and a pass of every plane at this shape:
    ctx.render_aov_async(cam, full, AOV_ALL)      # the buffers below exist and hold W x H elements
    for first in range(step):
        ctx.synchronize()
        d = ctx.device_aov_buffers()
        assert all(d.values())
        for k in aov_ref.NAMES:
            devbuf.fill(ctx, d[k], elems[k] * W * H, _word(AOV_SENTINEL[k]))
        devbuf.poison(ctx, W * H, rgb=True)
        p = abi.make_params(W, H, stripe_rows=16, stripe_first=first, stripe_step=step)
        ctx.render_aov_async(cam, p, mask)
        ctx.synchronize()
        assert ctx.device_aov_buffers() == d
        own = devbuf.owned_rows(p, 0)
        assert own.any() and not own.all()
        for k in aov_ref.NAMES:
            got = devbuf.read(ctx, d[k], elems[k] * W * H).reshape(H, -1)
            sentinel = np.uint32(_word(AOV_SENTINEL[k]))
            if mask & aov_ref.BITS[k]:
                assert aov_ref.same(got[own].view(want[k].dtype), want[k].reshape(H, -1)[own]), (k, first)
                assert (got[~own] == sentinel).all(), f"{k}: rows share {first} does not own were written"
            else:
                assert (got == sentinel).all(), f"{k}: a plane the mask does not name was written"
        px, rgb = devbuf.peek(ctx, W * H, rgb=True)
        assert (px == devbuf.PX_SENTINEL).all() and (rgb == devbuf.RGB_SENTINEL).all(), "the pass wrote the colour buffer"


# ---- the light-count limits -----------------------------------------------------------------------

LW, LH = 44, 28


class _Keep:
    """Keeps the host scene and the ctypes light array of a hand-built scene alive."""


_room = {}


def _room_scene(tmp_path_factory, n_lights, only=None):
    """The Lambert room (five planes) with lowpoly_bunny2 and n point lights at distinct positions
    strictly inside it (|x| < 5, 0 < y < 10, z < 10); with `only`, every other light has intensity 0.
    The scene file gives the geometry; the light list replaces the file's through the ABI struct."""
    key = (n_lights, only)
    if key in _room:
        return _room[key][1:]
    path = tmp_path_factory.mktemp("room") / "room.rtxscene"
    path.write_text("\n".join([
        "camera 0 3 -9 45",
        "material lambert 0.49 0.57 0.57 1",
        "material lambert 1 1 1 1",
        "mesh lowpoly_bunny2 2 back scale 2 2 2",
        "plane 0 0 10   0 0 -1  1",
        "plane 0 0 0    0 1 0   1",
        "plane 0 10 0   0 -1 0  1",
        "plane 5 0 0   -1 0 0   1",
        "plane -5 0 0   1 0 0   1",
        "light point 0 5 5  50 1 1 1",
    ]) + "\n")
    keep = _Keep()
    keep.hs = HostScene(f"file:{path}")
    base, cam = keep.hs.view()
    keep.lights = (abi.Light * n_lights)()
    for i in range(n_lights):   # 7, 5 and 3 are coprime to 33: no two lights share a coordinate
        L = keep.lights[i]
        L.origin[:] = (-4.0 + 8.0 * ((7 * i) % 33) / 32.0, 2.0 + 6.0 * ((5 * i) % 33) / 32.0,
                       -6.0 + 14.0 * ((3 * i) % 33) / 32.0)
        L.color[:] = (1.0 - 0.02 * (i % 7), 0.6 + 0.05 * (i % 5), 0.45 + 0.05 * (i % 11))
        L.intensity = 4.0 if only is None or i == only else 0.0
        L.type = abi.RTX_LIGHT_POINT
    s = abi.Scene()
    C.memmove(C.byref(s), C.byref(base), C.sizeof(abi.Scene))
    s.lights, s.n_lights = keep.lights, n_lights
    _room[key] = (keep, s, cam)
    return s, cam


def _room_want(s, cam, mode=3, sh=1):
    return _frozen(*oracle_bind.render(s, cam, abi.make_params(LW, LH, mode, sh)))


def _room_frames(ctx, s, cam, want, what):
    """Frames 1, 2 and 3 of the Combined schedule, each poisoned first (the warm-up that allocates the
    buffers at this shape is a BRDF-mode frame, a schedule of its own); returns after frame 1 measured."""
    ctx.upload(s)
    _queue(ctx, cam, abi.make_params(LW, LH, 2, 1))
    p = abi.make_params(LW, LH)
    for f in (1, 2, 3):
        _poisoned(ctx, cam, p, [want], f"{what} frame {f}")
        yield f


@pytest.mark.parametrize("n_lights", [K_MAX_LIGHTS - 1, K_MAX_LIGHTS, K_MAX_LIGHTS + 1])
@pytest.mark.parametrize("which", ["plain", "split", "cull", "lm"])
def test_light_count_limits(plain_ctx, split_ctx, cull_ctx, lm_ctx, tmp_path_factory, which, n_lights):
    """31, 32 and 33 lights: every frame is the oracle's, and each limit's fallback (no split, no cull
    records, one piece instead of light-major) starts exactly at 33."""
    ctx = {"plain": plain_ctx, "split": split_ctx, "cull": cull_ctx, "lm": lm_ctx}[which]
    s, cam = _room_scene(tmp_path_factory, n_lights)
    within = n_lights <= K_MAX_LIGHTS
    for f in _room_frames(ctx, s, cam, _room_want(s, cam), f"{which} {n_lights} lights"):
        if which == "split":
            heavy, parts = ctx.split_info()
            assert (parts > 0) == within and (parts > 1) == within, (n_lights, parts)
            assert heavy == (_tiles(LW, LH) if within else 0), (n_lights, heavy)
        elif which == "cull":
            assert ctx.cull_info()[0] == within, n_lights
        elif which == "lm":
            assert ctx.light_major_info()[0] == within, n_lights
        else:
            _assert_ordered(ctx, _tiles(LW, LH))


def test_occlusion_bit_of_light_31(split_ctx, tmp_path_factory):
    """32 lights of which only the last shines: the split path's per-pixel occlusion word must carry
    bit 31 (1u << li), or the frame loses its only shadows."""
    s, cam = _room_scene(tmp_path_factory, K_MAX_LIGHTS, only=K_MAX_LIGHTS - 1)
    lit, shadowed = _room_want(s, cam, 3, 0), _room_want(s, cam, 3, 1)
    assert not np.array_equal(lit[0], shadowed[0]), "light 31 casts no visible shadow: the case shows nothing"
    for f in _room_frames(split_ctx, s, cam, shadowed, "only light 31"):
        heavy, parts = split_ctx.split_info()
        assert parts > 1 and heavy == _tiles(LW, LH), (f, heavy, parts)
