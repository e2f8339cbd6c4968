"""Relighting (rtx_render_shadows_async: PHASE 9 of the render kernel; rtx_relight*: rtx_relight_kernel) on the GPU.
The shadow plane equals the CPU checker (tests/relight_ref.py: rayq_ref.shadow + rayq_ref.occluded per light) word
for word, in every specialised variant and the generic kernel, with the room skip, the exact cull and the deep
stacks, for views and stripes and for 32 lights; the relight equals the colour frame of the same parameters word
for word in both planes and through a relighting loop of uploads; both leave the frames, the planes and the
policies alone and fail as the contract says.  The plane (tests/shadowbuf.py) and the frame buffer
(tests/devbuf.py) are poisoned before the launch under test, so every owned word is proved written and no other
word touched.

At 37 x 23 every light of W4_Bunny and of Bunny8Lights has occluded and unoccluded hit pixels (the checker alone
says so: asserted in test 1), so no size or camera was changed for it."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import aov_ref
import devbuf
import gpu_support as gs
import oracle_bind
import relight_ref
import shadowbuf
from checkers import checker  # noqa: F401
from gp1_raytracer_2223_amd import abi
from gp1_raytracer_2223_amd.renderer import AOV_ALL, AOV_DEPTH, DeviceContext, Renderer, aov_host_planes
from gp1_raytracer_2223_amd.scene import HostScene
from gpu_support import CONFIGS, DEV, FP, LIGHTS, MATS, POW_FREE_MODES, UP
from gpu_support import ctx  # noqa: F401
from test_gpu_deep_bvh import deep_scene

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
EXE = ROOT / "gp1_raytracer_2223_amd" / "lib" / "rtx_render"
W, H = 37, 23   # five tile columns and three tile rows, one of each partial; a row is one partial 64-pixel piece


_planes = {}   # (scene, w, h) -> the checker's (bits, hit), computed once


def _want_plane(checker, name, w, h):
    if (name, w, h) not in _planes:
        s, cam = gs.view(name)
        bits, hit = relight_ref.plane(checker, s, cam, w, h)
        bits.setflags(write=False)
        _planes[(name, w, h)] = (bits, hit)
    return _planes[(name, w, h)]


def _shadow_pass(c, want_bits, w, h, what, n_views=1, shape=None):
    """The shadow pass of the last hit pass, into a poisoned plane: every owned word the checker's."""
    c.render_shadows_async()   # (the plane exists at this size: it can be poisoned)
    shadowbuf.poison(c, n_views * w * h)
    c.render_shadows_async()
    shadowbuf.check(c, shape if shape is not None else abi.make_params(w, h), n_views, want_bits, what)


def _relight_and_check(c, w, h, mode, sh, want, what, n_views=1, shape=None):
    """Poison, relight the last passes with (mode, sh), and demand the frame `want` in every owned word."""
    devbuf.poison(c, n_views * w * h, rgb=True)
    # the size and stripe fields of the relight's parameters are ignored: the pass supplies them
    c.relight_async(abi.make_params(1, 1, mode, sh), True)
    devbuf.check(c, shape if shape is not None else abi.make_params(w, h, mode, sh), n_views, want[0], want[1], what)


# ---- 1. the plane equals the checker ----------------------------------------------------------------------

PLANE = ["W4_Bunny", "W4_Optional", "W3", "W4_Reference", "W1", "Bunny8Lights", "fuzz:room0_0"]
_seen = {}   # scene -> the variants its comparison frames took


def _plane_equals_the_checker(c, checker, name, w, h):
    s, cam = gs.view(name)
    bits, _ = _want_plane(checker, name, w, h)
    c.upload(s)
    seen = set()
    gs.frames(c, cam, w, h, [(3, 1)], seen)   # the frame whose shadow rays the pass repeats, and its variant
    room = c.room_info()[0]
    c.render_aov_async(cam, abi.make_params(w, h), AOV_ALL)
    _shadow_pass(c, bits, w, h, f"{name} {w}x{h}")
    got = c.download_shadows()
    assert np.array_equal(got, bits), name
    prim = c.download_aov(aov_host_planes(w, h, AOV_ALL))["primitive"]
    assert not got[prim == 0].any(), f"{name}: a miss has a bit set"
    assert not (got >> np.uint32(s.n_lights)).any(), f"{name}: a bit past the lights is set"
    return seen, room, got, prim != 0


@pytest.mark.parametrize("name", PLANE)
def test_plane_equals_the_checker(ctx, checker, name):
    seen, room, got, hit = _plane_equals_the_checker(ctx, checker, name, W, H)
    _seen[name] = seen
    s, _ = gs.view(name)
    if name == "W4_Bunny":
        assert room, "W4_Bunny renders with the room skip"
    if name in ("W4_Bunny", "Bunny8Lights"):
        assert s.n_lights == (8 if name == "Bunny8Lights" else 3)
        for l in range(s.n_lights):   # every light has an occluded and an unoccluded hit pixel at this size
            b = ((got >> np.uint32(l)) & 1)[hit]
            assert b.any() and not b.all(), (name, l)


@pytest.mark.parametrize("w,h", [(1, 1), (8, 8)])
def test_plane_at_one_pixel_and_one_tile(ctx, checker, w, h):
    _plane_equals_the_checker(ctx, checker, "W4_Bunny", w, h)


def test_the_scenes_covered_every_variant(ctx, checker):
    for name in PLANE:   # (those a selection left out)
        if name not in _seen:
            _seen[name] = _plane_equals_the_checker(ctx, checker, name, W, H)[0]
    got = set().union(*_seen.values())
    assert got >= {-1, 0, 1, 2, 3}, {k: sorted(v) for k, v in _seen.items()}


# ---- 2. the relight equals the frame ------------------------------------------------------------------------

def _relight_equals_the_frame(c, name, w, h, oracle_all_modes=False):
    s, cam = gs.view(name)
    c.upload(s)
    frames = gs.frames(c, cam, w, h, CONFIGS)
    c.render_aov_async(cam, abi.make_params(w, h), AOV_ALL)
    c.render_shadows_async()
    for (mode, sh), want in frames.items():
        _relight_and_check(c, w, h, mode, sh, want, f"{name} {w}x{h} mode {mode} shadows {sh}")
        if oracle_all_modes or mode in POW_FREE_MODES:
            gpx, grgb = devbuf.peek(c, w * h, rgb=True)
            rpx, rrgb = oracle_bind.render(s, cam, abi.make_params(w, h, mode, sh))
            assert np.array_equal(gpx, rpx), (name, mode, sh)
            assert np.array_equal(grgb, rrgb.view(np.uint32)), (name, mode, sh)
    # the blocking call, through the contract's comparison
    devbuf.poison(c, w * h, rgb=True)
    px, rgb = c.relight(abi.make_params(w, h), True)
    assert aov_ref.same(px, frames[(3, 1)][0]) and aov_ref.same(rgb, frames[(3, 1)][1]), name
    return frames


@pytest.mark.parametrize("name", PLANE)
def test_relight_equals_the_frame(ctx, name):
    _relight_equals_the_frame(ctx, name, W, H, oracle_all_modes=name == "W4_Bunny")


@pytest.mark.parametrize("w,h", [(1, 1), (8, 8), (130, 5)])
def test_relight_at_one_pixel_one_tile_and_three_row_pieces(ctx, w, h):
    """(130 pixels: two full 64-pixel pieces of a row and a piece of two.)"""
    _relight_equals_the_frame(ctx, "W4_Bunny", w, h, oracle_all_modes=True)


# ---- 3. the relighting loop -----------------------------------------------------------------------------------

# uploads that keep every shadow ray: only light colours and intensities, only material values
KEEP = {
    "recoloured": (MATS, ["light point 0 5 5  60 0.4 0.7 1", "light point -2.5 5 -5  35 0.3 1 0.5"]),
    "one_light_dark": (MATS, [LIGHTS[0], "light point -2.5 5 -5  0 1 0.8 0.45"]),
    "lambert_to_cook_torrance": ([MATS[0], "material cook_torrance 0.95 0.93 0.88 1 0.3", MATS[2], MATS[3]], LIGHTS),
    "both": ([MATS[0], "material cook_torrance 0.95 0.93 0.88 0 0.6", MATS[2], "material lambert 0.9 0.9 0.2 1"],
             ["light point 0 5 5  80 1 1 1", "light point -2.5 5 -5  20 0.2 0.4 1"]),
}
# uploads that change a shadow ray: refused with shadows on, relit correctly with shadows off
STALE = {
    "moved": (MATS, ["light point 1.5 6 3  50 1 0.61 0.45", LIGHTS[1]]),
    "added": (MATS, LIGHTS + ["light point 3 2 -3  40 0.6 0.8 1"]),
    "removed": (MATS, LIGHTS[:1]),
    "type_changed": (MATS, [LIGHTS[0], "light directional -2.5 5 -5  70 1 0.8 0.45"]),
}


def _relit_equals_a_fresh_render(c, cam, mode, sh, what):
    devbuf.poison(c, W * H, rgb=True)
    c.relight_async(abi.make_params(W, H, mode, sh), True)
    got = devbuf.peek(c, W * H, rgb=True)
    want = c.render(cam, abi.make_params(W, H, mode, sh))
    assert np.array_equal(got[0], want[0]), (what, mode, sh, int((got[0] != want[0]).sum()))
    assert np.array_equal(got[1], want[1].view(np.uint32)), (what, mode, sh)
    return want


def test_relight_loop(tmp_path):
    c = DeviceContext(DEV)
    p = abi.make_params(W, H)
    try:
        base = gs.file_scene(tmp_path, "base", MATS, LIGHTS)
        s, cam = base.view()
        assert s.n_materials == 5
        c.upload(s)
        frames = gs.frames(c, cam, W, H, CONFIGS)
        c.render_aov_async(cam, p, AOV_ALL)
        c.render_shadows_async()
        plane = c.download_shadows()
        assert plane.any()
        for (mode, sh), want in frames.items():   # one pair of passes: every mode and shadow toggle
            _relight_and_check(c, W, H, mode, sh, want, f"base mode {mode} shadows {sh}")
        for name, (mats, lights) in KEEP.items():
            hs = gs.file_scene(tmp_path, name, mats, lights)
            s2, cam2 = hs.view()
            assert s2.n_materials == 5 and bytes(cam2) == bytes(cam)
            c.upload(s2)   # the same geometry, material indices and light positions: no new pass of either kind
            for mode, sh in ((3, 1), (3, 0), (1, 1), (2, 0)):
                want = _relit_equals_a_fresh_render(c, cam, mode, sh, name)
                if mode == 3:
                    assert not np.array_equal(want[0], frames[(mode, sh)][0]), f"{name}: the upload changes nothing"
        assert np.array_equal(c.download_shadows(), plane)   # the plane was only read
        for name, (mats, lights) in STALE.items():
            hs = gs.file_scene(tmp_path, name, mats, lights)
            s2, _ = hs.view()
            c.upload(s2)
            for mode in (3, 0):
                assert c.lib.rtx_relight_async(c.h, C.byref(abi.make_params(W, H, mode, 1)), 1) == abi.RTX_E_STATE, name
            assert b"shadow pass" in c.lib.rtx_last_error(c.h)
            _relit_equals_a_fresh_render(c, cam, 3, 0, name)   # without shadows the plane is not needed
            _relit_equals_a_fresh_render(c, cam, 1, 0, name)
            # ... and a new shadow pass for these lights makes it current again
            c.render_shadows_async()
            _relit_equals_a_fresh_render(c, cam, 3, 1, name + " after a new shadow pass")
        # the base lights again: the plane is the last STALE scene's, so still refused until it is traced again
        c.upload(s)
        assert c.lib.rtx_relight_async(c.h, C.byref(p), 1) == abi.RTX_E_STATE
        c.render_shadows_async()
        _relight_and_check(c, W, H, 3, 1, frames[(3, 1)], "the base scene again")
        # a new hit pass without a new shadow pass
        c.render_aov_async(cam, p, AOV_ALL)
        assert c.lib.rtx_relight_async(c.h, C.byref(p), 1) == abi.RTX_E_STATE
        assert c.lib.rtx_download_shadows(c.h, plane.ctypes.data_as(UP)) == abi.RTX_E_STATE
        _relight_and_check(c, W, H, 3, 0, frames[(3, 0)], "shadows off after a new hit pass")
        c.render_shadows_async()
        _relight_and_check(c, W, H, 3, 1, frames[(3, 1)], "after both passes again")
    finally:
        c.close()


# ---- 4. the walk paths of the shadow pass -----------------------------------------------------------------------

@pytest.mark.parametrize("name", ["Synthetic100k", "W4_Optional"])
def test_exact_cull(checker, name):
    s, cam = gs.view(name)
    w, h = 64, 40
    bits, _ = _want_plane(checker, name, w, h)
    c = DeviceContext(DEV)
    try:
        c.upload(s)
        frames = gs.frames(c, cam, w, h, [(3, 1)])
        assert c.cull_info()[0], f"{name} renders without the exact cull"
        c.render_aov_async(cam, abi.make_params(w, h), AOV_ALL)
        _shadow_pass(c, bits, w, h, name)
        assert c.cull_info()[0]
        _relight_and_check(c, w, h, 3, 1, frames[(3, 1)], name)
        # the same scene uploaded again leaves the lights' records to the next launch: this shadow pass builds them
        updates = c.cull_info()[1]
        c.upload(s)
        shadowbuf.poison(c, w * h)
        c.render_shadows_async()
        shadowbuf.check(c, abi.make_params(w, h), 1, bits, f"{name} after an upload")
        assert c.cull_info() == (True, updates), "the shadow pass built camera records, or dropped the cull"
        _relight_and_check(c, w, h, 3, 1, frames[(3, 1)], f"{name} after an upload")
        assert np.array_equal(c.render(cam, abi.make_params(w, h))[0], frames[(3, 1)][0])
    finally:
        c.close()


@pytest.mark.parametrize("T", [300, 1100])
def test_deep_stacks(ctx, checker, T):
    s, cam, keep = deep_scene(T)
    w, h = 64, 40
    bits, hit = relight_ref.plane(checker, s, cam, w, h)
    ctx.upload(s)
    frames = gs.frames(ctx, cam, w, h, [(0, 1), (3, 1)])
    ctx.render_aov_async(cam, abi.make_params(w, h), AOV_ALL)
    _shadow_pass(ctx, bits, w, h, f"chain of {T}")
    for cfg in ((0, 1), (3, 1)):
        _relight_and_check(ctx, w, h, *cfg, frames[cfg], f"chain of {T} {cfg}")
    rpx, _ = oracle_bind.render(s, cam, abi.make_params(w, h, 0, 1))
    assert np.array_equal(frames[(0, 1)][0], rpx)
    del keep


# ---- 5. views and stripes ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("first", [0, 1])
def test_views_and_stripes(ctx, checker, first):
    s, cam = gs.view("W4_Bunny")
    w, h, nv = 40, 32, 3
    n = w * h
    cams = gs.cams3(cam)
    arr = (abi.Camera * nv)(*cams)
    p = abi.make_params(w, h, 3, 1, abi.XRGB8888, 16, first, 2)
    want_bits = [relight_ref.plane(checker, s, cv, w, h)[0] for cv in cams]
    ctx.upload(s)
    sent_px, sent_rgb, sent_bits = np.uint32(0xABCDEF01), np.float32(-7.5), np.uint32(0x5A5A5A5A)

    def gather():
        px, rgb = np.full(nv * n, sent_px, np.uint32), np.full(3 * nv * n, sent_rgb, np.float32)
        ctx.gather_async(px, rgb)
        ctx.synchronize()
        return px, rgb

    abi.check(ctx.lib.rtx_render_views_async(ctx.h, arr, nv, C.byref(p), 1), "rtx_render_views_async", ctx.h)
    want = gather()
    ctx.render_aov_async(cams, p, AOV_ALL)
    _shadow_pass(ctx, want_bits, w, h, f"3 views, first {first}", n_views=nv, shape=p)
    _relight_and_check(ctx, w, h, 3, 1, want, f"3 views, first {first}", n_views=nv, shape=p)
    got = gather()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    # the plane's copies are full-frame and write owned rows only
    bits = np.full(nv * n, sent_bits, np.uint32)
    ctx.gather_shadows_async(bits)
    ctx.synchronize()
    assert np.array_equal(bits, ctx.download_shadows(np.full(nv * n, sent_bits, np.uint32)))
    for v in range(nv):
        own = devbuf.owned_rows(p, v)
        assert own.any() and not own.all()
        rows = got[0][v * n:(v + 1) * n].reshape(h, w)
        assert (rows[~own] == sent_px).all() and not (rows[own] == sent_px).any()
        crow = got[1][3 * v * n:3 * (v + 1) * n].reshape(h, 3 * w)
        assert (crow[~own] == sent_rgb).all() and not (crow[own] == sent_rgb).any()
        brow = bits[v * n:(v + 1) * n].reshape(h, w)
        assert (brow[~own] == sent_bits).all() and np.array_equal(brow[own], want_bits[v].reshape(h, w)[own])
    # views 0 and 2 own the same rows and differ there, in the frame and in the plane
    own = devbuf.owned_rows(p, 0)
    assert np.array_equal(own, devbuf.owned_rows(p, 2))
    assert not np.array_equal(got[0][:n].reshape(h, w)[own], got[0][2 * n:].reshape(h, w)[own])
    assert not np.array_equal(bits[:n].reshape(h, w)[own], bits[2 * n:].reshape(h, w)[own])


# ---- 6. the light limit -----------------------------------------------------------------------------------------

def test_32_lights_and_the_refusal_of_33(checker, tmp_path):
    c = DeviceContext(DEV)
    p = abi.make_params(W, H)
    try:
        hs = gs.file_scene(tmp_path, "lights32", MATS, gs.many_lights(32))
        s, cam = hs.view()
        assert s.n_lights == 32
        bits, hit = relight_ref.plane(checker, s, cam, W, H)
        top = (bits >> np.uint32(31))[hit]
        assert top.any() and not top.all(), "light 31 decides nothing in the checker's plane"
        c.upload(s)
        frames = gs.frames(c, cam, W, H, [(3, 1), (1, 1), (0, 0)])
        c.render_aov_async(cam, p, AOV_ALL)
        c.render_shadows_async()
        got = c.download_shadows()
        assert np.array_equal(got, bits), int((got != bits).sum())
        for cfg, want in frames.items():
            _relight_and_check(c, W, H, *cfg, want, f"32 lights {cfg}")
        hs33 = gs.file_scene(tmp_path, "lights33", MATS, gs.many_lights(33))
        s33, _ = hs33.view()
        assert s33.n_lights == 33
        c.upload(s33)
        assert c.lib.rtx_render_shadows_async(c.h) == abi.RTX_E_UNSUPPORTED
        assert b"32" in c.lib.rtx_last_error(c.h)
        assert c.lib.rtx_relight_async(c.h, C.byref(p), 0) == abi.RTX_E_STATE   # (the plane is 32 lights')
        px, rgb = c.render(cam, p)
        rpx, rrgb = oracle_bind.render(s33, cam, p)
        assert np.array_equal(px, rpx) and np.array_equal(rgb.view(np.uint32), rrgb.view(np.uint32))
        _relit_equals_a_fresh_render(c, cam, 3, 0, "33 lights, shadows off")
    finally:
        c.close()


# ---- 7. isolation ---------------------------------------------------------------------------------------------------

def test_isolation_and_records():
    s, cam = gs.view("W4_Bunny")
    n = W * H
    c = DeviceContext(DEV)
    try:
        c.upload(s)
        frames = gs.frames(c, cam, W, H, [(3, 1), (0, 0)])
        big = c.render(cam, abi.make_params(64, 48))   # the last colour frame: 64 x 48, variant 0
        spec, split = c.spec_info(), c.split_info()
        assert spec[1] == 0
        before = c.render_aov(cam, abi.make_params(W, H), AOV_ALL)
        # the shadow pass writes no word of the colour frame buffer
        devbuf.poison(c, 64 * 48, rgb=True)
        c.render_shadows_async()
        gpx, grgb = devbuf.peek(c, 64 * 48, rgb=True)
        assert (gpx == devbuf.PX_SENTINEL).all() and (grgb == devbuf.RGB_SENTINEL).all()
        _relight_and_check(c, W, H, 0, 0, frames[(0, 0)], "ObservedArea after a Combined frame")
        _relight_and_check(c, W, H, 3, 1, frames[(3, 1)], "Combined")
        # the planes and their record are read only; the frames' records of the variant and the split are untouched
        after = c.download_aov(aov_host_planes(W, H, AOV_ALL))
        assert not aov_ref.diff(after, before)
        assert c.spec_info() == spec and c.split_info() == split
        # the last-frame record is the pass's shape: rtx_download gives the 37 x 23 relit frame
        px, rgb = np.zeros(n, np.uint32), np.zeros(3 * n, np.float32)
        abi.check(c.lib.rtx_download(c.h, px.ctypes.data_as(UP), rgb.ctypes.data_as(FP)), "rtx_download", c.h)
        assert aov_ref.same(px, frames[(3, 1)][0]) and aov_ref.same(rgb, frames[(3, 1)][1])
        assert big[0].size == 64 * 48
        # want_rgb = 0, then a colour download
        devbuf.poison(c, n)
        abi.check(c.lib.rtx_relight_async(c.h, C.byref(abi.make_params(W, H, 0, 0)), 0), "rtx_relight_async", c.h)
        assert c.lib.rtx_download(c.h, px.ctypes.data_as(UP), rgb.ctypes.data_as(FP)) == abi.RTX_E_STATE
        abi.check(c.lib.rtx_download(c.h, px.ctypes.data_as(UP), None), "rtx_download", c.h)
        assert aov_ref.same(px, frames[(0, 0)][0])
        # a relight queued between two frames of different cameras changes neither
        cam_b = gs.cams3(cam)[1]
        p = abi.make_params(W, H)
        want_a, want_b = c.render(cam, p), c.render(cam_b, p)
        assert not np.array_equal(want_a[0], want_b[0])
        got = [(np.zeros(n, np.uint32), np.zeros(3 * n, np.float32)) for _ in range(3)]
        c.render_async(cam, p, True)
        c.gather_async(*got[0])
        c.relight_async(abi.make_params(W, H, 3, 1), True)
        c.gather_async(*got[1])
        c.render_async(cam_b, p, True)
        c.gather_async(*got[2])
        c.synchronize()
        assert aov_ref.same(got[0][0], want_a[0]) and aov_ref.same(got[0][1], want_a[1])
        assert aov_ref.same(got[1][0], frames[(3, 1)][0]) and aov_ref.same(got[1][1], frames[(3, 1)][1])
        assert aov_ref.same(got[2][0], want_b[0]) and aov_ref.same(got[2][1], want_b[1])
    finally:
        c.close()


# ---- 8. the error table ---------------------------------------------------------------------------------------------

def test_error_table(tmp_path):
    s, cam = gs.view("W4_Bunny")
    p = abi.make_params(W, H)
    off = abi.make_params(W, H, 3, 0)
    px = np.zeros(W * H, np.uint32)
    ms = C.c_float()
    c = DeviceContext(DEV)
    lib = c.lib

    def relight_rc(q, want_rgb=1):
        return lib.rtx_relight_async(c.h, C.byref(q) if q is not None else None, want_rgb)

    try:
        d = C.POINTER(C.c_uint32)()
        assert lib.rtx_device_shadow_buffer(c.h, None) == abi.RTX_E_INVALID
        assert lib.rtx_device_shadow_buffer(c.h, C.byref(d)) == abi.RTX_OK and not d   # no plane yet
        for rc in (lib.rtx_render_shadows_async(c.h), relight_rc(p), relight_rc(off)):
            assert rc == abi.RTX_E_STATE                                # no scene
        c.upload(s)
        for rc in (lib.rtx_render_shadows_async(c.h), relight_rc(p), relight_rc(off)):
            assert rc == abi.RTX_E_STATE                                # no hit pass yet
        assert b"pass" in lib.rtx_last_error(c.h)
        assert lib.rtx_download_shadows(c.h, px.ctypes.data_as(UP)) == abi.RTX_E_STATE
        gs.renders_correctly(c, s, cam, W, H)
        assert relight_rc(None) == abi.RTX_E_INVALID
        assert lib.rtx_relight(c.h, C.byref(p), None, None) == abi.RTX_E_INVALID
        assert lib.rtx_download_shadows(c.h, None) == abi.RTX_E_INVALID
        assert lib.rtx_gather_shadows_async(c.h, None) == abi.RTX_E_INVALID
        c.render_aov(cam, p, AOV_DEPTH)
        for rc in (lib.rtx_render_shadows_async(c.h), relight_rc(p), relight_rc(off)):
            assert rc == abi.RTX_E_STATE                                # not all four planes
        gs.renders_correctly(c, s, cam, W, H)
        c.render_aov(cam, p, AOV_ALL)
        assert relight_rc(p) == abi.RTX_E_STATE                         # shadows on, no shadow pass yet
        assert b"shadow pass" in lib.rtx_last_error(c.h)
        assert lib.rtx_download_shadows(c.h, px.ctypes.data_as(UP)) == abi.RTX_E_STATE
        assert lib.rtx_gather_shadows_async(c.h, px.ctypes.data_as(UP)) == abi.RTX_E_STATE
        want_off = c.render(cam, off)
        _relight_and_check(c, W, H, 3, 0, want_off, "shadows off needs no shadow pass")
        for bad in (abi.make_params(W, H, 4), abi.make_params(W, H, -1), abi.make_params(W, H, 3, 1, (25, 8, 0, 0))):
            assert relight_rc(bad) == abi.RTX_E_INVALID                 # what rtx_render rejects
            assert lib.rtx_render_async(c.h, C.byref(cam), C.byref(bad), 0) == abi.RTX_E_INVALID
        gs.renders_correctly(c, s, cam, W, H)
        c.set_supersample(2)
        assert lib.rtx_render_shadows_async(c.h) == abi.RTX_E_UNSUPPORTED
        assert relight_rc(off) == abi.RTX_E_UNSUPPORTED
        c.set_supersample(1)
        gs.renders_correctly(c, s, cam, W, H)
        # a scene with fewer materials than the pass's: refused on the host, as by rtx_shade_aov
        four = gs.file_scene(tmp_path, "four_materials", MATS[:3], LIGHTS)
        s4, cam4 = four.view()
        full = gs.file_scene(tmp_path, "five_materials", MATS, LIGHTS)
        s5, cam5 = full.view()
        c.upload(s5)
        c.render_aov(cam5, p, AOV_ALL)
        c.upload(s4)
        assert relight_rc(off) == abi.RTX_E_STATE
        gs.renders_correctly(c, s4, cam4, W, H)
        # and it still works
        c.upload(s)
        c.render_aov(cam, p, AOV_ALL)
        want = c.render(cam, p)
        abi.check(lib.rtx_render_shadows_async(c.h), "rtx_render_shadows_async", c.h)
        devbuf.poison(c, W * H)
        assert lib.rtx_relight(c.h, C.byref(p), px.ctypes.data_as(UP), None) == abi.RTX_OK
        assert np.array_equal(px, want[0])
        assert lib.rtx_device_shadow_buffer(c.h, C.byref(d)) == abi.RTX_OK and d
        assert lib.rtx_time_shadows(c.h, 0, C.byref(ms)) == abi.RTX_E_INVALID
        assert lib.rtx_time_shadows(c.h, 1, None) == abi.RTX_E_INVALID
        assert lib.rtx_time_relight(c.h, C.byref(p), 0, 0, C.byref(ms)) == abi.RTX_E_INVALID
        assert c.time_shadows(2) > 0.0 and c.time_relight(p, False, 2) > 0.0
        assert np.array_equal(c.relight(p, False)[0], want[0])           # the timed passes left valid state
    finally:
        c.close()


# ---- 9. the Python Renderer and the CLI -----------------------------------------------------------------------------

def test_renderer_relight_follows_mode_and_shadows(checker):
    hs = HostScene("W4_Bunny")
    r = Renderer(W, H, DEV)
    try:
        with pytest.raises(RuntimeError):
            r.RenderShadows()   # no pass yet
        with pytest.raises(RuntimeError):
            r.Relight()
        r.Render(hs, want_rgb=True)   # (the frame buffer and its colour plane exist: they can be poisoned)
        r.RenderAOV(hs, upload=False)
        bits = r.RenderShadows()
        assert np.array_equal(bits, _want_plane(checker, "W4_Bunny", W, H)[0])
        seen = set()
        for _ in range(4):
            r.CycleLightingMode()
            for _ in range(2):
                r.ToggleShadows()
                devbuf.poison(r.ctx, W * H, rgb=True)
                got = r.Relight(want_rgb=True).copy()
                got_rgb = r.rgb.copy()
                want = r.Render(hs, upload=False, want_rgb=True)
                assert aov_ref.same(got, want) and aov_ref.same(got_rgb, r.rgb), (r.m_CurrentLightingMode, r.m_ShadowsEnabled)
                seen.add((r.m_CurrentLightingMode, r.m_ShadowsEnabled, got.tobytes()))
        assert len(seen) == 8 and len({x[2] for x in seen}) >= 6
    finally:
        r.ctx.close()


def test_cli_relight_writes_the_plain_runs_files(checker, tmp_path):
    assert EXE.exists(), "lib/rtx_render is not built"
    planes = ("_depth.f32", "_normal.f32", "_material.u32", "_primitive.u32")

    def run(*args):
        subprocess.run([str(EXE), "W4_Optional", "61", "45", *args], check=True, cwd=tmp_path, timeout=120)

    run("--out", "plain.bmp", "--aov", "plain")
    run("--out", "relight.bmp", "--aov", "relight", "--relight")
    run("--out", "relight_only.bmp", "--relight")
    run("--out", "plain_m0.bmp", "--mode", "0", "--no-shadows")
    run("--out", "relight_m0.bmp", "--mode", "0", "--no-shadows", "--relight")
    want = (tmp_path / "plain.bmp").read_bytes()
    assert len(want) == 54 + 4 * 61 * 45
    assert (tmp_path / "relight.bmp").read_bytes() == want and (tmp_path / "relight_only.bmp").read_bytes() == want
    for k in planes:
        assert (tmp_path / f"relight{k}").read_bytes() == (tmp_path / f"plain{k}").read_bytes(), k
    bits = np.fromfile(tmp_path / "relight_shadow.u32", np.uint32)
    assert np.array_equal(bits, _want_plane(checker, "W4_Optional", 61, 45)[0])
    m0 = (tmp_path / "plain_m0.bmp").read_bytes()
    assert (tmp_path / "relight_m0.bmp").read_bytes() == m0 and m0 != want
    assert not list(tmp_path.glob("relight_only_*")) and not (tmp_path / "plain_shadow.u32").exists()
