"""Deferred shading (rtx_shade_aov*, PHASE 8 of the render kernel) on the GPU: the shaded hit pass equals the
colour frame of the same parameters word for word in both planes, in every specialised variant and the
generic kernel, with the room skip, the exact cull and the deep stacks, for views and stripes, after relight
uploads, beside the frames and the planes it must not disturb, on its error paths, through the Python
Renderer and the CLI.  The frame buffer is poisoned (tests/devbuf.py) before every shade that follows a frame
of its size (all but a context's first launches and the shade queued between two frames), so every owned pixel
is proved written and no other word touched."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import aov_ref
import devbuf
import gpu_support as gs
import oracle_bind
from gp1_raytracer_2223_amd import abi
from gp1_raytracer_2223_amd.renderer import AOV_ALL, AOV_DEPTH, DeviceContext, Renderer, aov_host_planes
from gp1_raytracer_2223_amd.scene import HostScene
from gpu_support import CONFIGS, DEV, FP, LIGHTS, MATS, POW_FREE_MODES, UP
from gpu_support import ctx  # noqa: F401
from test_gpu_deep_bvh import deep_scene

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
EXE = ROOT / "gp1_raytracer_2223_amd" / "lib" / "rtx_render"
W, H = 37, 23   # five tile columns and three tile rows, one of each partial


def _shade_rc(c, p, want_rgb=1):
    return c.lib.rtx_shade_aov_async(c.h, C.byref(p) if p is not None else None, want_rgb)


def _shade_and_check(c, w, h, mode, sh, want, what, n_views=1, shape=None):
    """Poison, shade the last pass with (mode, sh), and demand the frame `want` in every owned word."""
    devbuf.poison(c, n_views * w * h, rgb=True)
    # the size and stripe fields of the shade's parameters are ignored: the pass supplies them
    c.shade_aov_async(abi.make_params(1, 1, mode, sh), True)
    devbuf.check(c, shape if shape is not None else abi.make_params(w, h, mode, sh), n_views, want[0], want[1], what)


def _equals_the_frame(c, name, w, h, seen, oracle_all_modes=False):
    s, cam = gs.view(name)
    c.upload(s)
    frames = gs.frames(c, cam, w, h, CONFIGS, seen)
    room = c.room_info()[0]
    c.render_aov_async(cam, abi.make_params(w, h), AOV_ALL)
    for (mode, sh), want in frames.items():
        _shade_and_check(c, w, h, mode, sh, want, f"{name} {w}x{h} mode {mode} shadows {sh}")
        if oracle_all_modes or mode in POW_FREE_MODES:
            gpx, grgb = devbuf.peek(c, w * h, rgb=True)
            rpx, rrgb = oracle_bind.render(s, cam, abi.make_params(w, h, mode, sh))
            assert np.array_equal(gpx, rpx), (name, mode, sh)
            assert np.array_equal(grgb, rrgb.view(np.uint32)), (name, mode, sh)
    # the blocking call, through the contract's comparison
    devbuf.poison(c, w * h, rgb=True)
    px, rgb = c.shade_aov(abi.make_params(w, h), True)
    assert aov_ref.same(px, frames[(3, 1)][0]) and aov_ref.same(rgb, frames[(3, 1)][1]), name
    return room


# ---- 1. equals the frame --------------------------------------------------------------------------

EQUAL = ["W4_Bunny", "W4_Optional", "W3", "W4_Reference", "W1", "fuzz:room0_0"]
_seen = {}   # scene -> the variants its comparison frames took


@pytest.mark.parametrize("name", EQUAL)
def test_equals_the_frame(ctx, name):
    seen = set()
    room = _equals_the_frame(ctx, name, W, H, seen, oracle_all_modes=name == "W4_Bunny")
    _seen[name] = seen
    if name == "W4_Bunny":
        assert room, "W4_Bunny renders with the room skip"


@pytest.mark.parametrize("w,h", [(1, 1), (8, 8)])
def test_equals_the_frame_at_one_pixel_and_one_tile(ctx, w, h):
    _equals_the_frame(ctx, "W4_Bunny", w, h, set(), oracle_all_modes=True)


def test_the_scenes_covered_every_variant(ctx):
    for name in EQUAL:   # (those a selection left out)
        if name not in _seen:
            _seen[name] = set()
            _equals_the_frame(ctx, name, W, H, _seen[name])
    got = set().union(*_seen.values())
    assert got >= {-1, 0, 1, 2, 3}, {k: sorted(v) for k, v in _seen.items()}


# ---- 2. the exact cull ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["Synthetic100k", "W4_Optional"])
def test_exact_cull(name):
    s, cam = gs.view(name)
    w, h = 64, 40
    c = DeviceContext(DEV)
    try:
        c.upload(s)
        frames = gs.frames(c, cam, w, h, [(3, 1)])
        assert c.cull_info()[0], f"{name} renders without the exact cull"
        c.render_aov_async(cam, abi.make_params(w, h), AOV_ALL)
        _shade_and_check(c, w, h, 3, 1, frames[(3, 1)], name)
        assert c.cull_info()[0]
        # the same scene uploaded again leaves the lights' records to the next launch: this shade builds them
        updates = c.cull_info()[1]
        c.upload(s)
        _shade_and_check(c, w, h, 3, 1, frames[(3, 1)], f"{name} after an upload")
        assert c.cull_info() == (True, updates), "the shade built camera records, or dropped the cull"
        assert np.array_equal(c.render(cam, abi.make_params(w, h))[0], frames[(3, 1)][0])
    finally:
        c.close()


# ---- 3. the deep stacks -----------------------------------------------------------------------------

@pytest.mark.parametrize("T", [300, 1100])
def test_deep_stacks(ctx, T):
    s, cam, keep = deep_scene(T)
    w, h = 64, 40
    ctx.upload(s)
    frames = gs.frames(ctx, cam, w, h, [(0, 1)])
    assert (frames[(0, 1)][0] != frames[(0, 1)][0][0]).any()
    ctx.render_aov_async(cam, abi.make_params(w, h), AOV_ALL)
    _shade_and_check(ctx, w, h, 0, 1, frames[(0, 1)], f"chain of {T}")
    rpx, rrgb = oracle_bind.render(s, cam, abi.make_params(w, h, 0, 1))
    assert np.array_equal(frames[(0, 1)][0], rpx)
    del keep


# ---- 4. views and stripes -----------------------------------------------------------------------------

@pytest.mark.parametrize("first", [0, 1])
def test_views_and_stripes(ctx, first):
    s, cam = gs.view("W4_Bunny")
    w, h, nv = 40, 32, 3
    n = w * h
    cams = gs.cams3(cam)
    arr = (abi.Camera * nv)(*cams)
    p = abi.make_params(w, h, 3, 1, abi.XRGB8888, 16, first, 2)
    ctx.upload(s)
    sent_px, sent_rgb = np.uint32(0xABCDEF01), np.float32(-7.5)

    def gather():
        px, rgb = np.full(nv * n, sent_px, np.uint32), np.full(3 * nv * n, sent_rgb, np.float32)
        ctx.gather_async(px, rgb)
        ctx.synchronize()
        return px, rgb

    abi.check(ctx.lib.rtx_render_views_async(ctx.h, arr, nv, C.byref(p), 1), "rtx_render_views_async", ctx.h)
    want = gather()
    ctx.render_aov_async(cams, p, AOV_ALL)
    _shade_and_check(ctx, w, h, 3, 1, want, f"3 views, first {first}", n_views=nv, shape=p)
    got = gather()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    for v in range(nv):
        own = devbuf.owned_rows(p, v)
        assert own.any() and not own.all()
        rows = got[0][v * n:(v + 1) * n].reshape(h, w)
        assert (rows[~own] == sent_px).all() and not (rows[own] == sent_px).any()
        crow = got[1][3 * v * n:3 * (v + 1) * n].reshape(h, 3 * w)
        assert (crow[~own] == sent_rgb).all() and not (crow[own] == sent_rgb).any()
    # views 0 and 2 own the same rows and differ there: a shade with one camera for all of them would not pass
    own = devbuf.owned_rows(p, 0)
    assert np.array_equal(own, devbuf.owned_rows(p, 2))
    assert not np.array_equal(got[0][:n].reshape(h, w)[own], got[0][2 * n:].reshape(h, w)[own])


# ---- 5. relight ---------------------------------------------------------------------------------------

# name -> (materials, lights, the variant and the room fact its frames take)
RELIGHT = {
    "moved_recoloured": (MATS, ["light point 1.5 6 3  60 0.4 0.7 1", LIGHTS[1]], 0, True),
    "one_more_light": (MATS, LIGHTS + ["light point 3 2 -3  40 0.6 0.8 1"], 0, True),
    "directional_added": (MATS, LIGHTS + ["light directional 0 -1 0.5  1.5 1 1 0.9"], -1, None),
    "light_outside_room": (MATS, LIGHTS + ["light point 6.5 4 3  60 0.6 0.8 1"], 0, False),
    "lambert_to_cook_torrance": ([MATS[0], "material cook_torrance 0.95 0.93 0.88 1 0.3", MATS[2], MATS[3]], LIGHTS, 1, True),
}


def test_relight(tmp_path):
    c = DeviceContext(DEV)
    try:
        base = gs.file_scene(tmp_path, "base", MATS, LIGHTS)
        s, cam = base.view()
        assert s.n_materials == 5
        c.upload(s)
        frames = gs.frames(c, cam, W, H, CONFIGS)
        assert c.spec_info()[1] == 0 and c.room_info()[0]
        c.render_aov_async(cam, abi.make_params(W, H), AOV_ALL)
        for (mode, sh), want in frames.items():   # one pass: every mode and shadow toggle
            _shade_and_check(c, W, H, mode, sh, want, f"base mode {mode} shadows {sh}")
        for name, (mats, lights, variant, room) in RELIGHT.items():
            hs = gs.file_scene(tmp_path, name, mats, lights)
            s2, cam2 = hs.view()
            assert s2.n_materials == 5 and bytes(cam2) == bytes(cam)
            c.upload(s2)   # the same geometry and material indices: no new pass
            for mode, sh in ((3, 1), (2, 0)):
                devbuf.poison(c, W * H, rgb=True)
                c.shade_aov_async(abi.make_params(W, H, mode, sh), True)
                got = devbuf.peek(c, W * H, rgb=True)
                want = c.render(cam, abi.make_params(W, H, mode, sh))
                assert np.array_equal(got[0], want[0]), (name, mode, sh, int((got[0] != want[0]).sum()))
                assert np.array_equal(got[1], want[1].view(np.uint32)), (name, mode, sh)
                if (mode, sh) == (3, 1):
                    assert c.spec_info()[1] == variant, (name, c.spec_info())
                    assert not np.array_equal(want[0], frames[(3, 1)][0]), f"{name}: the relight changes nothing"
            if room is not None:
                assert c.room_info()[0] == room, name
        # a scene with fewer materials than the pass's: refused on the host
        four = gs.file_scene(tmp_path, "four_materials", MATS[:3], LIGHTS)
        s4, _ = four.view()
        assert s4.n_materials == 4
        c.upload(s4)
        assert _shade_rc(c, abi.make_params(W, H)) == abi.RTX_E_STATE
        px, rgb = c.render(cam, abi.make_params(W, H))
        rpx, rrgb = oracle_bind.render(s4, cam, abi.make_params(W, H))
        assert np.array_equal(px, rpx) and np.array_equal(rgb.view(np.uint32), rrgb.view(np.uint32))
    finally:
        c.close()


# ---- 6. isolation and records ---------------------------------------------------------------------------

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
        _shade_and_check(c, W, H, 0, 0, frames[(0, 0)], "ObservedArea after a Combined frame")
        # the planes and their record are read only; the frames' records of the variant and the split are untouched
        after = c.download_aov(aov_host_planes(W, H, AOV_ALL))
        assert not aov_ref.diff(after, before)
        assert c.spec_info() == spec and c.split_info() == split
        # the last-frame record is the pass's shape: rtx_download gives the 37 x 23 shaded frame
        px, rgb = np.zeros(n, np.uint32), np.zeros(3 * n, np.float32)
        abi.check(c.lib.rtx_download(c.h, px.ctypes.data_as(UP), rgb.ctypes.data_as(FP)), "rtx_download", c.h)
        assert aov_ref.same(px, frames[(0, 0)][0]) and aov_ref.same(rgb, frames[(0, 0)][1])
        assert big[0].size == 64 * 48
        # want_rgb = 0, then a colour download
        devbuf.poison(c, n)
        abi.check(_shade_rc(c, abi.make_params(W, H), 0), "rtx_shade_aov_async", c.h)
        assert c.lib.rtx_download(c.h, px.ctypes.data_as(UP), rgb.ctypes.data_as(FP)) == abi.RTX_E_STATE
        abi.check(c.lib.rtx_download(c.h, px.ctypes.data_as(UP), None), "rtx_download", c.h)
        assert aov_ref.same(px, frames[(3, 1)][0])
        # a shade queued between two frames of different cameras changes neither
        cam_b = gs.cams3(cam)[1]
        p = abi.make_params(W, H)
        want_a, want_b = c.render(cam, p), c.render(cam_b, p)
        assert not np.array_equal(want_a[0], want_b[0])
        got = [(np.zeros(n, np.uint32), np.zeros(3 * n, np.float32)) for _ in range(3)]
        c.render_async(cam, p, True)
        c.gather_async(*got[0])
        c.shade_aov_async(abi.make_params(W, H, 0, 0), True)
        c.gather_async(*got[1])
        c.render_async(cam_b, p, True)
        c.gather_async(*got[2])
        c.synchronize()
        assert aov_ref.same(got[0][0], want_a[0]) and aov_ref.same(got[0][1], want_a[1])
        assert aov_ref.same(got[1][0], frames[(0, 0)][0]) and aov_ref.same(got[1][1], frames[(0, 0)][1])
        assert aov_ref.same(got[2][0], want_b[0]) and aov_ref.same(got[2][1], want_b[1])
    finally:
        c.close()


def test_the_dispatch_order_changes_no_pixel():
    """The shade reads the dispatch order of the context's last frames when they had its tile set: before any
    frame (tile order), after frames of another size, after frames of its size, and on a context without
    cost-ordered dispatch, the same words."""
    s, cam = gs.view("W4_Bunny")
    w, h = 96, 64
    n = w * h
    p = abi.make_params(w, h)
    os.environ["RTX_TILE_ORDER"] = "0"
    try:
        plain = DeviceContext(DEV)
    finally:
        del os.environ["RTX_TILE_ORDER"]
    c = DeviceContext(DEV)
    try:
        got = []
        for x in (c, plain):
            x.upload(s)
            x.render_aov_async(cam, p, AOV_ALL)
            got.append(x.shade_aov(p, True))               # no frame yet: tile order
        c.render(cam, abi.make_params(W, H))
        devbuf.poison(c, n, rgb=True)
        got.append(c.shade_aov(p, True))                    # the frames' order is another tile set's
        want = c.render(cam, p)
        for _ in range(3):
            c.render(cam, p)                                # (the measured frame's order is adopted)
        devbuf.poison(c, n, rgb=True)
        c.shade_aov_async(p, True)
        devbuf.check(c, p, 1, want[0], want[1], "in the frames' order")
        for px, rgb in got:
            assert aov_ref.same(px, want[0]) and aov_ref.same(rgb, want[1])
        assert aov_ref.same(plain.render(cam, p)[0], want[0])
    finally:
        c.close()
        plain.close()


# ---- 7. the error table -----------------------------------------------------------------------------------

def test_error_table():
    s, cam = gs.view("W4_Bunny")
    p = abi.make_params(W, H)
    px = np.zeros(W * H, np.uint32)
    c = DeviceContext(DEV)
    try:
        assert _shade_rc(c, p) == abi.RTX_E_STATE                     # no scene
        c.upload(s)
        assert _shade_rc(c, p) == abi.RTX_E_STATE                     # no pass yet
        assert b"pass" in c.lib.rtx_last_error(c.h)
        gs.renders_correctly(c, s, cam, W, H)
        assert _shade_rc(c, None) == abi.RTX_E_INVALID
        assert c.lib.rtx_shade_aov(c.h, C.byref(p), None, None) == abi.RTX_E_INVALID
        c.render_aov(cam, p, AOV_DEPTH)
        assert _shade_rc(c, p) == abi.RTX_E_STATE                     # not all four planes
        gs.renders_correctly(c, s, cam, W, H)
        c.render_aov(cam, p, AOV_ALL)
        for bad in (abi.make_params(W, H, 4), abi.make_params(W, H, -1), abi.make_params(W, H, 3, 1, (25, 8, 0, 0))):
            assert _shade_rc(c, bad) == abi.RTX_E_INVALID             # what rtx_render rejects
            assert c.lib.rtx_render_async(c.h, C.byref(cam), C.byref(bad), 0) == abi.RTX_E_INVALID
        gs.renders_correctly(c, s, cam, W, H)
        c.set_supersample(2)
        assert _shade_rc(c, p) == abi.RTX_E_UNSUPPORTED
        c.set_supersample(1)
        gs.renders_correctly(c, s, cam, W, H)
        want = c.render(cam, p)
        devbuf.poison(c, W * H)
        assert c.lib.rtx_shade_aov(c.h, C.byref(p), px.ctypes.data_as(UP), None) == abi.RTX_OK   # and it still shades
        assert np.array_equal(px, want[0])
        ms = C.c_float()
        assert c.lib.rtx_time_shade_aov(c.h, C.byref(p), 0, 0, C.byref(ms)) == abi.RTX_E_INVALID
        assert c.time_shade_aov(p, False, 2) > 0.0
    finally:
        c.close()


# ---- 8. the Python Renderer -------------------------------------------------------------------------------

def test_renderer_shade_aov_follows_mode_and_shadows():
    hs = HostScene("W4_Bunny")
    r = Renderer(W, H, DEV)
    try:
        with pytest.raises(RuntimeError):
            r.ShadeAOV()   # no pass yet
        r.Render(hs, want_rgb=True)   # (the frame buffer and its colour plane exist: they can be poisoned)
        r.RenderAOV(hs, upload=False)
        seen = set()
        for _ in range(4):
            r.CycleLightingMode()
            for _ in range(2):
                r.ToggleShadows()
                devbuf.poison(r.ctx, W * H, rgb=True)
                got = r.ShadeAOV(want_rgb=True).copy()
                got_rgb = r.rgb.copy()
                want = r.Render(hs, upload=False, want_rgb=True)
                assert aov_ref.same(got, want) and aov_ref.same(got_rgb, r.rgb), (r.m_CurrentLightingMode, r.m_ShadowsEnabled)
                seen.add((r.m_CurrentLightingMode, r.m_ShadowsEnabled, got.tobytes()))
        assert len(seen) == 8 and len({x[2] for x in seen}) >= 6
    finally:
        r.ctx.close()


# ---- 9. the CLI ---------------------------------------------------------------------------------------------

def test_cli_deferred_writes_the_plain_runs_files(tmp_path):
    assert EXE.exists(), "lib/rtx_render is not built"
    planes = ("_depth.f32", "_normal.f32", "_material.u32", "_primitive.u32")

    def run(*args):
        subprocess.run([str(EXE), "W4_Optional", "61", "45", *args], check=True, cwd=tmp_path, timeout=120)

    run("--out", "plain.bmp", "--aov", "plain")
    run("--out", "deferred.bmp", "--aov", "deferred", "--deferred")
    run("--out", "deferred_only.bmp", "--deferred")
    run("--out", "plain_m0.bmp", "--mode", "0", "--no-shadows")
    run("--out", "deferred_m0.bmp", "--mode", "0", "--no-shadows", "--deferred")
    want = (tmp_path / "plain.bmp").read_bytes()
    assert len(want) == 54 + 4 * 61 * 45
    assert (tmp_path / "deferred.bmp").read_bytes() == want and (tmp_path / "deferred_only.bmp").read_bytes() == want
    for k in planes:
        assert (tmp_path / f"deferred{k}").read_bytes() == (tmp_path / f"plain{k}").read_bytes(), k
    m0 = (tmp_path / "plain_m0.bmp").read_bytes()
    assert (tmp_path / "deferred_m0.bmp").read_bytes() == m0 and m0 != want
    assert not list(tmp_path.glob("deferred_only_*"))
