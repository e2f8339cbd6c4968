"""The incremental shadow pass (rtx_update_shadows_async, rtx_refresh_shadows_async: PHASE 9 of the render kernel
under a trace mask and a keep mask) on the GPU.

Every update under test runs on a FORGED plane (tests/shadowforge.py): random words in the rows the pass owns, a
sentinel elsewhere.  Afterwards every owned word must be (F & keep) | (want & trace), `want` being the CPU
checker's plane (tests/relight_ref.py) of the scene uploaded now, and every other word untouched.  That one
comparison proves the traced bits rewritten in every owned pixel, the kept bits carried verbatim, the other bits
cleared and nothing else written.  The relights that follow run on a true plane (a full pass of the old lights,
then the update unforged) and equal a fresh render word for word.

Each test asserts from the checker's planes that its edit changes the bits it should (> 0 words) and no other."""
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
import relight_ref
import shadow_update_scenes as sus
import shadowbuf
import shadowforge
from checkers import checker  # noqa: F401
from gp1_raytracer_2223_amd import abi
from gp1_raytracer_2223_amd.renderer import AOV_ALL, AOV_DEPTH, DeviceContext, Renderer, aov_host_planes
from gp1_raytracer_2223_amd.scene import HostScene
from gpu_support import CONFIGS, DEV, POW_FREE_MODES
from gpu_support import ctx  # noqa: F401
from test_gpu_deep_bvh import deep_scene

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
EXE = ROOT / "gp1_raytracer_2223_amd" / "lib" / "rtx_render"
W, H = 37, 23   # five tile columns and three tile rows, one of each partial


@pytest.fixture(scope="module")
def files(tmp_path_factory, checker):
    """(geometry, variant) -> (host scene, scene, camera, the checker's plane at W x H), each computed once."""
    d = tmp_path_factory.mktemp("scenes")
    cache = {}

    def get(geometry, variant):
        if (geometry, variant) not in cache:
            hs = sus.file_scene(d, geometry, variant)
            s, cam = hs.view()
            bits, hit = relight_ref.plane(checker, s, cam, W, H)
            bits.setflags(write=False)
            cache[(geometry, variant)] = (hs, s, cam, bits)
        return cache[(geometry, variant)][1:]
    return get


def _all(s) -> int:
    return (1 << s.n_lights) - 1


def _moved(s, moves: dict):
    """A copy of the flat scene whose light l is moved by moves[l] (binary32 sums); the copy keeps its arrays."""
    arr = (abi.Light * s.n_lights)()
    for l in range(s.n_lights):
        C.memmove(C.byref(arr[l]), C.byref(s.lights[l]), C.sizeof(abi.Light))
    for l, d in moves.items():
        for k in range(3):
            arr[l].origin[k] = np.float32(arr[l].origin[k]) + np.float32(d[k])
    s2 = abi.Scene()
    C.memmove(C.byref(s2), C.byref(s), C.sizeof(abi.Scene))
    s2.lights = arr
    s2._keep = (arr, s)
    return s2


def _assert_changes(old_bits, new_bits, mask: int, what, counts: dict | None = None):
    """The checker's two planes differ in the bits of `mask`, each in at least one word, and in no other bit."""
    changed = sus.changed_per_bit(old_bits, new_bits)
    for l in range(32):
        if (mask >> l) & 1:
            assert changed[l] > 0, f"{what}: the edit changes no word in bit {l}"
        else:
            assert changed[l] == 0, f"{what}: the edit changes {changed[l]} words in bit {l}"
    if counts is not None:
        assert {l: c for l, c in enumerate(changed) if c} == counts, (what, changed)


def _passes(c, s, cam, p, n_views=1):
    """Upload, the hit pass and the full shadow pass."""
    c.upload(s)
    c.render_aov_async(cam, p, AOV_ALL)
    c.render_shadows_async()


def _forged_update(c, p, want, trace, keep, seed, what, n_views=1, sentinel=shadowbuf.SENTINEL):
    """The standard check: forge the plane, update the lights of `trace`, demand (F & keep) | (want & trace)."""
    F = shadowforge.forged(p, n_views, seed, sentinel)
    shadowforge.write(c, F)
    c.update_shadows_async(trace)
    return shadowforge.check(c, p, n_views, F, want, trace, keep, what)


def _relit_equals_a_fresh_render(c, cam, w, h, mode, sh, what):
    want = c.render(cam, abi.make_params(w, h, mode, sh))
    devbuf.poison(c, w * h, rgb=True)
    c.relight_async(abi.make_params(1, 1, mode, sh), True)   # (size and stripes are the pass's)
    devbuf.check(c, abi.make_params(w, h, mode, sh), 1, want[0], want[1], f"{what} mode {mode} shadows {sh}")
    return want


# ---- 1. the update equals the checker -------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ["move0", "move1_out", "move12", "type2"])
@pytest.mark.parametrize("geometry", ["room", "open"])
def test_update_equals_the_checker(ctx, files, geometry, variant):
    c = ctx
    p = abi.make_params(W, H)
    s0, cam, bits0 = files(geometry, "base")
    s1, cam1, bits1 = files(geometry, variant)
    mask = sus.VARIANTS[variant][1]
    assert bytes(cam1) == bytes(cam) and s1.n_lights == s0.n_lights == 3
    assert sus.dirty_mask(sus.light_keys(s0), sus.light_keys(s1)) == mask
    _assert_changes(bits0, bits1, mask, (geometry, variant))
    what = f"{geometry} {variant}"
    _passes(c, s0, cam, p)
    c.upload(s1)
    _forged_update(c, p, bits1, mask, _all(s1) & ~mask, 1, what)
    # a true plane: the base lights' full pass, then the update carries its untraced bits over
    c.upload(s0)
    c.render_shadows_async()
    c.upload(s1)
    assert c.lib.rtx_relight_async(c.h, C.byref(p), 0) == abi.RTX_E_STATE   # (stale until the update)
    c.update_shadows_async(mask)
    assert np.array_equal(shadowbuf.peek(c, W * H), bits1), what
    assert np.array_equal(c.download_shadows(), bits1), what
    for mode, sh in CONFIGS:
        want = _relit_equals_a_fresh_render(c, cam, W, H, mode, sh, what)
        if mode in POW_FREE_MODES:
            rpx, rrgb = oracle_bind.render(s1, cam, abi.make_params(W, H, mode, sh))
            assert np.array_equal(want[0], rpx) and np.array_equal(want[1].view(np.uint32), rrgb.view(np.uint32)), what


# ---- 2. the first traced light is not light 0 -------------------------------------------------------------------

def test_first_traced_light_is_not_light_0(ctx, files):
    """`open` has two planes that are no room: the shadow rays take the plane loop whose numerators the first light
    of the loop stores in LDS for the later ones.  Under a mask without bit 0 the first light is the first TRACED
    one; an update that read the cache before filling it would fail the forged-plane check here."""
    c = ctx
    p = abi.make_params(W, H)
    s0, cam, bits0 = files("open", "base")
    s1, _, bits1 = files("open", "move12")
    _assert_changes(bits0, bits1, 0b110, "open move12")
    _passes(c, s0, cam, p)
    assert not c.room_info()[0]
    c.upload(s1)
    c.update_shadows_async(0b110)   # the record is move12's: any mask is now a legal re-trace
    assert np.array_equal(shadowbuf.peek(c, W * H), bits1)
    for k, mask in enumerate((0b010, 0b100, 0b110)):
        _forged_update(c, p, bits1, mask, 0b111 & ~mask, 10 + k, f"open move12 mask {mask:#b}")
    # re-tracing without a change: the full pass's plane
    _passes(c, s0, cam, p)
    full = shadowbuf.peek(c, W * H)
    assert np.array_equal(full, bits0)
    for k, mask in enumerate((0b001, 0b111)):
        c.update_shadows_async(mask)
        assert np.array_equal(shadowbuf.peek(c, W * H), full), bin(mask)
        _forged_update(c, p, bits0, mask, 0b111 & ~mask, 20 + k, f"open base mask {mask:#b}")
        c.render_shadows_async()


# ---- 3. refresh ---------------------------------------------------------------------------------------------------

def test_refresh(ctx, files):
    c = ctx
    p = abi.make_params(W, H)
    n = W * H
    rng = np.random.default_rng(3)
    s0, cam, bits0 = files("room", "base")
    _passes(c, s0, cam, p)
    recorded, plane = s0, bits0
    assert c.refresh_shadows_async() == 0   # nothing changed yet
    steps = ["move0", "move12", "base", "added", "removed", "removed"]
    expected_traced = {"move0": 0b001, "move12": 0b111, "base": 0b110, "added": 0b1000, "removed": 0}
    for k, name in enumerate(steps):
        s, cam_k, bits = files("room", name)
        assert bytes(cam_k) == bytes(cam)
        old_keys, new_keys = sus.light_keys(recorded), sus.light_keys(s)
        dirty = sus.dirty_mask(old_keys, new_keys)
        assert dirty == expected_traced[name], (name, bin(dirty))
        keep = _all(s) & ~dirty
        clears = recorded.n_lights > s.n_lights
        if dirty or clears:
            _assert_changes(plane, bits, dirty | (_all(recorded) & ~_all(s)), f"step {k} {name}")
        c.upload(s)
        what = f"refresh step {k}: {name}"
        if dirty or clears:
            assert c.lib.rtx_relight_async(c.h, C.byref(p), 0) == abi.RTX_E_STATE, what
            # forged: the true plane in the kept bits, garbage (for a removed light: 1 everywhere) in all others
            junk = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
            if clears:
                junk |= np.uint32(_all(recorded) & ~_all(s))
            F = (plane & np.uint32(keep)) | (junk & np.uint32(~keep & 0xFFFFFFFF))
            shadowforge.write(c, F)
            assert c.refresh_shadows_async() == dirty, what
            got = shadowforge.check(c, p, 1, F, bits, dirty, keep, what)
            assert np.array_equal(got, bits), what
            if name == "added":
                assert ((got >> np.uint32(3)) & 1).any()
            if name == "removed":
                assert not (got >> np.uint32(2)).any()
        else:   # the same scene again: nothing is launched, so a forged plane stays bit for bit
            F = shadowforge.forged(p, 1, 77)
            shadowforge.write(c, F)
            assert c.refresh_shadows_async() == 0, what
            assert np.array_equal(shadowbuf.peek(c, n), F), f"{what}: something was launched"
            shadowforge.write(c, bits)
        _relit_equals_a_fresh_render(c, cam, W, H, 3, 1, what)
        recorded, plane = s, bits
    # a new hit pass: the plane is stale, refresh is the full pass and carries nothing over
    c.render_aov_async(cam, p, AOV_ALL)
    assert c.lib.rtx_update_shadows_async(c.h, 1) == abi.RTX_E_STATE
    F = shadowforge.forged(p, 1, 78)
    shadowforge.write(c, F)
    assert c.refresh_shadows_async() == _all(recorded)
    got = shadowforge.check(c, p, 1, F, plane, _all(recorded), 0, "refresh after a new hit pass")
    assert np.array_equal(got, plane)
    _relit_equals_a_fresh_render(c, cam, W, H, 3, 1, "after the full refresh")


# ---- 4. variants and walks ----------------------------------------------------------------------------------------

def test_room_skip_flips_between_the_passes(ctx, files):
    """move1_out puts L1 at x = 8, outside the wall x = 5: the base pass ran the room-skip variant's kernel with the
    fact true, the update runs with the fact false, and merges into the bits the other wrote."""
    c = ctx
    p = abi.make_params(W, H)
    s0, cam, bits0 = files("room", "base")
    s1, _, bits1 = files("room", "move1_out")
    _passes(c, s0, cam, p)
    assert c.room_info()[0]
    c.upload(s1)
    assert not c.room_info()[0]
    _forged_update(c, p, bits1, 0b010, 0b101, 30, "room skip off")
    # and back: the fact true again, the update merges into bits written without it
    c.render_shadows_async()
    c.upload(s0)
    assert c.room_info()[0]
    _forged_update(c, p, bits0, 0b010, 0b101, 31, "room skip on")
    c.upload(s1)
    c.render_shadows_async()
    c.upload(s0)
    c.update_shadows_async(0b010)
    assert np.array_equal(shadowbuf.peek(c, W * H), bits0)
    _relit_equals_a_fresh_render(c, cam, W, H, 3, 1, "room skip on")


CATALOGUE = [("W4_Bunny", W, H, {2: (-1.0, 1.0, 1.0)}, {2: 35}, False),
             ("Bunny8Lights", W, H, {0: (1.0, -0.5, 0.5), 7: (-1.0, 0.5, -0.5)}, {0: 5, 7: 3}, False),
             ("W4_Optional", 64, 40, {1: (1.0, 0.0, 1.0)}, {1: 44}, True),
             ("Synthetic100k", 64, 40, {0: (0.5, 0.5, 0.0)}, {0: 8}, True)]


@pytest.mark.parametrize("name,w,h,moves,counts,cull", CATALOGUE, ids=[x[0] for x in CATALOGUE])
def test_catalogue_scenes(checker, name, w, h, moves, counts, cull):
    """(Exact cull: the upload of the moved scene leaves the light anchors' records pending; the update builds them.)"""
    hs = HostScene(name)
    s0, cam = hs.view()
    s1 = _moved(s0, moves)
    mask = sum(1 << l for l in moves)
    bits0, _ = relight_ref.plane(checker, s0, cam, w, h)
    bits1, _ = relight_ref.plane(checker, s1, cam, w, h)
    _assert_changes(bits0, bits1, mask, name, counts)
    p = abi.make_params(w, h)
    c = DeviceContext(DEV)
    try:
        _passes(c, s0, cam, p)
        assert bool(c.cull_info()[0]) == cull
        assert np.array_equal(shadowbuf.peek(c, w * h), bits0)
        c.upload(s1)
        assert c.lib.rtx_update_shadows_async(c.h, 0) == abi.RTX_E_STATE   # a moved light outside the empty mask
        c.update_shadows_async(mask)
        assert bool(c.cull_info()[0]) == cull
        assert np.array_equal(shadowbuf.peek(c, w * h), bits1), name
        _forged_update(c, p, bits1, mask, _all(s1) & ~mask, 40, name)
        # the first launch after an upload is the update under the forged check
        c.upload(s0)
        c.render_shadows_async()
        c.upload(s1)
        _forged_update(c, p, bits1, mask, _all(s1) & ~mask, 41, f"{name} right after the upload")
        c.upload(s0)
        c.render_shadows_async()
        c.upload(s1)
        assert c.refresh_shadows_async() == mask
        assert np.array_equal(shadowbuf.peek(c, w * h), bits1), name
        _relit_equals_a_fresh_render(c, cam, w, h, 3, 1, name)
    finally:
        c.close()


@pytest.mark.parametrize("T", [300, 1100])
def test_deep_stacks(ctx, checker, T):
    s0, cam, keep = deep_scene(T)
    w, h = 64, 40
    p = abi.make_params(w, h)
    s1 = _moved(s0, {1: (1.0, 0.5, 2.0)})
    bits0, _ = relight_ref.plane(checker, s0, cam, w, h)
    bits1, _ = relight_ref.plane(checker, s1, cam, w, h)
    _assert_changes(bits0, bits1, 0b010, f"chain of {T}")
    _passes(ctx, s0, cam, p)
    ctx.upload(s1)
    _forged_update(ctx, p, bits1, 0b010, 0b101, 50, f"chain of {T}")
    ctx.upload(s0)
    ctx.render_shadows_async()
    ctx.upload(s1)
    ctx.update_shadows_async(0b010)
    assert np.array_equal(shadowbuf.peek(ctx, w * h), bits1)
    for cfg in ((0, 1), (3, 1)):
        _relit_equals_a_fresh_render(ctx, cam, w, h, *cfg, f"chain of {T}")
    del keep


def test_generic_kernel(files):
    os.environ["RTX_NO_SPEC"] = "1"   # read once, at context creation
    try:
        c = DeviceContext(DEV)
    finally:
        del os.environ["RTX_NO_SPEC"]
    try:
        p = abi.make_params(W, H)
        s0, cam, bits0 = files("open", "base")
        s1, _, bits1 = files("open", "move12")
        c.upload(s0)
        c.render(cam, p)
        assert c.spec_info()[1] == -1
        _passes(c, s0, cam, p)
        c.upload(s1)
        for k, mask in enumerate((0b110, 0b010, 0b100)):   # (after the first, re-traces of the recorded lights)
            _forged_update(c, p, bits1, mask, 0b111 & ~mask, 60 + k, f"generic kernel mask {mask:#b}")
        c.upload(s0)
        c.render_shadows_async()
        c.upload(s1)
        c.update_shadows_async(0b110)
        assert np.array_equal(shadowbuf.peek(c, W * H), bits1)
        _relit_equals_a_fresh_render(c, cam, W, H, 3, 1, "generic kernel")
    finally:
        c.close()


# ---- 5. views and stripes -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("first", [0, 1])
def test_views_and_stripes(ctx, checker, first):
    hs = HostScene("W4_Bunny")
    s0, cam = hs.view()
    s1 = _moved(s0, {2: (-1.0, 1.0, 1.0)})
    w, h, nv = 40, 32, 3
    n = w * h
    cams = gs.cams3(cam)
    p = abi.make_params(w, h, 3, 1, abi.XRGB8888, 16, first, 2)
    want0 = [relight_ref.plane(checker, s0, cv, w, h)[0] for cv in cams]
    want1 = [relight_ref.plane(checker, s1, cv, w, h)[0] for cv in cams]
    for v in range(nv):
        own = devbuf.owned_rows(p, v)
        assert own.any() and not own.all()
        _assert_changes(want0[v].reshape(h, w)[own], want1[v].reshape(h, w)[own], 0b100, f"view {v} owned rows")
    ctx.upload(s0)
    ctx.render_aov_async(cams, p, AOV_ALL)
    ctx.render_shadows_async()
    ctx.upload(s1)
    _forged_update(ctx, p, want1, 0b100, 0b011, 70 + first, f"3 views, first {first}", n_views=nv)
    # a true plane, and its copies: full-frame, owned rows only
    ctx.upload(s0)
    ctx.render_shadows_async()
    ctx.upload(s1)
    ctx.update_shadows_async(0b100)
    sent = np.uint32(0x5A5A5A5A)
    bits = np.full(nv * n, sent, np.uint32)
    ctx.gather_shadows_async(bits)
    ctx.synchronize()
    for v in range(nv):
        own = devbuf.owned_rows(p, v)
        brow = bits[v * n:(v + 1) * n].reshape(h, w)
        assert (brow[~own] == sent).all() and np.array_equal(brow[own], want1[v].reshape(h, w)[own])


# ---- 6. 32 lights ---------------------------------------------------------------------------------------------------

def _lights_scene(tmp_path, name, lights):
    path = tmp_path / f"{name}.rtxscene"
    path.write_text("\n".join([sus.CAMERA, *sus.MATS, *sus.GEOMETRY["room"], *lights]) + "\n")
    return HostScene(f"file:{path}")


def test_32_lights_and_the_refusal_of_33(checker, tmp_path):
    c = DeviceContext(DEV)
    p = abi.make_params(W, H)
    try:
        hs = _lights_scene(tmp_path, "lights32", gs.many_lights(32))
        s0, cam = hs.view()
        assert s0.n_lights == 32
        s1 = _moved(s0, {31: (1.5, 1.0, -2.0), 0: (-1.5, 0.5, -1.0)})
        mask = 0x80000001
        bits0, _ = relight_ref.plane(checker, s0, cam, W, H)
        bits1, _ = relight_ref.plane(checker, s1, cam, W, H)
        _assert_changes(bits0, bits1, mask, "32 lights")
        assert devbuf.owned_rows(p, 0).all()   # no stripes: every row is owned, no sentinel is needed
        _passes(c, s0, cam, p)
        c.upload(s1)
        # (the forged words use all 32 bits; with every row owned the sentinel value is never written anywhere)
        _forged_update(c, p, bits1, mask, 0xFFFFFFFF & ~mask, 80, "32 lights", sentinel=0)
        c.upload(s0)
        c.render_shadows_async()
        c.upload(s1)
        assert c.refresh_shadows_async() == mask
        assert np.array_equal(shadowbuf.peek(c, W * H), bits1)
        _relit_equals_a_fresh_render(c, cam, W, H, 3, 1, "32 lights")
        hs33 = _lights_scene(tmp_path, "lights33", gs.many_lights(33))
        s33, _ = hs33.view()
        assert s33.n_lights == 33
        c.upload(s33)
        traced = C.c_uint32(5)
        assert c.lib.rtx_refresh_shadows_async(c.h, C.byref(traced)) == abi.RTX_E_UNSUPPORTED
        assert b"32" in c.lib.rtx_last_error(c.h)
        assert c.lib.rtx_update_shadows_async(c.h, 1) == abi.RTX_E_UNSUPPORTED
        px, rgb = c.render(cam, p)
        rpx, rrgb = oracle_bind.render(s33, cam, p)
        assert np.array_equal(px, rpx) and np.array_equal(rgb.view(np.uint32), rrgb.view(np.uint32))
    finally:
        c.close()


# ---- 7. the error table and isolation ---------------------------------------------------------------------------------

def test_error_table(files):
    hs = HostScene("W4_Bunny")
    s, cam = hs.view()
    p = abi.make_params(W, H)
    ms = C.c_float()
    c = DeviceContext(DEV)
    lib = c.lib
    upd = lambda m: lib.rtx_update_shadows_async(c.h, m)   # noqa: E731
    try:
        assert upd(1) == abi.RTX_E_STATE and upd(0) == abi.RTX_E_STATE                  # no scene
        assert lib.rtx_refresh_shadows_async(c.h, None) == abi.RTX_E_STATE
        c.upload(s)
        assert upd(1) == abi.RTX_E_STATE                                                   # no hit pass
        assert lib.rtx_refresh_shadows_async(c.h, None) == abi.RTX_E_STATE
        gs.renders_correctly(c, s, cam, W, H)
        c.render_aov(cam, p, AOV_DEPTH)
        assert upd(1) == abi.RTX_E_STATE                                                   # fewer than four planes
        assert lib.rtx_refresh_shadows_async(c.h, None) == abi.RTX_E_STATE
        gs.renders_correctly(c, s, cam, W, H)
        c.render_aov(cam, p, AOV_ALL)
        assert upd(1) == abi.RTX_E_STATE and b"shadow pass" in lib.rtx_last_error(c.h)     # no shadow pass
        assert lib.rtx_time_shadows_update(c.h, 1, 1, C.byref(ms)) == abi.RTX_E_STATE
        gs.renders_correctly(c, s, cam, W, H)
        c.render_shadows_async()
        plane = shadowbuf.peek(c, W * H)
        assert upd(0) == abi.RTX_OK and upd(0b111) == abi.RTX_OK
        assert np.array_equal(shadowbuf.peek(c, W * H), plane)
        assert upd(0b1000) == abi.RTX_E_INVALID and upd(0x80000000) == abi.RTX_E_INVALID  # a bit past the lights
        assert lib.rtx_time_shadows_update(c.h, 0b1000, 1, C.byref(ms)) == abi.RTX_E_INVALID
        assert lib.rtx_time_shadows_update(c.h, 1, 0, C.byref(ms)) == abi.RTX_E_INVALID
        assert lib.rtx_time_shadows_update(c.h, 1, -3, C.byref(ms)) == abi.RTX_E_INVALID
        assert lib.rtx_time_shadows_update(c.h, 1, 1, None) == abi.RTX_E_INVALID
        assert c.time_shadows_update(0b101, 2) > 0.0
        assert np.array_equal(shadowbuf.peek(c, W * H), plane)
        gs.renders_correctly(c, s, cam, W, H)
        c.set_supersample(2)
        assert upd(1) == abi.RTX_E_UNSUPPORTED
        assert lib.rtx_refresh_shadows_async(c.h, None) == abi.RTX_E_UNSUPPORTED
        c.set_supersample(1)
        gs.renders_correctly(c, s, cam, W, H)
        # a light outside the mask moved: refused by name, the plane and its record as before
        s1 = _moved(s, {1: (0.5, 0.0, 0.5), 2: (0.0, 0.5, 0.0)})
        c.upload(s1)
        F = shadowforge.forged(p, 1, 90)
        shadowforge.write(c, F)
        assert upd(0b100) == abi.RTX_E_STATE and b"light 1" in lib.rtx_last_error(c.h)
        assert upd(0b001) == abi.RTX_E_STATE and b"light 1" in lib.rtx_last_error(c.h)
        assert upd(0b010) == abi.RTX_E_STATE and b"light 2" in lib.rtx_last_error(c.h)
        assert np.array_equal(shadowbuf.peek(c, W * H), F)
        assert lib.rtx_relight_async(c.h, C.byref(p), 0) == abi.RTX_E_STATE               # still refused
        shadowforge.write(c, plane)
        c.upload(s)
        assert lib.rtx_relight_async(c.h, C.byref(p), 0) == abi.RTX_OK                    # the record was kept
        gs.renders_correctly(c, s, cam, W, H)
        # a changed light count
        s2, cam2, _ = files("room", "base")
        s3, _, _ = files("room", "added")
        _passes(c, s2, cam2, p)
        c.upload(s3)
        assert upd(0b1000) == abi.RTX_E_STATE and upd(0b1111) == abi.RTX_E_STATE
        assert b"lights" in lib.rtx_last_error(c.h)
        gs.renders_correctly(c, s3, cam2, W, H)
        # a hit pass newer than the plane
        c.upload(s2)
        c.render_aov(cam2, p, AOV_ALL)
        assert upd(1) == abi.RTX_E_STATE and b"earlier hit pass" in lib.rtx_last_error(c.h)
        gs.renders_correctly(c, s2, cam2, W, H)
    finally:
        c.close()


def test_isolation():
    hs = HostScene("W4_Bunny")
    s, cam = hs.view()
    s1 = _moved(s, {2: (-1.0, 1.0, 1.0)})
    n = W * H
    p = abi.make_params(W, H)
    c = DeviceContext(DEV)
    try:
        c.upload(s)
        c.render(cam, abi.make_params(64, 48))   # the last colour frame: 64 x 48
        before = c.render_aov(cam, p, AOV_ALL)
        c.render_shadows_async()
        c.upload(s1)
        spec, split = c.spec_info(), c.split_info()
        # no word of the colour frame buffer
        devbuf.poison(c, 64 * 48, rgb=True)
        c.update_shadows_async(0b100)
        assert c.refresh_shadows_async() == 0
        gpx, grgb = devbuf.peek(c, 64 * 48, rgb=True)
        assert (gpx == devbuf.PX_SENTINEL).all() and (grgb == devbuf.RGB_SENTINEL).all()
        # the hit planes and the frames' records
        after = c.download_aov(aov_host_planes(W, H, AOV_ALL))
        assert not aov_ref.diff(after, before)
        assert c.spec_info() == spec and c.split_info() == split
        # queued between two frames of different cameras, it changes neither
        cam_b = gs.cams3(cam)[1]
        want_a, want_b = c.render(cam, p), c.render(cam_b, p)
        assert not np.array_equal(want_a[0], want_b[0])
        got = [(np.zeros(n, np.uint32), np.zeros(3 * n, np.float32)) for _ in range(2)]
        c.render_async(cam, p, True)
        c.gather_async(*got[0])
        c.update_shadows_async(0b100)
        c.render_async(cam_b, p, True)
        c.gather_async(*got[1])
        c.synchronize()
        assert aov_ref.same(got[0][0], want_a[0]) and aov_ref.same(got[0][1], want_a[1])
        assert aov_ref.same(got[1][0], want_b[0]) and aov_ref.same(got[1][1], want_b[1])
    finally:
        c.close()


# ---- 8. the Python Renderer and the CLI -----------------------------------------------------------------------------

def test_renderer_update_and_refresh(checker):
    hs = HostScene("W4_Bunny")
    s0, cam = hs.view()
    moved = [float(np.float32(s0.lights[2].origin[k]) + np.float32(d)) for k, d in enumerate((-1.0, 1.0, 1.0))]
    r = Renderer(W, H, DEV)
    other = Renderer(W + 3, H, DEV)
    try:
        with pytest.raises(RuntimeError):
            r.UpdateShadows(1)   # no pass yet
        with pytest.raises(RuntimeError):
            r.RefreshShadows()
        r.RenderAOV(hs)
        bits0 = r.RenderShadows()
        assert np.array_equal(bits0, relight_ref.plane(checker, s0, cam, W, H)[0])
        hs.set_light_origin(2, moved)
        s1, _ = hs.view()
        bits1 = relight_ref.plane(checker, s1, cam, W, H)[0]
        _assert_changes(bits0, bits1, 0b100, "Renderer", {2: 35})
        r.ctx.upload(s1)
        assert np.array_equal(r.UpdateShadows(0b100), bits1)
        got = r.Relight().copy()
        assert aov_ref.same(got, r.Render(hs, upload=False))
        hs.set_light_origin(2, list(s0.lights[2].origin)[:2] + [-5.0])
        r.ctx.upload(hs.view()[0])
        assert np.array_equal(r.RefreshShadows(), relight_ref.plane(checker, hs.view()[0], cam, W, H)[0])
        # the _own_pass guard: a renderer of another size on the same context's pass
        other.ctx.close()
        other.ctx = r.ctx
        with pytest.raises(RuntimeError, match="not this renderer's"):
            other.UpdateShadows(0b100)
        with pytest.raises(RuntimeError, match="not this renderer's"):
            other.RefreshShadows()
    finally:
        r.ctx.close()


def test_cli_move_light(checker, tmp_path):
    assert EXE.exists(), "lib/rtx_render is not built"
    move = "1,-1.5,5,-4"

    def run(*args):
        return subprocess.run([str(EXE), "W4_Optional", "61", "45", *args], check=True, cwd=tmp_path, timeout=120,
                              capture_output=True, text=True).stdout

    run("--out", "plain.bmp")
    run("--move-light", move, "--out", "a.bmp")
    out = run("--move-light", move, "--relight", "--aov", "r", "--out", "b.bmp")
    a = (tmp_path / "a.bmp").read_bytes()
    assert len(a) == 54 + 4 * 61 * 45
    assert (tmp_path / "b.bmp").read_bytes() == a and (tmp_path / "plain.bmp").read_bytes() != a
    assert "0x2" in out   # only light 1 was re-traced
    hs = HostScene("W4_Optional")
    hs.set_light_origin(1, (-1.5, 5.0, -4.0))
    s, cam = hs.view()
    bits = np.fromfile(tmp_path / "r_shadow.u32", np.uint32)
    assert np.array_equal(bits, relight_ref.plane(checker, s, cam, 61, 45)[0])
    # a light the scene does not have: refused before any device work
    r = subprocess.run([str(EXE), "W4_Optional", "61", "45", "--move-light", "3,0,0,0", "--out", "c.bmp"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--move-light" in r.stderr and not (tmp_path / "c.bmp").exists()
