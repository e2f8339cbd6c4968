"""The contract every consumer of the stored hit pass shares (deferred shading, the relight and its resolve, the
three shadow entry points, and the rtx_time_* form of each that has one), on the GPU at 32 x 16:

1. the ORDER of the checks: single faults, and pairs of faults set at once so that the earlier check must win;
2. a failed call changes nothing: pixels, shadow words and buffer addresses after the failing calls equal those
   before, word for word;
3. a timed form leaves what its async form leaves, rejects `iters <= 0` and a NULL `mean_ms` before any other
   check (a NULL context included), and the incremental timer with an empty mask returns exactly 0.

The expected codes and message texts are literals here, copied from the library's source; none is produced by
calling the library.  The scene is the room of tests/shadow_update_scenes.py."""
import ctypes as C
import math

import numpy as np
import pytest

import shadow_update_scenes as sus
from gp1_raytracer_2223_amd import abi
from gp1_raytracer_2223_amd.renderer import AOV_ALL, AOV_DEPTH, DeviceContext, aov_host_planes
from gp1_raytracer_2223_amd.scene import HostScene
from gpu_support import DEV, FP, UP

pytestmark = pytest.mark.gpu

W, H = 32, 16
INVALID, STATE, UNSUPPORTED = abi.RTX_E_INVALID, abi.RTX_E_STATE, abi.RTX_E_UNSUPPORTED

# ---- the literals (rtx_pass.hip, rtx_relight.hip) ----------------------------------------------------------------
NO_SCENE = (STATE, "no scene uploaded")
NO_PASS = (STATE, "no hit pass rendered yet")
BAD_MODE = (INVALID, "bad lighting mode")
BAD_FORMAT = (INVALID, "bad pixel format")
FEWER_MATERIALS = (STATE, "the scene has 2 materials, the hit pass was traced with 5")
LIGHTS_33 = (UNSUPPORTED, "the shadow plane holds 32 lights, the scene has 33")
BAD_FACTOR = (INVALID, "the resolve factor must be 2, 4 or 8")
NO_SAMPLE_FRAME = (INVALID, "the hit pass of 30x16 is no sample frame of factor 4: both sides must be multiples of it")


def supersampled(what):
    return (UNSUPPORTED, f"no {what} on a supersampled context (factor 2): the hit pass has one record per pixel")


def depth_only(what):
    return (STATE, f"{what} needs all four planes: the last hit pass wrote mask 1")


# ---- the entry points: name -> (what its messages call it, takes parameters, async form, timed form or None) ------
# Each form is f(lib, h, p, k) -> code; the shadow entries ignore p and k, all but the resolve ignore k.
def _ms():
    return C.byref(C.c_float())


ENTRIES = {
    "shade_aov": ("deferred shading", True,
                  lambda lib, h, p, k: lib.rtx_shade_aov_async(h, C.byref(p), 0),
                  lambda lib, h, p, k: lib.rtx_time_shade_aov(h, C.byref(p), 0, 1, _ms())),
    "relight": ("relight", True,
                lambda lib, h, p, k: lib.rtx_relight_async(h, C.byref(p), 0),
                lambda lib, h, p, k: lib.rtx_time_relight(h, C.byref(p), 0, 1, _ms())),
    "relight_resolve": ("relight", True,
                        lambda lib, h, p, k: lib.rtx_relight_resolve_async(h, C.byref(p), k, 0),
                        lambda lib, h, p, k: lib.rtx_time_relight_resolve(h, C.byref(p), k, 0, 1, _ms())),
    "render_shadows": ("shadow pass", False,
                       lambda lib, h, p, k: lib.rtx_render_shadows_async(h),
                       lambda lib, h, p, k: lib.rtx_time_shadows(h, 1, _ms())),
    "update_shadows": ("shadow pass", False,
                       lambda lib, h, p, k: lib.rtx_update_shadows_async(h, 1),
                       lambda lib, h, p, k: lib.rtx_time_shadows_update(h, 1, 1, _ms())),
    "refresh_shadows": ("shadow pass", False,
                        lambda lib, h, p, k: lib.rtx_refresh_shadows_async(h, None),
                        None),
}
SHADE = [e for e, v in ENTRIES.items() if v[1]]
SHADOWS = [e for e, v in ENTRIES.items() if not v[1]]


def _params(mode=abi.RTX_MODE_COMBINED, shadows=True, fmt=abi.XRGB8888):
    return abi.make_params(1, 1, mode, shadows, fmt)   # (the size and the stripes are the pass's)


GOOD = _params()
MODE_9 = _params(mode=9)
FORMAT_25 = _params(fmt=(25, 8, 0, 0))
MODE_9_FORMAT_25 = _params(mode=9, fmt=(25, 8, 0, 0))


# ---- the scenes -------------------------------------------------------------------------------------------------
def _write(d, name, lines):
    path = d / f"{name}.rtxscene"
    path.write_text("\n".join(lines) + "\n")
    return HostScene(f"file:{path}")


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    """name -> (host scene, scene, camera): the room; the room under light 0 moved; the room with one material
    besides the default one; the room under 33 lights."""
    d = tmp_path_factory.mktemp("pass_contract")
    room = sus.GEOMETRY["room"][:5] + ["mesh lowpoly_bunny2 1 back scale 2 2 2"]   # (the planes' material is 1 too)
    ring = [f"light point {3.5 * math.cos(0.19 * i):.4f} {4.0 + 0.1 * i:.4f} {4.0 + 3.5 * math.sin(0.19 * i):.4f}  "
            f"{6 + i % 5} 0.5 0.7 0.9" for i in range(33)]
    hs = {"room": sus.file_scene(d, "room", "base"),
          "moved": sus.file_scene(d, "room", "move0"),
          "two_materials": _write(d, "two_materials", [sus.CAMERA, sus.MATS[0], *room, *sus.BASE]),
          "lights33": _write(d, "lights33", [sus.CAMERA, *sus.MATS, *sus.GEOMETRY["room"], *ring])}
    out = {k: (v, *v.view()) for k, v in hs.items()}
    assert out["room"][1].n_materials == 5 and out["two_materials"][1].n_materials == 2
    assert out["room"][1].n_lights == 3 and out["lights33"][1].n_lights == 33
    return out


def _context(scenes, scene="room", mask=0, shadows=False, w=W, h=H, then=None, ss=1):
    """A fresh context: `scene` uploaded (None: no scene), supersampling `ss`, a hit pass of `mask` at w x h (0:
    none), its shadow pass when asked for, then the upload of scene `then`."""
    c = DeviceContext(DEV)
    if scene is not None:
        _, s, cam = scenes[scene]
        c.upload(s)
        if ss != 1:
            c.set_supersample(ss)
        if mask:
            c.render_aov_async(cam, abi.make_params(w, h), mask)
        if shadows:
            c.render_shadows_async()
        if then is not None:
            c.upload(scenes[then][1])
    return c


# ---- 1. the order of the checks ----------------------------------------------------------------------------------
# state -> how its context is made; the faults of a row are its state and its parameters together
STATES = {
    "no_scene": dict(scene=None),
    "supersampled": dict(ss=2),
    "no_pass": dict(),
    "depth_only": dict(mask=AOV_DEPTH),
    "passes": dict(mask=AOV_ALL, shadows=True),
    "fewer_materials": dict(mask=AOV_ALL, shadows=True, then="two_materials"),
    "fewer_materials_no_shadow_pass": dict(mask=AOV_ALL, then="two_materials"),
    "lights33": dict(mask=AOV_ALL, shadows=True, then="lights33"),
    "pass_30x16": dict(mask=AOV_ALL, shadows=True, w=30),
}

# (state, entries, parameters, factor, expected (code, message)); an expected value that is callable takes the
# entry's `what`
ROWS = [
    # single faults
    ("no_scene", SHADE + SHADOWS, GOOD, 2, NO_SCENE),
    ("supersampled", SHADE + SHADOWS, GOOD, 2, supersampled),
    ("no_pass", SHADE + SHADOWS, GOOD, 2, NO_PASS),
    ("depth_only", SHADE + SHADOWS, GOOD, 2, depth_only),
    ("fewer_materials", SHADE, GOOD, 2, FEWER_MATERIALS),
    ("passes", SHADE, MODE_9, 2, BAD_MODE),
    ("passes", SHADE, FORMAT_25, 2, BAD_FORMAT),
    ("lights33", SHADOWS, GOOD, 2, LIGHTS_33),
    ("passes", ["relight_resolve"], GOOD, 3, BAD_FACTOR),
    ("pass_30x16", ["relight_resolve"], GOOD, 4, NO_SAMPLE_FRAME),
    # pairs: the earlier check wins
    ("no_scene", SHADE, MODE_9, 2, BAD_MODE),                     # mode before scene
    ("supersampled", SHADE, FORMAT_25, 2, BAD_FORMAT),            # format before supersampling
    ("passes", ["relight_resolve"], MODE_9, 3, BAD_FACTOR),       # factor before mode
    ("passes", SHADE, MODE_9_FORMAT_25, 2, BAD_MODE),             # mode before format
    ("no_scene", ["relight_resolve"], MODE_9, 3, BAD_FACTOR),     # factor before mode before scene
    ("depth_only", SHADE, FORMAT_25, 2, BAD_FORMAT),              # format before the planes
    ("pass_30x16", ["relight_resolve"], MODE_9, 4, BAD_MODE),     # the relight's checks before divisibility
    # materials before the shadow plane's currency: shadows on, and no shadow pass was ever rendered
    ("fewer_materials_no_shadow_pass", ["relight", "relight_resolve"], GOOD, 2, FEWER_MATERIALS),
]
CASES = [(state, entry, form, p, k, want) for state, entries, p, k, want in ROWS for entry in entries
         for form in (2, 3) if ENTRIES[entry][form] is not None]


@pytest.fixture(scope="module")
def states(scenes):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _context(scenes, **STATES[name])
        return made[name]
    yield get
    for c in made.values():
        c.close()


def _expect(c, call, p, k, want, what):
    rc = call(c.lib, c.h, p, k)
    got = (c.lib.rtx_last_error(c.h) or b"").decode()
    print(f"{what}: code {rc}, {got!r}")
    assert (rc, got) == want, what


@pytest.mark.parametrize("state,entry,form,p,k,want", CASES,
                         ids=[f"{s}-{e}{'-timed' if f == 3 else ''}-{i}" for i, (s, e, f, *_) in enumerate(CASES)])
def test_check_order(states, state, entry, form, p, k, want):
    what = ENTRIES[entry][0]
    _expect(states(state), ENTRIES[entry][form], p, k, want(what) if callable(want) else want, (state, entry, form))


# ---- 2. a failed call changes nothing ----------------------------------------------------------------------------
def _download(c, n, rgb=True):
    px, col = np.zeros(n, np.uint32), np.zeros(3 * n, np.float32)
    abi.check(c.lib.rtx_download(c.h, px.ctypes.data_as(UP), col.ctypes.data_as(FP) if rgb else None), "rtx_download",
              c.h)
    return px, col.view(np.uint32)


def test_a_failed_call_changes_nothing(scenes):
    c = _context(scenes, mask=AOV_ALL, shadows=True)
    try:
        c.relight_async(GOOD, True)
        before = (*_download(c, W * H), c.download_shadows(), c.device_buffers(), c.device_shadow_buffer(),
                  c.device_aov_buffers())
        failed = 0
        for state, entries, p, k, want in ROWS:
            if state != "passes":
                continue
            for entry in entries:
                for form in (2, 3):
                    if ENTRIES[entry][form] is not None:
                        _expect(c, ENTRIES[entry][form], p, k, want, ("unchanged", entry, form))
                        failed += 1
        ms = C.c_float(7.0)
        for rc in (c.lib.rtx_update_shadows_async(c.h, 8),                       # a light the scene does not have
                   c.lib.rtx_time_shadows_update(c.h, 8, 1, C.byref(ms)),
                   c.lib.rtx_time_relight(c.h, C.byref(GOOD), 1, 0, C.byref(ms)),
                   c.lib.rtx_time_shadows(c.h, 1, None)):
            assert rc == INVALID
            failed += 1
        assert failed == 26 and ms.value == 7.0
        c.relight_async(GOOD, True)
        after = (*_download(c, W * H), c.download_shadows(), c.device_buffers(), c.device_shadow_buffer(),
                 c.device_aov_buffers())
        for a, b in zip(before, after):
            assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
        assert before[0].any() and before[2].any()
    finally:
        c.close()


# ---- 3. the timed forms ------------------------------------------------------------------------------------------
def _timed_vs_async(scenes, prepare, timed, queued, read):
    """prepare(c); then timed(c) -> ms on one context and queued(c) on a fresh one; read(c) -> arrays, equal."""
    out = []
    for run in (timed, queued):
        c = _context(scenes)
        try:
            prepare(c)
            ms = run(c)
            if run is timed:
                print(f"mean {ms} ms")
                assert math.isfinite(ms) and ms > 0.0
            out.append(read(c))
        finally:
            c.close()
    assert len(out[0]) == len(out[1])
    for a, b in zip(*out):
        assert a.any() and np.array_equal(a, b)


def _passes(scenes, w=W, h=H, shadows=True):
    def prepare(c):
        c.render_aov_async(scenes["room"][2], abi.make_params(w, h), AOV_ALL)
        if shadows:
            c.render_shadows_async()
    return prepare


def test_time_shade_aov_leaves_the_shade(scenes):
    _timed_vs_async(scenes, _passes(scenes, shadows=False), lambda c: c.time_shade_aov(GOOD, True, 3),
                    lambda c: c.shade_aov_async(GOOD, True), lambda c: _download(c, W * H))


def test_time_relight_leaves_the_relight(scenes):
    _timed_vs_async(scenes, _passes(scenes), lambda c: c.time_relight(GOOD, True, 3),
                    lambda c: c.relight_async(GOOD, True), lambda c: _download(c, W * H))


def test_time_relight_resolve_leaves_the_resolve(scenes):
    _timed_vs_async(scenes, _passes(scenes, 64, 32), lambda c: c.time_relight_resolve(GOOD, 2, True, 3),
                    lambda c: c.relight_resolve_async(GOOD, 2, True), lambda c: _download(c, W * H))


def test_time_shadows_leaves_the_plane(scenes):
    _timed_vs_async(scenes, _passes(scenes, shadows=False), lambda c: c.time_shadows(3),
                    lambda c: c.render_shadows_async(), lambda c: (c.download_shadows(),))


def test_time_shadows_update_leaves_the_update(scenes):
    def prepare(c):
        _passes(scenes)(c)
        c.upload(scenes["moved"][1])   # light 0 moved: the plane's bit 0 is stale

    def read(c):   # the plane, and the relight that takes it for current
        c.relight_async(GOOD, False)
        return c.download_shadows(), _download(c, W * H, False)[0]
    _timed_vs_async(scenes, prepare, lambda c: c.time_shadows_update(1, 3), lambda c: c.update_shadows_async(1), read)


def test_time_aov_frames_leaves_the_pass(scenes):
    p = abi.make_params(W, H)
    _timed_vs_async(scenes, lambda c: None, lambda c: c.time_aov_frames(scenes["room"][2], p, AOV_ALL, 3),
                    lambda c: c.render_aov_async(scenes["room"][2], p, AOV_ALL),
                    lambda c: [v.view(np.uint32) for v in c.download_aov(aov_host_planes(W, H, AOV_ALL)).values()])


def test_time_shadows_update_of_no_light_is_zero(scenes):
    c = _context(scenes, mask=AOV_ALL, shadows=True)
    try:
        before = c.download_shadows()
        ms = C.c_float(7.0)
        assert c.lib.rtx_time_shadows_update(c.h, 0, 3, C.byref(ms)) == abi.RTX_OK
        assert ms.value == 0.0
        assert before.any() and np.array_equal(c.download_shadows(), before)
    finally:
        c.close()


def test_timed_forms_reject_their_own_arguments_first(scenes):
    """iters = 0 or a NULL mean_ms: RTX_E_INVALID before any other check, from a context that fails every later
    check (no scene) and from a NULL context, which every timed form tolerates with such arguments."""
    c = _context(scenes, scene=None)
    lib, cam, p, bad = c.lib, scenes["room"][2], abi.make_params(W, H), MODE_9
    planes = abi.AovPlanes()
    forms = {
        "rtx_time_views": lambda h, it, ms: lib.rtx_time_views(h, C.byref(cam), 1, C.byref(p), it, ms),
        "rtx_time_frames": lambda h, it, ms: lib.rtx_time_frames(h, C.byref(cam), C.byref(p), it, ms),
        "rtx_time_aov_frames": lambda h, it, ms: lib.rtx_time_aov_frames(h, C.byref(cam), C.byref(p), AOV_ALL, it, ms),
        "rtx_time_shade_aov": lambda h, it, ms: lib.rtx_time_shade_aov(h, C.byref(bad), 0, it, ms),
        "rtx_time_relight": lambda h, it, ms: lib.rtx_time_relight(h, C.byref(bad), 0, it, ms),
        "rtx_time_relight_resolve": lambda h, it, ms: lib.rtx_time_relight_resolve(h, C.byref(bad), 3, 0, it, ms),
        "rtx_time_shadows": lambda h, it, ms: lib.rtx_time_shadows(h, it, ms),
        "rtx_time_shadows_update": lambda h, it, ms: lib.rtx_time_shadows_update(h, 1, it, ms),
        "rtx_time_ray_queries": lambda h, it, ms: lib.rtx_time_ray_queries(h, None, 64, 0, AOV_ALL, C.byref(planes), None,
                                                                        it, ms),
        "rtx_time_shade_rays": lambda h, it, ms: lib.rtx_time_shade_rays(h, None, 64, C.byref(p), None, None, it, ms),
        "rtx_time_adaptive_frames": lambda h, it, ms: lib.rtx_time_adaptive_frames(h, C.byref(cam), C.byref(p), 2, 16,
                                                                                it, ms),
    }
    try:
        for name, f in forms.items():
            ms = C.c_float(7.0)
            for h in (c.h, None):
                assert f(h, 0, C.byref(ms)) == INVALID, (name, h, "iters = 0")
                assert f(h, -1, C.byref(ms)) == INVALID, (name, h, "iters < 0")
                assert f(h, 1, None) == INVALID, (name, h, "NULL mean_ms")
            assert ms.value == 7.0, name
    finally:
        c.close()
