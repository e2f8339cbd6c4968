"""The hit pass (rtx_render_aov*, PHASE 7 of the render kernel) on the GPU against the checker of
tests/aov_ref.py: every plane word for word (a NaN float equals any NaN), on the catalogue scenes,
the fuzz scenes and their committed goldens, every walk the colour frames take (exact cull, deep
stacks in LDS and in HBM), stripes, views and groups, beside colour frames that it must not
disturb, after a device Update, through the Python Renderer and the CLI, and on its error paths.
Frames are 37 x 23 unless a case needs more: five tile columns and three tile rows, one of each
partial."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import aov_ref
import gpu_support as gs
import oracle_bind
from checkers import checker  # noqa: F401
from gp1_raytracer_2223_amd import abi
from gp1_raytracer_2223_amd.renderer import (AOV_ALL, AOV_DEPTH, AOV_MATERIAL, AOV_NORMAL, AOV_PRIMITIVE,
                                             DeviceAnimation, DeviceContext, DeviceGroup, Renderer,
                                             aov_host_planes)
from gp1_raytracer_2223_amd.scene import HostScene
from gpu_support import DEV
from gpu_support import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
G = ROOT / "tests" / "golden" / "aov"
W, H = 37, 23
SENTINEL = {"depth": np.float32(-7.5), "normal": np.float32(-7.5), "material": np.uint32(0xDEADBEEF),
            "primitive": np.uint32(0xDEADBEEF)}


_want = {}


def _ref(checker, name, t=-1.0, w=W, h=H):
    """The checker's planes (computed once per case, never written to)."""
    key = (name, t, w, h)
    if key not in _want:
        s, cam = gs.view(name, t)
        p = aov_ref.planes(checker, s, cam, w, h)
        for a in p.values():
            a.setflags(write=False)
        _want[key] = p
    return _want[key]


def _equal(got, want, what, names=aov_ref.NAMES):
    bad = aov_ref.diff(got, want, names)
    assert not bad, f"{what}: planes {bad} differ"


PARITY = [("W1", -1.0), ("W2", -1.0), ("W3", -1.0), ("W4_Reference", -1.0), ("W4_Bunny", -1.0), ("W4_Bunny", 1.3),
          ("W4_Optional", -1.0)]


@pytest.mark.parametrize("name,t", PARITY)
def test_parity(ctx, checker, name, t):
    s, cam = gs.view(name, t)
    ctx.upload(s)
    got = ctx.render_aov(cam, abi.make_params(W, H))
    assert sorted(got) == sorted(aov_ref.NAMES)
    _equal(got, _ref(checker, name, t), f"{name}/t{t}")


CASES = aov_ref.golden_cases()


@pytest.mark.parametrize("family,seed", CASES, ids=[f"{f}_{s}" for f, s in CASES])
def test_fuzz_scenes_and_goldens(ctx, checker, tmp_path, family, seed):
    w, h = aov_ref.GOLDEN_W, aov_ref.GOLDEN_H
    keep, s, cam = aov_ref.golden_view(family, seed, tmp_path)
    ctx.upload(s)
    got = ctx.render_aov(cam, abi.make_params(w, h))
    _equal(got, aov_ref.planes(checker, s, cam, w, h), f"{family}_{seed} against the checker")
    g = np.load(G / f"{family}_{seed}.npz")
    _equal(got, {k: g[k] for k in aov_ref.NAMES}, f"{family}_{seed} against the golden")
    del keep


def test_mask_subsets_and_lazy_planes(checker):
    s, cam = gs.view("W4_Reference")
    want = _ref(checker, "W4_Reference")
    p = abi.make_params(W, H)
    c = DeviceContext(DEV)
    try:
        c.upload(s)
        assert c.device_aov_buffers() == {k: 0 for k in aov_ref.NAMES}
        got = c.render_aov(cam, p, AOV_DEPTH)
        assert list(got) == ["depth"]
        _equal(got, want, "DEPTH", ["depth"])
        d = c.device_aov_buffers()
        assert d["depth"] and not d["normal"] and not d["material"] and not d["primitive"]
        got = c.render_aov(cam, p, AOV_NORMAL | AOV_PRIMITIVE)
        assert sorted(got) == ["normal", "primitive"]
        _equal(got, want, "NORMAL|PRIMITIVE", ["normal", "primitive"])
        d2 = c.device_aov_buffers()
        assert d2["depth"] == d["depth"] and d2["normal"] and d2["primitive"] and not d2["material"]
        _equal(c.render_aov(cam, p, AOV_ALL), want, "ALL")
        assert all(c.device_aov_buffers().values())
    finally:
        c.close()


def test_culled_walk(checker):
    """Synthetic100k renders with the exact cull: the pass takes the CULLK instantiation."""
    s, cam = gs.view("Synthetic100k")
    c = DeviceContext(DEV)
    try:
        c.upload(s)
        assert c.cull_info()[0]
        got = c.render_aov(cam, abi.make_params(128, 72))
        assert c.cull_info() == (True, 1)       # the view's camera records, built by the pass
        _equal(got, _ref(checker, "Synthetic100k", -1.0, 128, 72), "Synthetic100k")
        assert (aov_ref.kind(got["primitive"]) == 3).any()
    finally:
        c.close()


@pytest.mark.parametrize("T", [300, 1100])
def test_deep_stack_variants(ctx, checker, T):
    """T = 300: the deep LDS stack (DEEP); 1100: the stacks in HBM (DEEP + HSTK)."""
    from test_gpu_deep_bvh import deep_scene
    s, cam, keep = deep_scene(T)
    ctx.upload(s)
    got = ctx.render_aov(cam, abi.make_params(W, H))
    _equal(got, aov_ref.planes(checker, s, cam, W, H), f"chain of {T}")
    tri = aov_ref.kind(got["primitive"]) == 3
    assert tri.any() and (aov_ref.index(got["primitive"])[tri] < T).all()
    del keep


def test_stripes_gather_into_one_frame(checker):
    w, h, n = 37, 53, 3
    s, cam = gs.view("W4_Reference")
    want = _ref(checker, "W4_Reference", -1.0, w, h)
    frame = {k: np.full_like(want[k], SENTINEL[k]) for k in aov_ref.NAMES}
    ctxs = [DeviceContext(DEV) for _ in range(n)]
    try:
        for r, c in enumerate(ctxs):
            c.upload(s)
            c.render_aov_async(cam, abi.make_params(w, h, stripe_rows=16, stripe_first=r, stripe_step=n))
        one = {k: np.full_like(want[k], SENTINEL[k]) for k in aov_ref.NAMES}
        ctxs[1].gather_aov_async(one)
        for c in ctxs:
            c.gather_aov_async(frame)
        for c in ctxs:
            c.synchronize()
        _equal(frame, want, "three stripe owners")
        own = np.array([(y // 16) % n == 1 for y in range(h)])
        for k in aov_ref.NAMES:
            a, b = one[k].reshape(h, -1), want[k].reshape(h, -1)
            assert aov_ref.same(a[own], b[own]), k
            assert (a[~own] == SENTINEL[k]).all(), k
    finally:
        for c in ctxs:
            c.close()


def test_views_equal_single_view_passes(ctx):
    n = 3
    s, cam = gs.view("W4_Reference")
    views = []
    for f in range(n):
        v = abi.Camera()
        C.memmove(C.byref(v), C.byref(cam), C.sizeof(abi.Camera))
        v.origin[0] = cam.origin[0] + 0.5 * f
        v.origin[1] = cam.origin[1] + 0.25 * f
        views.append(v)
    ctx.upload(s)
    p = abi.make_params(W, H)
    ctx.render_aov_async(views, p)
    got = ctx.download_aov(aov_host_planes(W, H, AOV_ALL, n))
    singles = [ctx.render_aov(v, p) for v in views]
    for f in range(n):
        for k in aov_ref.NAMES:
            e = 3 if k == "normal" else 1
            assert aov_ref.same(got[k][e * f * W * H:e * (f + 1) * W * H], singles[f][k]), (f, k)
    assert not aov_ref.same(singles[0]["depth"], singles[2]["depth"])   # (the cameras do differ)


def test_group_equals_single_context(ctx):
    w, h = 37, 53
    s, cam = gs.view("W4_Reference")
    ctx.upload(s)
    want = ctx.render_aov(cam, abi.make_params(w, h))
    grp = DeviceGroup([DEV, DEV])
    try:
        grp.upload(s)
        _equal(grp.render_aov(cam, abi.make_params(w, h)), want, "group of 2")
        got = grp.render_aov(cam, abi.make_params(w, h), AOV_MATERIAL)
        assert list(got) == ["material"] and aov_ref.same(got["material"], want["material"])
    finally:
        grp.close()


def test_colour_frames_are_untouched(checker):
    s, cam = gs.view("W4_Bunny")
    p = abi.make_params(W, H)
    c = DeviceContext(DEV)
    try:
        c.upload(s)
        before = c.render(cam, p)
        spec = c.spec_info()
        _equal(c.render_aov(cam, p), _ref(checker, "W4_Bunny"), "pass between colour frames")
        assert c.spec_info() == spec
        # a colour gather after a pass (of another size) still copies the colour frame's rows
        c.render_aov_async(cam, abi.make_params(24, 16), AOV_DEPTH)
        px = np.full(W * H, 0xDEADBEEF, np.uint32)
        c.gather_async(px)
        c.synchronize()
        assert np.array_equal(px, before[0])
        # ... and an AOV gather after a colour frame still copies the pass's
        c.render_async(cam, p)
        small = c.download_aov(aov_host_planes(24, 16, AOV_DEPTH))
        assert aov_ref.same(small["depth"], _ref(checker, "W4_Bunny", -1.0, 24, 16)["depth"])
        after = c.render(cam, p)
        assert np.array_equal(after[0], before[0]) and np.array_equal(after[1].view(np.uint32), before[1].view(np.uint32))
        assert c.spec_info() == spec
    finally:
        c.close()


def _split_ctx():
    os.environ["RTX_SPLIT"] = "force"
    try:
        return DeviceContext(DEV)
    finally:
        del os.environ["RTX_SPLIT"]


def test_split_frames_interleaved_with_passes(checker):
    """A context that splits every tile from its second frame on: its colour frames 1-4 with a pass
    after each equal the same frames without the passes, frame by frame, and the passes (which
    render every tile themselves) equal the checker."""
    w, h = 64, 48
    s, cam = gs.view("W4_Bunny")
    p = abi.make_params(w, h)
    want = _ref(checker, "W4_Bunny", -1.0, w, h)
    a, b = _split_ctx(), _split_ctx()
    try:
        a.upload(s)
        b.upload(s)
        for frame in range(1, 5):
            fa = a.render(cam, p)
            _equal(a.render_aov(cam, p), want, f"pass after split frame {frame}")
            fb = b.render(cam, p)
            assert np.array_equal(fa[0], fb[0]), frame
            assert np.array_equal(fa[1].view(np.uint32), fb[1].view(np.uint32)), frame
            assert a.split_info() == b.split_info(), frame
        assert a.split_info()[0] == (w // 8) * (h // 8)   # every tile is split by now
        rpx, _ = oracle_bind.render(s, cam, p)
        assert np.array_equal(fa[0], rpx)
    finally:
        a.close()
        b.close()


def test_device_update(checker):
    dev_scene = HostScene("W4_Reference")
    c = DeviceContext(DEV)
    anim = DeviceAnimation(dev_scene, c)
    try:
        anim.update(1.3, c)
        got = c.render_aov(gs.view("W4_Reference", 1.3)[1], abi.make_params(W, H))
        assert list(anim.status(0)[:1]) == [0]
        _equal(got, _ref(checker, "W4_Reference", 1.3), "after a device Update")
        assert (aov_ref.kind(got["primitive"]) == 3).any()
    finally:
        anim.close()
        c.close()


def test_renderer_and_cli(checker, tmp_path):
    want = _ref(checker, "W4_Bunny")
    r = Renderer(W, H, device=DEV)
    try:
        hs = HostScene("W4_Bunny")
        _equal(r.RenderAOV(hs), want, "Renderer.RenderAOV")
        got = r.RenderAOV(hs, AOV_PRIMITIVE, upload=False)
        assert list(got) == ["primitive"] and aov_ref.same(got["primitive"], want["primitive"])
    finally:
        r.ctx.close()
    exe = Path(abi.LIB_DIR) / "rtx_render"
    pre = tmp_path / "P"
    subprocess.run([str(exe), "W4_Bunny", str(W), str(H), "--aov", str(pre), "--out", str(tmp_path / "shot.bmp")],
                   check=True, cwd=tmp_path, timeout=120)
    files = {"depth": ("_depth.f32", "<f4"), "normal": ("_normal.f32", "<f4"), "material": ("_material.u32", "<u4"),
             "primitive": ("_primitive.u32", "<u4")}
    got = {k: np.fromfile(str(pre) + suffix, dt).astype(want[k].dtype) for k, (suffix, dt) in files.items()}
    _equal(got, want, "rtx_render --aov")
    bad = subprocess.run([str(exe), "W4_Bunny", str(W), str(H), "--aov", str(pre), "--benchmark", "1"], cwd=tmp_path,
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--aov" in bad.stderr


def test_errors_leave_the_context_usable(checker):
    s, cam = gs.view("W4_Bunny")
    want = _ref(checker, "W4_Bunny")
    p = abi.make_params(W, H)
    c = DeviceContext(DEV)
    lib, h = c.lib, c.h

    def still_renders(after):
        gs.renders_correctly(c, s, cam, W, H)
        _equal(c.render_aov(cam, p), want, f"after {after}")

    try:
        out = abi.AovPlanes()
        # no scene uploaded
        assert lib.rtx_render_aov_async(h, C.byref(cam), 1, C.byref(p), AOV_ALL) == abi.RTX_E_STATE
        assert b"no scene" in lib.rtx_last_error(h)
        # nothing rendered yet
        depth = np.zeros(W * H, np.float32)
        out.depth = depth.ctypes.data_as(C.POINTER(C.c_float))
        assert lib.rtx_download_aov(h, C.byref(out)) == abi.RTX_E_STATE
        assert b"no hit pass" in lib.rtx_last_error(h)
        c.upload(s)
        still_renders("the calls without a scene")
        # empty and unknown masks
        for mask in (0, 16, AOV_ALL | 32):
            assert lib.rtx_render_aov_async(h, C.byref(cam), 1, C.byref(p), mask) == abi.RTX_E_INVALID, mask
            assert b"mask" in lib.rtx_last_error(h), mask
            still_renders(f"mask {mask}")
        # a supersampled context
        c.set_supersample(2)
        assert lib.rtx_render_aov_async(h, C.byref(cam), 1, C.byref(p), AOV_ALL) == abi.RTX_E_UNSUPPORTED
        assert b"supersampled" in lib.rtx_last_error(h)
        c.set_supersample(1)
        still_renders("the supersampled refusal")
        # a plane the last pass did not write, through the download and the gather
        c.render_aov_async(cam, p, AOV_MATERIAL)
        assert lib.rtx_download_aov(h, C.byref(out)) == abi.RTX_E_STATE
        assert b"did not write" in lib.rtx_last_error(h)
        assert lib.rtx_gather_aov_async(h, C.byref(out)) == abi.RTX_E_STATE
        assert b"did not write" in lib.rtx_last_error(h)
        assert (depth == 0).all()
        still_renders("the refused downloads")
    finally:
        c.close()
