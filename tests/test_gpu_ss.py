"""Supersampled frames (rtx_set_supersample) on the GPU against the reference-derived oracle: the
oracle's kW x kH frame (the samples, by definition) resolved and quantized by tests/ss_ref.py.
Pow-free scenes must match bit for bit in both planes; scenes with powf within the project's 1e-4 /
1 LSB (each sample is within 1e-4, so their mean is, up to the mean's own roundings of ~1e-7).
Every other property (stripes, views, groups, the split path, the counters, the factor as context
state) is checked at the smallest frames that still span several wave tiles and a partial one."""
import ctypes as C
import os

import numpy as np
import pytest

import gpu_support as gs
import oracle_bind
import ss_ref
from gp1_raytracer_2223_amd import abi
from gp1_raytracer_2223_amd.renderer import DeviceContext, DeviceGroup
from gp1_raytracer_2223_amd.scene import HostScene
from gpu_support import DEV
from test_gpu_parity import POW_FREE, _compare

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ss_ctx():
    """The context whose factor the tests change (the session's gpu_ctx stays at 1)."""
    ctx = DeviceContext(DEV)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def split_ctx():
    """A context that splits EVERY tile (RTX_SPLIT=force) from its second frame on."""
    os.environ["RTX_SPLIT"] = "force"
    try:
        ctx = DeviceContext(DEV)
    finally:
        del os.environ["RTX_SPLIT"]
    yield ctx
    ctx.close()


_oracle = {}


def _ref(name, t, W, H, k, mode=3, shadows=1):
    """The oracle's supersampled frame (computed once per case, never written to)."""
    key = (name, t, W, H, k, mode, shadows)
    if key not in _oracle:
        s, cam = gs.view(name, t)
        _, hi = oracle_bind.render(s, cam, abi.make_params(k * W, k * H, mode, shadows))
        rgb = ss_ref.resolve(hi, W, H, k)
        px = ss_ref.quantize(rgb)
        rgb.setflags(write=False)
        px.setflags(write=False)
        _oracle[key] = (px, rgb)
    return _oracle[key]


def _same(a, b, what):
    assert np.array_equal(a[0], b[0]), f"{what}: {(a[0] != b[0]).sum()} pixels differ"
    if a[1] is not None and b[1] is not None:
        assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), f"{what}: colours differ"


PARITY = [(n, -1.0, k) for n in ("W4_Bunny", "W2", "W3") for k in (2, 4, 8)] + [("W4_Bunny", 1.3, 2)]


@pytest.mark.parametrize("name,t,k", PARITY)
def test_parity(ss_ctx, name, t, k):
    W, H = 37, 23   # k = 2: 74 x 46 samples, neither a multiple of the 8 x 8 wave tile
    s, cam = gs.view(name, t)
    ss_ctx.upload(s)
    ss_ctx.set_supersample(k)
    gpx, grgb = ss_ctx.render(cam, abi.make_params(W, H))
    rpx, rrgb = _ref(name, t, W, H, k)
    _compare(f"{name}/t{t}/k{k}", gpx, grgb, rpx, rrgb, exact=name in POW_FREE)


def test_k1_after_k4_is_todays_frame(ss_ctx):
    s, cam = gs.view("W4_Bunny")
    ss_ctx.upload(s)
    ss_ctx.set_supersample(4)
    ss_ctx.render(cam, abi.make_params(80, 60))       # a larger frame first: its pixels stay in the buffer
    ss_ctx.render(cam, abi.make_params(37, 23))
    ss_ctx.set_supersample(1)
    got = ss_ctx.render(cam, abi.make_params(37, 23))
    fresh = DeviceContext(DEV)
    try:
        fresh.upload(s)
        want = fresh.render(cam, abi.make_params(37, 23))
    finally:
        fresh.close()
    _same(got, want, "k = 1 after k = 4")
    rpx, rrgb = _ref("W4_Bunny", -1.0, 37, 23, 1)
    _compare("k1", got[0], got[1], rpx, rrgb, exact=True)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("shadows", [0, 1])
def test_modes(ss_ctx, mode, shadows):
    W, H = 40, 30
    s, cam = gs.view("W3")
    ss_ctx.upload(s)
    ss_ctx.set_supersample(2)
    gpx, grgb = ss_ctx.render(cam, abi.make_params(W, H, mode, shadows))
    rpx, rrgb = _ref("W3", -1.0, W, H, 2, mode, shadows)
    _compare(f"W3/m{mode}/s{shadows}/k2", gpx, grgb, rpx, rrgb, exact=mode in (0, 1))


def test_stripes_stitch_bit_identical(ss_ctx):
    W, H = 64, 48
    s, cam = gs.view("W4_Bunny")
    ss_ctx.upload(s)
    ss_ctx.set_supersample(2)
    full, full_rgb = ss_ctx.render(cam, abi.make_params(W, H))
    rpx, rrgb = _ref("W4_Bunny", -1.0, W, H, 2)
    _compare("unstriped", full, full_rgb, rpx, rrgb, exact=True)
    for n in (2, 3):
        stitched = np.full(W * H, 0xDEADBEEF, np.uint32)
        for r in range(n):
            px, _ = ss_ctx.render(cam, abi.make_params(W, H, stripe_rows=16, stripe_first=r, stripe_step=n),
                                  want_rgb=False)
            rows = np.array([(y // 16) % n == r for y in range(H)])
            stitched.reshape(H, W)[rows] = px.reshape(H, W)[rows]
        assert np.array_equal(stitched, full), f"n={n}: {(stitched != full).sum()} pixels differ"


def test_views_equal_single_view_frames(ss_ctx):
    W, H, N = 37, 23, 2
    s, cam = gs.view("W4_Bunny")
    views = (abi.Camera * N)()
    for f in range(N):
        C.memmove(C.byref(views[f]), C.byref(cam), C.sizeof(abi.Camera))
        views[f].origin[0] = cam.origin[0] + 0.25 * f
    ss_ctx.upload(s)
    ss_ctx.set_supersample(2)
    p = abi.make_params(W, H)
    abi.check(ss_ctx.lib.rtx_render_views_async(ss_ctx.h, views, N, C.byref(p), 1), "views", ss_ctx.h)
    px = np.zeros(N * W * H, np.uint32)
    rgb = np.zeros(3 * N * W * H, np.float32)
    abi.check(ss_ctx.lib.rtx_download(ss_ctx.h, px.ctypes.data_as(C.POINTER(C.c_uint32)),
                                      rgb.ctypes.data_as(C.POINTER(C.c_float))), "download", ss_ctx.h)
    for f in range(N):
        one = ss_ctx.render(views[f], p)
        _same((px[f * W * H:(f + 1) * W * H], rgb[3 * f * W * H:3 * (f + 1) * W * H]), one, f"view {f}")
    assert not np.array_equal(px[:W * H], px[W * H:])   # (the two cameras do differ)


def test_group_equals_single_context(ss_ctx):
    W, H = 64, 48
    s, cam = gs.view("W4_Bunny")
    ss_ctx.upload(s)
    ss_ctx.set_supersample(2)
    want = ss_ctx.render(cam, abi.make_params(W, H))
    grp = DeviceGroup([DEV, DEV])
    try:
        grp.upload(s)
        grp.set_supersample(2)
        got = grp.render(cam, abi.make_params(W, H))
        _same(got, want, "group of 2")
        with pytest.raises(RuntimeError, match="1, 2, 4 or 8"):
            grp.set_supersample(3)
        _same(grp.render(cam, abi.make_params(W, H)), want, "group after a refused factor")
    finally:
        grp.close()


def test_split_path(split_ctx):
    W, H = 64, 48
    s, cam = gs.view("W4_Bunny")
    split_ctx.upload(s)
    split_ctx.set_supersample(2)
    p = abi.make_params(W, H)
    first = split_ctx.render(cam, p)                  # measured frame: selects the heavy set
    heavy, parts = split_ctx.split_info()
    assert parts > 1 and heavy == (2 * W // 8) * (2 * H // 8), (heavy, parts)   # every wave tile of the samples
    split_ctx.render(cam, p)
    third = split_ctx.render(cam, p)                  # rendered by the split launches
    _same(third, first, "split frame 3 against frame 1")
    rpx, rrgb = _ref("W4_Bunny", -1.0, W, H, 2)
    _compare("split", third[0], third[1], rpx, rrgb, exact=True)
    split_ctx.set_supersample(1)


def test_light_major_frame():
    """The light-major frame's shading launch (PHASE 6) has the resolving epilogue too."""
    os.environ["RTX_LIGHT_MAJOR"] = "1"
    try:
        ctx = DeviceContext(DEV)
    finally:
        del os.environ["RTX_LIGHT_MAJOR"]
    try:
        W, H = 64, 48
        s, cam = gs.view("W4_Bunny")
        ctx.upload(s)
        ctx.set_supersample(2)
        rpx, rrgb = _ref("W4_Bunny", -1.0, W, H, 2)
        for frame in range(2):   # identity order, then the cost order
            gpx, grgb = ctx.render(cam, abi.make_params(W, H))
            assert ctx.light_major_info()[0]
            _compare(f"light-major frame {frame}", gpx, grgb, rpx, rrgb, exact=True)
    finally:
        ctx.close()


@pytest.mark.parametrize("T", [300, 1100])
def test_deep_stack_variants(ss_ctx, T):
    """The kernels for BVHs deeper than the LDS stack (T = 300: the deep LDS stack, 1100: stacks in
    HBM, one per wave of the sample frame's launch) resolve like the default one."""
    from test_gpu_deep_bvh import deep_scene
    W, H = 37, 23
    s, cam, keep = deep_scene(T)
    ss_ctx.upload(s)
    ss_ctx.set_supersample(2)
    gpx, grgb = ss_ctx.render(cam, abi.make_params(W, H))
    _, hi = oracle_bind.render(s, cam, abi.make_params(2 * W, 2 * H))
    rrgb = ss_ref.resolve(hi, W, H, 2)
    _compare(f"chain of {T}", gpx, grgb, ss_ref.quantize(rrgb), rrgb, exact=True)
    a = ss_ctx.count_work(cam, abi.make_params(W, H))
    assert np.array_equal(a, oracle_bind.count(s, cam, abi.make_params(2 * W, 2 * H)))
    ss_ctx.set_supersample(1)
    del keep


def test_renderer_and_cli_take_the_factor(tmp_path):
    """`Renderer(..., supersample=k)` and `rtx_render --ss K` render the same supersampled frame."""
    import subprocess
    from pathlib import Path
    from gp1_raytracer_2223_amd.renderer import Renderer
    W, H = 37, 23
    rpx, _ = _ref("W4_Bunny", -1.0, W, H, 2)
    r = Renderer(W, H, device=DEV, supersample=2)
    try:
        assert np.array_equal(r.Render(HostScene("W4_Bunny")), rpx)
    finally:
        r.ctx.close()
    exe = Path(abi.LIB_DIR) / "rtx_render"
    out = tmp_path / "shot.bmp"
    subprocess.run([str(exe), "W4_Bunny", str(W), str(H), "--ss", "2", "--out", str(out)], check=True, cwd=tmp_path,
                   timeout=120)
    b = out.read_bytes()
    assert b[:2] == b"BM" and int.from_bytes(b[10:14], "little") == 54
    shot = np.frombuffer(b, np.uint32, W * H, 54).reshape(H, W)[::-1].reshape(-1)   # bottom-up rows
    assert np.array_equal(shot, rpx)


def test_work_counters_count_the_sample_frame(ss_ctx):
    s, cam = gs.view("W4_Bunny")
    ss_ctx.upload(s)
    ss_ctx.set_supersample(2)
    a = ss_ctx.count_work(cam, abi.make_params(64, 48))
    ss_ctx.set_supersample(1)
    b = ss_ctx.count_work(cam, abi.make_params(128, 96))
    assert a[0] == 128 * 96
    assert np.array_equal(a, b), dict(zip(oracle_bind.COUNTER_NAMES, zip(a.tolist(), b.tolist())))


def test_errors_leave_the_factor_and_the_context_intact(ss_ctx):
    W, H = 37, 23
    s, cam = gs.view("W4_Bunny")
    lib, h = ss_ctx.lib, ss_ctx.h
    ss_ctx.upload(s)
    ss_ctx.set_supersample(2)
    for k in (0, 3, 16):
        assert lib.rtx_set_supersample(h, k) == abi.RTX_E_INVALID, k
        assert lib.rtx_last_error(h), k
    rpx, rrgb = _ref("W4_Bunny", -1.0, W, H, 2)
    gpx, grgb = ss_ctx.render(cam, abi.make_params(W, H))      # still 2 x 2
    _compare("after bad factors", gpx, grgb, rpx, rrgb, exact=True)
    ss_ctx.set_supersample(8)
    p = abi.make_params(16384, 16)                             # 131072 samples per row: outside div_rn's domain
    assert lib.rtx_render_async(h, C.byref(cam), C.byref(p), 0) == abi.RTX_E_INVALID
    assert b"65536" in lib.rtx_last_error(h)
    ss_ctx.set_supersample(2)
    gpx, grgb = ss_ctx.render(cam, abi.make_params(W, H))      # the context renders normally afterwards
    _compare("after a refused frame", gpx, grgb, rpx, rrgb, exact=True)
    ss_ctx.set_supersample(1)
