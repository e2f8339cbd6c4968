"""Adaptive supersampling (rtx_render_adaptive*: rtx_classify_kernel, rtx_adaptive_kernel) on the GPU.

The expected frame is always compose(P, S, edges(P)) of tests/adaptive_ref.py with P (factor 1) and S
(rtx_set_supersample) rendered through the existing API on the same device, compared with array_equal on
the uint32 plane and on the float plane viewed as uint32; on pow-free scenes it is compared with the
oracle's composition as well.  Every parity case also asserts 0 < |E| < W * H and adaptive_refined() ==
|E|, so a frame that refines nothing or everything cannot pass as parity."""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import adaptive_ref
import gpu_support as gs
import oracle_bind
from gp1_raytracer_2223_amd import abi
from gp1_raytracer_2223_amd.renderer import AOV_ALL, DeviceContext, Renderer, aov_host_planes
from gp1_raytracer_2223_amd.scene import HostScene
from gpu_support import DEV
from test_gpu_parity import POW_FREE

pytestmark = pytest.mark.gpu

XRGB = adaptive_ref.XRGB8888
W0, H0 = 37, 23   # k = 2: 74 x 46 samples, neither a multiple of the 8 x 8 wave tile


@pytest.fixture(scope="module")
def ad_ctx():
    """The context the adaptive frames are rendered on."""
    ctx = DeviceContext(DEV)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def ref_ctx():
    """The context P and S come from (the existing API; its factor is changed and put back)."""
    ctx = DeviceContext(DEV)
    yield ctx
    ctx.close()


_device = {}
_oracle = {}


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def _device_ps(ref_ctx, key, s, cam, W, H, k, mode=3, shadows=1, fmt=XRGB):
    """(P, S) = ((px, rgb), (px, rgb)) of the device's own plain and supersampled frames, once per case."""
    key = (key, W, H, k, mode, shadows, fmt)
    if key not in _device:
        p = abi.make_params(W, H, mode, shadows, fmt)
        ref_ctx.upload(s)
        ref_ctx.set_supersample(1)
        P = _frozen(*ref_ctx.render(cam, p))
        ref_ctx.set_supersample(k)
        try:
            S = _frozen(*ref_ctx.render(cam, p))
        finally:
            ref_ctx.set_supersample(1)
        _device[key] = (P, S)
    return _device[key]


def _oracle_ps(key, s, cam, W, H, k, mode=3, shadows=1, fmt=XRGB):
    key = (key, W, H, k, mode, shadows, fmt)
    if key not in _oracle:
        _, prgb = oracle_bind.render(s, cam, abi.make_params(W, H, mode, shadows))
        _, hi = oracle_bind.render(s, cam, abi.make_params(k * W, k * H, mode, shadows))
        import ss_ref
        P = _frozen(ss_ref.quantize(prgb, fmt), prgb)
        S = _frozen(*adaptive_ref.supersampled(hi, W, H, k, fmt))
        _oracle[key] = (P, S)
    return _oracle[key]


def _compose(P, S, W, H, tau, fmt=XRGB):
    E = adaptive_ref.edges(P[0], W, H, tau, fmt)
    return adaptive_ref.compose(P[0], S[0], E), adaptive_ref.compose(P[1], S[1], E), E


def _same(got, want, what):
    px, rgb = got
    wpx, wrgb = want[0], want[1]
    assert np.array_equal(px, wpx), f"{what}: {(px != wpx).sum()} pixels differ"
    if rgb is not None:
        assert np.array_equal(rgb.view(np.uint32), wrgb.view(np.uint32)), \
            f"{what}: {(rgb.view(np.uint32) != wrgb.view(np.uint32)).sum()} colour words differ"


def _parity(ad_ctx, ref_ctx, name, t, W, H, k, tau, mode=3, shadows=1, fmt=XRGB, exact=None, s_cam=None, partial=True):
    """One adaptive frame against the device's own composition (and the oracle's where `exact`)."""
    s, cam = s_cam if s_cam is not None else gs.view(name, t)
    P, S = _device_ps(ref_ctx, (name, t), s, cam, W, H, k, mode, shadows, fmt)
    wpx, wrgb, E = _compose(P, S, W, H, tau, fmt)
    n = int(E.sum())
    print(f"{name} t{t} {W}x{H} k{k} tau{tau} m{mode}s{shadows}: |E| = {n} of {W * H}")
    ad_ctx.upload(s)
    got = ad_ctx.render_adaptive(cam, abi.make_params(W, H, mode, shadows, fmt), k, tau)
    refined = ad_ctx.adaptive_refined()
    if partial:
        assert 0 < n < W * H, (n, W * H)
    assert refined == n, (refined, n)
    _same(got, (wpx, wrgb), f"{name}/k{k}/tau{tau} against the device's P and S")
    if exact if exact is not None else name in POW_FREE:
        oP, oS = _oracle_ps((name, t), s, cam, W, H, k, mode, shadows, fmt)
        opx, orgb, oE = _compose(oP, oS, W, H, tau, fmt)
        assert np.array_equal(oE, E)
        _same(got, (opx, orgb), f"{name}/k{k}/tau{tau} against the oracle's composition")
    return got, E


PARITY = [(n, -1.0, k, 32) for n in ("W4_Bunny", "W2", "W3") for k in (2, 4, 8)] + \
         [("W4_Bunny", -1.0, 4, 8), ("W4_Bunny", 1.3, 2, 32)]
# the oracle's mask sizes of tests/test_adaptive_cpu.py: 87 = 5 * 16 + 7 = 21 * 4 + 3 leaves a partial tail
# wave at k = 2 (16 pixels a wave) and at k = 4 (4 a wave), 452 = 28 * 16 + 4 at k = 2
SIZES = {("W4_Bunny", -1.0, 32): 87, ("W2", -1.0, 32): 452}


@pytest.mark.parametrize("name,t,k,tau", PARITY)
def test_parity(ad_ctx, ref_ctx, name, t, k, tau):
    _, E = _parity(ad_ctx, ref_ctx, name, t, W0, H0, k, tau)
    if (name, t, tau) in SIZES:
        assert int(E.sum()) == SIZES[(name, t, tau)]
        assert k != 2 or int(E.sum()) % 16 != 0   # (the tail wave is partial)


@pytest.mark.parametrize("k", [2, 4, 8])
def test_threshold_0_is_the_supersampled_frame(ad_ctx, ref_ctx, k):
    """Every pixel of this frame differs from a neighbour: the list is W * H long and A = S."""
    s, cam = gs.view("W4_Bunny")
    P, S = _device_ps(ref_ctx, ("W4_Bunny", -1.0), s, cam, W0, H0, k)
    assert adaptive_ref.edges(P[0], W0, H0, 0).all()
    ad_ctx.upload(s)
    got = ad_ctx.render_adaptive(cam, abi.make_params(W0, H0), k, 0)
    assert ad_ctx.adaptive_refined() == W0 * H0
    _same(got, S, f"tau 0, k {k}")
    oP, oS = _oracle_ps(("W4_Bunny", -1.0), s, cam, W0, H0, k)
    _same(got, oS, f"tau 0, k {k}, oracle")


def test_threshold_255_is_the_plain_frame(ad_ctx, ref_ctx):
    s, cam = gs.view("W4_Bunny")
    P, _ = _device_ps(ref_ctx, ("W4_Bunny", -1.0), s, cam, W0, H0, 2)
    ad_ctx.upload(s)
    ad_ctx.render_adaptive(cam, abi.make_params(W0, H0), 2, 0)     # (a full list first: nothing of it may be used)
    got = ad_ctx.render_adaptive(cam, abi.make_params(W0, H0), 4, 255)
    assert ad_ctx.adaptive_refined() == 0
    _same(got, P, "tau 255")


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("shadows", [0, 1])
def test_modes_and_shadows(ad_ctx, ref_ctx, mode, shadows):
    _parity(ad_ctx, ref_ctx, "W3", -1.0, 40, 30, 2, 32, mode, shadows, exact=mode in (0, 1))


def test_without_the_colour_plane(ref_ctx):
    """want_rgb = 0 on a context that never had a colour plane: the refinement stores pixels only."""
    s, cam = gs.view("W4_Bunny")
    P, S = _device_ps(ref_ctx, ("W4_Bunny", -1.0), s, cam, W0, H0, 4)
    wpx, _, E = _compose(P, S, W0, H0, 32)
    ctx = DeviceContext(DEV)
    try:
        ctx.upload(s)
        px, rgb = ctx.render_adaptive(cam, abi.make_params(W0, H0), 4, 32, want_rgb=False)
        assert rgb is None and ctx.device_buffers()[1] == 0
        assert ctx.adaptive_refined() == int(E.sum()) and 0 < int(E.sum()) < W0 * H0
        assert np.array_equal(px, wpx), f"{(px != wpx).sum()} pixels differ"
    finally:
        ctx.close()


# {0, 8, 16, 0xFF000000}: the channels in another order under a constant alpha; {24, 16, 8, 0xFF}: a channel in
# bits 24-31, where a classifier reading fixed shifts 16 / 8 / 0 would see green, blue and the constant alpha
@pytest.mark.parametrize("fmt", [(0, 8, 16, 0xFF000000), (24, 16, 8, 0x000000FF)])
def test_pixel_format(ad_ctx, ref_ctx, fmt):
    got, E = _parity(ad_ctx, ref_ctx, "W4_Bunny", -1.0, W0, H0, 2, 32, fmt=fmt)
    assert ((got[0] & np.uint32(fmt[3])) == np.uint32(fmt[3])).all()
    assert int(E.sum()) == 87   # (the same channels as XRGB8888's, so the same mask)


def test_few_waves_stride_over_the_list(ref_ctx):
    """RTX_ADAPTIVE_WAVES=4: 1,976 one-pixel items (k = 8) over four waves, 494 steps each."""
    os.environ["RTX_ADAPTIVE_WAVES"] = "4"
    try:
        ctx = DeviceContext(DEV)
    finally:
        del os.environ["RTX_ADAPTIVE_WAVES"]
    try:
        _, E = _parity(ctx, ref_ctx, "W4_Bunny", -1.0, 160, 120, 8, 8)
        assert int(E.sum()) == 1976
    finally:
        ctx.close()


@pytest.mark.parametrize("T", [300, 1100])
def test_deep_stack_variants(ad_ctx, ref_ctx, T):
    """T = 300: the deep LDS stack; 1100: the stacks in HBM, one per persistent wave."""
    from test_gpu_deep_bvh import deep_scene
    s, cam, keep = deep_scene(T)
    _parity(ad_ctx, ref_ctx, f"chain{T}", -1.0, W0, H0, 2, 32, exact=True, s_cam=(s, cam))
    del keep


def test_split_frames_and_context_state(ref_ctx):
    W, H, k, tau = 64, 48, 2, 32
    os.environ["RTX_SPLIT"] = "force"
    try:
        ctx = DeviceContext(DEV)
    finally:
        del os.environ["RTX_SPLIT"]
    try:
        s, cam = gs.view("W4_Bunny")
        p = abi.make_params(W, H)
        P, S = _device_ps(ref_ctx, ("W4_Bunny", -1.0), s, cam, W, H, k)
        want = _compose(P, S, W, H, tau)
        assert 0 < int(want[2].sum()) < W * H
        ctx.upload(s)
        # a hit pass before the adaptive frames reads back unchanged after them
        before = ctx.render_aov(cam, p, AOV_ALL)
        first = ctx.render_adaptive(cam, p, k, tau)          # its plain frame is measured: selects the heavy set
        heavy, parts = ctx.split_info()
        assert parts > 1 and heavy == (W // 8) * (H // 8), (heavy, parts)
        ctx.render_adaptive(cam, p, k, tau)
        third = ctx.render_adaptive(cam, p, k, tau)          # its plain frame is the split launches'
        assert ctx.adaptive_refined() == int(want[2].sum())
        _same(first, want, "adaptive frame 1")
        _same(third, want, "adaptive frame 3 (after split launches)")
        # queued without a host wait in between, the classifier still sees the joined chain's pixels
        for _ in range(3):
            ctx.render_adaptive_async(cam, p, k, tau, want_rgb=True)
        px, rgb = np.zeros(W * H, np.uint32), np.zeros(3 * W * H, np.float32)
        abi.check(ctx.lib.rtx_download(ctx.h, px.ctypes.data_as(C.POINTER(C.c_uint32)),
                                       rgb.ctypes.data_as(C.POINTER(C.c_float))), "rtx_download", ctx.h)
        _same((px, rgb), want, "three queued adaptive frames")
        after = ctx.download_aov(aov_host_planes(W, H, AOV_ALL))
        for name in before:
            assert np.array_equal(before[name].view(np.uint32), after[name].view(np.uint32)), name
        # a plain frame afterwards is a fresh context's
        _same(ctx.render(cam, p), P, "a plain frame after adaptive frames")
        # after uploading another scene the adaptive frame is that scene's
        s2, cam2 = gs.view("W2")
        P2, S2 = _device_ps(ref_ctx, ("W2", -1.0), s2, cam2, W, H, k)
        want2 = _compose(P2, S2, W, H, tau)
        ctx.upload(s2)
        _same(ctx.render_adaptive(cam2, p, k, tau), want2, "another scene")
        assert ctx.adaptive_refined() == int(want2[2].sum()) and not np.array_equal(want2[0], want[0])
    finally:
        ctx.close()


def test_errors_leave_the_context_rendering(ref_ctx):
    s, cam = gs.view("W4_Bunny")
    P, S = _device_ps(ref_ctx, ("W4_Bunny", -1.0), s, cam, W0, H0, 2)
    want = _compose(P, S, W0, H0, 32)
    ctx = DeviceContext(DEV)
    lib, h = ctx.lib, ctx.h
    px = np.zeros(W0 * H0, np.uint32)
    pp = px.ctypes.data_as(C.POINTER(C.c_uint32))
    n = C.c_uint32()

    def call(p, k=2, tau=32, cam_=cam):
        return lib.rtx_render_adaptive_async(h, C.byref(cam_) if cam_ is not None else None,
                                             C.byref(p) if p is not None else None, 1, k, tau)

    def still_renders(what):
        _same(ctx.render_adaptive(cam, abi.make_params(W0, H0), 2, 32), want, f"after {what}")

    try:
        good = abi.make_params(W0, H0)
        # no scene uploaded, no adaptive frame yet
        assert call(good) == abi.RTX_E_STATE and lib.rtx_last_error(h)
        assert lib.rtx_adaptive_refined(h, C.byref(n)) == abi.RTX_E_STATE
        ctx.upload(s)
        still_renders("no scene")
        # k not in {2, 4, 8}; tau > 255
        for k in (0, 1, 3, 16):
            assert call(good, k=k) == abi.RTX_E_INVALID, k
        assert call(good, tau=256) == abi.RTX_E_INVALID and b"255" in lib.rtx_last_error(h)
        still_renders("a bad factor and threshold")
        # anything rtx_render rejects
        assert call(None) == abi.RTX_E_INVALID and call(good, cam_=None) == abi.RTX_E_INVALID
        assert lib.rtx_render_adaptive(h, C.byref(cam), C.byref(good), 2, 32, None, None) == abi.RTX_E_INVALID
        assert lib.rtx_adaptive_refined(h, None) == abi.RTX_E_INVALID
        for bad in (abi.make_params(0, H0), abi.make_params(W0, 0), abi.make_params(W0, H0, mode=4),
                    abi.make_params(W0, H0, mode=-1), abi.make_params(W0, H0, fmt=(25, 8, 0, 0)),
                    abi.make_params(W0, H0, stripe_rows=8, stripe_first=0, stripe_step=2),
                    abi.make_params(W0, H0, stripe_rows=16, stripe_first=2, stripe_step=2)):
            assert lib.rtx_render_async(h, C.byref(cam), C.byref(bad), 0) == abi.RTX_E_INVALID
            assert call(bad) == abi.RTX_E_INVALID
        still_renders("parameters rtx_render rejects")
        # k * width or k * height above 65536 (each inside a plain frame's limit)
        assert call(abi.make_params(16384, 16), k=8) == abi.RTX_E_INVALID and b"65536" in lib.rtx_last_error(h)
        assert call(abi.make_params(16, 32769), k=2) == abi.RTX_E_INVALID
        still_renders("a sample frame beyond 65536")
        # a context factor other than 1; stripes
        ctx.set_supersample(2)
        assert call(good) == abi.RTX_E_UNSUPPORTED and lib.rtx_last_error(h)
        ctx.set_supersample(1)
        assert call(abi.make_params(W0, H0, stripe_rows=16, stripe_first=0, stripe_step=2)) == abi.RTX_E_UNSUPPORTED
        assert call(abi.make_params(W0, H0, stripe_rows=16, stripe_first=0, stripe_step=1)) == abi.RTX_OK   # (not striped)
        still_renders("a supersampled context and a striped frame")
        assert ctx.adaptive_refined() == int(want[2].sum())
        assert lib.rtx_time_adaptive_frames(h, C.byref(cam), C.byref(good), 2, 32, 0, C.byref(C.c_float())) == abi.RTX_E_INVALID
        assert ctx.time_adaptive_frames(cam, good, 2, 32, 2) > 0.0
        assert lib.rtx_download(h, pp, None) == abi.RTX_OK and np.array_equal(px, want[0])   # (the timed frames' too)
    finally:
        ctx.close()


def test_renderer_and_cli_take_the_mode(ref_ctx, tmp_path):
    """`Renderer(..., adaptive=(k, tau))`, `Renderer.RenderAdaptive` and `rtx_render --adaptive 2,32`."""
    s, cam = gs.view("W4_Bunny")
    P, S = _device_ps(ref_ctx, ("W4_Bunny", -1.0), s, cam, W0, H0, 2)
    wpx, wrgb, E = _compose(P, S, W0, H0, 32)
    r = Renderer(W0, H0, device=DEV, adaptive=(2, 32))
    try:
        hs = HostScene("W4_Bunny")
        assert np.array_equal(r.Render(hs, want_rgb=True), wpx)
        assert np.array_equal(r.rgb.view(np.uint32), wrgb.view(np.uint32))
        assert r.ctx.adaptive_refined() == int(E.sum())
        r.adaptive = None
        assert np.array_equal(r.Render(hs, upload=False), P[0])
        assert np.array_equal(r.RenderAdaptive(hs, 2, 32, upload=False), wpx)
    finally:
        r.ctx.close()
    exe = Path(abi.LIB_DIR) / "rtx_render"
    out = tmp_path / "shot.bmp"
    done = subprocess.run([str(exe), "W4_Bunny", str(W0), str(H0), "--adaptive", "2,32", "--out", str(out)], check=True,
                          cwd=tmp_path, timeout=120, capture_output=True, text=True)
    assert f"refined {int(E.sum())} of {W0 * H0} pixels" in done.stdout
    b = out.read_bytes()
    assert b[:2] == b"BM" and int.from_bytes(b[10:14], "little") == 54
    shot = np.frombuffer(b, np.uint32, W0 * H0, 54).reshape(H0, W0)[::-1].reshape(-1)   # bottom-up rows
    assert np.array_equal(shot, wpx)
