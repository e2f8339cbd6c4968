"""The room skip (csrc/rtx_hip.hip room_clear): waves whose shadow origins lie strictly inside the
room run no shadow-ray room-plane test when every light lies strictly inside it too.  The frames
must be the ones the kernel renders with the skip off (RTX_ROOM_SKIP=0), bit for bit, and the
oracle's, on the catalogue scenes that have the fact and on scenes built so that the fact or the
lane condition fails.  128x72 frames, the size at which test_gpu_parity.py's scene-file cases check
every float."""
import os

import numpy as np
import pytest

import gpu_support as gs
import oracle_bind
from gp1_raytracer_2223_amd import abi
from gp1_raytracer_2223_amd.renderer import DeviceContext
from gp1_raytracer_2223_amd.scene import HostScene
from gpu_support import BUNNY, DEV, ROOM

pytestmark = pytest.mark.gpu

W, H = 128, 72
TOL = 1e-4                                   # test_gpu_parity.py's tolerance where powf runs
POW_FREE = {"W4_Bunny", "Bunny8Lights"}      # Lambert only: bit-exact


def _ctx(**env):
    for k, v in env.items():   # read once, at context creation
        os.environ[k] = v
    try:
        return DeviceContext(DEV)
    finally:
        for k in env:
            del os.environ[k]


@pytest.fixture(scope="module")
def on_ctx():
    ctx = _ctx()
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def off_ctx():
    ctx = _ctx(RTX_ROOM_SKIP="0")
    yield ctx
    ctx.close()


def _same(name, a, b):
    assert np.array_equal(a[0], b[0]), f"{name}: {int((a[0] != b[0]).sum())} pixels differ between skip on and off"
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), f"{name}: colour words differ between skip on and off"


def _vs_oracle(name, gpu, ref, exact):
    (gpx, grgb), (rpx, rrgb) = gpu, ref
    assert not np.isnan(grgb).any()
    d = np.abs(grgb - rrgb)
    assert float(d.max(initial=0.0)) <= TOL, f"{name}: max-abs {d.max()}"
    assert np.abs(gs.channels(gpx) - gs.channels(rpx)).max(initial=0) <= 1, name
    if exact:
        assert np.array_equal(gpx, rpx), f"{name}: {int((gpx != rpx).sum())} pixels differ from the oracle"
        assert np.array_equal(grgb.view(np.uint32), rrgb.view(np.uint32)), \
            f"{name}: {int((grgb != rrgb).sum())} colour values differ from the oracle"


CATALOGUE = [("W3", -1.0), ("W4_Reference", -1.0), ("W4_Bunny", -1.0), ("W4_Bunny", 1.3), ("W4_Optional", -1.0),
             ("Bunny8Lights", -1.0)]


@pytest.mark.parametrize("name,t", CATALOGUE)
def test_catalogue_skip_on_equals_off_and_oracle(on_ctx, off_ctx, name, t):
    hs = HostScene(name)
    if t >= 0:
        hs.update(t)
    s, cam = hs.view()
    p = abi.make_params(W, H)
    on_ctx.upload(s)
    off_ctx.upload(s)
    fact, room_M = on_ctx.room_info()
    assert fact and room_M > 0, (fact, room_M)
    assert off_ctx.room_info() == (False, 0.0)
    on, off = on_ctx.render(cam, p), off_ctx.render(cam, p)
    _same(name, on, off)
    _vs_oracle(name, on, oracle_bind.render(s, cam, p), exact=name in POW_FREE)


# ---- scenes where the fact or the lane condition fails (Lambert only: bit-exact) ---------------

OUTWARD = ["plane 0 0 10   0 0 1  1", "plane 0 0 0    0 -1 0   1", "plane 0 10 0   0 1 0  1",
           "plane 5 0 0   1 0 0   1", "plane -5 0 0   -1 0 0   1"]
INSIDE = ["light point 0 5 5  50 1 0.61 0.45", "light point -2.5 5 -5  70 1 0.8 0.45"]
ONE_ULP = float(np.nextafter(np.float32(5), np.float32(0)))

# name -> (planes, mesh, lights, camera (origin, fov, pitch, yaw) or None, the fact expected)
SCENES = {
    "light_behind_wall": (ROOM, BUNNY, INSIDE + ["light point 6.5 4 3  60 0.6 0.8 1"], None, False),
    "light_on_wall": (ROOM, BUNNY, INSIDE + ["light point 5 4 3  60 0.6 0.8 1"], None, False),
    "light_one_ulp_inside": (ROOM, BUNNY, INSIDE + [f"light point {ONE_ULP!r} 4 3  60 0.6 0.8 1"], None, True),
    # the camera beyond the right wall, looking in through the open side: floor and back-wall
    # points beyond the wall are outside the room
    "camera_outside": (ROOM, BUNNY, INSIDE, ((11.0, 4.0, -9.0), 60.0, 0.0, -0.6), True),
    # ... and behind the back wall, looking at it from behind
    "camera_behind_wall": (ROOM, BUNNY, INSIDE, ((0.5, 4.0, 16.0), 60.0, 0.0, 3.0), True),
    "mesh_through_wall": (ROOM, BUNNY + " translate 4.6 0 2", INSIDE, None, True),
    "normals_outward": (OUTWARD, BUNNY, INSIDE, None, False),
}


def _file_scene(tmp_path, name):
    planes, mesh, lights, camera, fact = SCENES[name]
    path = tmp_path / f"{name}.rtxscene"
    path.write_text("\n".join(["camera 0 3 -9 45", "material lambert 0.49 0.57 0.57 1", "material lambert 1 1 1 1",
                               *planes, mesh, *lights]) + "\n")
    hs = HostScene(f"file:{path}")
    if camera:
        hs.set_camera(*camera)
    return hs, fact


@pytest.mark.parametrize("name", sorted(SCENES))
def test_fact_or_lane_condition_fails(on_ctx, off_ctx, tmp_path, name):
    hs, fact = _file_scene(tmp_path, name)
    s, cam = hs.view()
    p = abi.make_params(W, H)
    on_ctx.upload(s)
    got, room_M = on_ctx.room_info()
    assert got == fact, (name, got, room_M)
    assert (room_M > 0) == fact
    if name == "light_one_ulp_inside":
        assert room_M == 0.5   # 2^20 x one ulp of 5
    on = on_ctx.render(cam, p)
    ref = oracle_bind.render(s, cam, p)
    assert len(np.unique(ref[0])) > 4, "the view shows nothing"
    _vs_oracle(name, on, ref, exact=True)
    off_ctx.upload(s)
    _same(name, on, off_ctx.render(cam, p))


# ---- the other paths that run the light loop ----------------------------------------------------

def test_split_frame_skip_on_equals_off(gpu_ctx):
    """PHASE 3 (the split frame's shading launch) takes the skip too."""
    hs = HostScene("W4_Bunny")
    s, cam = hs.view()
    p = abi.make_params(W, H)
    frames = []
    for env in ({}, {"RTX_ROOM_SKIP": "0"}):
        ctx = _ctx(RTX_SPLIT="force", **env)
        try:
            ctx.upload(s)
            ctx.render(cam, p)                       # the measured frame selects the heavy set
            heavy, parts = ctx.split_info()
            assert parts > 1 and heavy == (W // 8) * (H // 8), (heavy, parts)
            frames.append(ctx.render(cam, p))        # rendered by the split launches
            assert ctx.room_info()[0] == (not env)
        finally:
            ctx.close()
    _same("split", *frames)
    gpu_ctx.upload(s)
    _same("split vs one piece", frames[0], gpu_ctx.render(cam, p))


def test_supersampled_frame_skip_on_equals_off(on_ctx, off_ctx):
    hs = HostScene("W4_Bunny")
    s, cam = hs.view()
    p = abi.make_params(W, H)
    frames = []
    for ctx in (on_ctx, off_ctx):
        ctx.upload(s)
        ctx.set_supersample(2)
        try:
            frames.append(ctx.render(cam, p))
        finally:
            ctx.set_supersample(1)
    _same("2x2", *frames)


def test_corner_seam(on_ctx, off_ctx):
    """The camera near the floor / left-wall corner, looking along it: tiles straddle the seam, and the
    shadow origins on either side lie 1e-4 from their own plane and almost on the other."""
    hs = HostScene("W4_Bunny")
    hs.set_camera((-4.6, 0.4, -3.0), 60.0, -0.05, -0.04)
    s, cam = hs.view()
    p = abi.make_params(W, H)
    on_ctx.upload(s)
    assert on_ctx.room_info()[0]
    on = on_ctx.render(cam, p)
    ref = oracle_bind.render(s, cam, p)
    assert len(np.unique(ref[0])) > 4, "the view shows nothing"
    _vs_oracle("corner", on, ref, exact=True)
    off_ctx.upload(s)
    _same("corner", on, off_ctx.render(cam, p))
