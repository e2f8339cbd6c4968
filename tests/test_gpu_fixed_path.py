"""The fixed path of the render kernel (csrc/rtx_hip.hip render_tile outside the walks: the camera's room
planes, the hit record, the light loop's set-up) on the smallest frames that hold every case: 8 x 8 and
16 x 8 frames (one and two waves) of a five-plane room with a one-triangle mesh and three lights, Lambert
only and with a Cook-Torrance triangle, from cameras whose waves hit only planes, only the triangle, and
both.  Against the oracle and against an RTX_NO_SPEC=1 context (the generic kernel)."""
import numpy as np
import pytest
import torch   # noqa: F401  (at collection, before librtx_hip.so is loaded)

import aov_ref
import oracle_bind
import ray_domains as RD
from checkers import checker  # noqa: F401
from gp1_raytracer_2223_amd import abi
from gpu_support import ctx  # noqa: F401
from ray_domains import generic_ctx  # noqa: F401

pytestmark = pytest.mark.gpu

TOL = 1e-4   # test_gpu_parity.py's tolerance where powf runs (the Cook-Torrance triangle)
WANT = {"mix": (True, True), "tri": (False, True), "planes": (True, False)}   # camera -> (planes hit, triangle hit)


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    d = tmp_path_factory.mktemp("fp_scenes")
    return {k: RD.room_scene(d, k) for k in RD.ROOM_MATS}


def _words(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("W,H", [(8, 8), (16, 8)])
@pytest.mark.parametrize("camera", sorted(RD.ROOM_CAMERAS))
@pytest.mark.parametrize("kind", sorted(RD.ROOM_MATS))
def test_room_frames(ctx, generic_ctx, checker, scenes, kind, camera, W, H):
    hs = scenes[kind]
    hs.set_camera(*RD.ROOM_CAMERAS[camera])
    s, cam = hs.view()
    # every wave of the frame is what the camera is for: all planes, all triangle, or both (the checker's hit pass)
    prim = np.asarray(aov_ref.planes(checker, s, cam, W, H)["primitive"]) >> 30
    for lanes in RD.wave_lanes(W, H):
        assert ((prim[lanes] == 2).any(), (prim[lanes] == 3).any()) == WANT[camera], camera
        assert (prim[lanes] != 0).all()
    ctx.upload(s)
    generic_ctx.upload(s)
    for mode, sh in ((abi.RTX_MODE_COMBINED, 1), (abi.RTX_MODE_COMBINED, 0), (abi.RTX_MODE_OBSERVED_AREA, 1),
                     (abi.RTX_MODE_BRDF, 1)):
        p = abi.make_params(W, H, mode, sh)
        gpx, grgb = ctx.render(cam, p)
        if (mode, sh) == (abi.RTX_MODE_COMBINED, 1):   # the specialised variants: Lambert only, and with Cook-Torrance
            assert ctx.spec_info()[1] == (0 if kind == "lambert" else 1), ctx.spec_info()
        npx, nrgb = generic_ctx.render(cam, p)
        assert generic_ctx.spec_info()[1] == -1
        what = f"{kind}/{camera} {W}x{H} mode {mode} shadows {sh}"
        assert np.array_equal(gpx, npx) and _words(grgb, nrgb), f"{what}: the specialised and the generic kernel differ"
        rpx, rrgb = oracle_bind.render(s, cam, p)
        if kind == "lambert" or mode == abi.RTX_MODE_OBSERVED_AREA:
            assert np.array_equal(gpx, rpx) and _words(grgb, rrgb), f"{what}: {int((gpx != rpx).sum())} pixels differ from the oracle"
        else:
            assert not np.isnan(grgb).any()
            assert float(np.abs(grgb - rrgb).max(initial=0.0)) <= TOL, what
