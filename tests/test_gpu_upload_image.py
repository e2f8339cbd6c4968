"""The upload on the device against the pins of tests/golden/pack_pins.json (tests/pack_cases.py;
tests/test_pack_cpu.py holds the packer to the same pins on the CPU): one scene per octant regime, the
registration layout of the device Update, and the image rotation an upload and an Update share."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import pack_cases as PC
from gp1_raytracer_2223_amd import abi
from gp1_raytracer_2223_amd.renderer import DeviceAnimation, DeviceContext
from gp1_raytracer_2223_amd.scene import HostScene

pytestmark = pytest.mark.gpu

CASES = {c.label: c for c in PC.cases()}
PINNED = json.loads(PC.PINS.read_text())


# W4_Bunny: 11 KB of nodes a copy, 8 host copies; W4_Optional: 115 KB, the device writes copies 1..7;
# Synthetic100k: above kOctantMaxNodeBytes, one copy; opt_reserve: rtx_anim_create's registration upload
@pytest.mark.parametrize("label", ["W4_Bunny", "W4_Optional", "Synthetic100k", "opt_reserve"])
def test_uploaded_image_equals_the_pins(label, tmp_path):
    img, facts = PC.device_image(CASES[label], tmp_path)
    pin = PINNED[label]
    assert facts == {k: pin[k] for k in facts}
    assert img.size == pin["total"] and PC.sha256(img) == pin["sha256"]
    if img.size < 2 << 20:   # (the CPU test holds the packer to every FNV; in Python it is ~0.2 s per MB)
        assert PC.fnv(img) == pin["img"]


def state(ctx, cam):
    nb = C.c_uint64(0)
    abi.check(ctx.lib.rtx_scene_bytes(ctx.h, C.byref(nb)), "rtx_scene_bytes")
    px, _ = ctx.render(cam, abi.make_params(64, 48))
    return int(nb.value), ctx.spec_info(), px, PC.read_image(ctx)


def test_an_upload_after_a_device_update_equals_a_fresh_one():
    """The next image and its adoption are one pair of functions for rtx_upload_scene and
    rtx_anim_update: a context that registered W4_Optional, updated it once on the device and was then
    given W4_Bunny holds what a fresh context given W4_Bunny holds."""
    bunny = HostScene("W4_Bunny")
    s, cam = bunny.view()
    device = int(os.environ.get("RTX_TEST_DEVICE", "0"))
    used, fresh = DeviceContext(device), DeviceContext(device)
    optional = HostScene("W4_Optional")
    anim = DeviceAnimation(optional, used)
    anim.update(1.3, used)
    used.upload(s)
    fresh.upload(s)
    a, b = state(used, cam), state(fresh, cam)
    anim.close()
    used.close()
    fresh.close()
    assert a[0] == b[0] == PINNED["W4_Bunny"]["total"] and a[1] == b[1]
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
