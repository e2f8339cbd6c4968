"""The incremental shadow pass (include/rtx.h: rtx_update_shadows_async, rtx_refresh_shadows_async) without a GPU:
the entry points are declared, exported and bound and refuse a NULL context without a device; the C++ mirror
compiles; the command-line program refuses a malformed --move-light before any device work; and the claim the
feature rests on, on the checker alone: bit l of the plane depends only on the hit record and on light l's origin
and type, so the planes of two scenes agree in every bit whose light kept its key."""
import ctypes as C

import numpy as np
import pytest

import abi_surface
import relight_ref
import shadow_update_scenes as sus
from checkers import checker  # noqa: F401
from gp1_raytracer_2223_amd import abi
from gp1_raytracer_2223_amd.scene import HostScene

W, H = 37, 23


def test_header_declares_and_abi_binds_the_symbols(tmp_path):
    abi_surface.declared_exported_and_bound(tmp_path, {
        "rtx_update_shadows_async": "int (*)(rtx_ctx*, uint32_t)",
        "rtx_refresh_shadows_async": "int (*)(rtx_ctx*, uint32_t*)",
    }, {"rtx_time_shadows_update": "int (*)(rtx_ctx*, uint32_t, int, float*)"}, ["RTX_ABI_VERSION == 2"])
    lib = abi.load_hip()
    assert lib.rtx_abi_version() == 2
    assert lib.rtx_update_shadows_async.argtypes[1:] == [C.c_uint32]
    assert lib.rtx_refresh_shadows_async.argtypes[1]._type_ is C.c_uint32
    assert lib.rtx_time_shadows_update.argtypes[1:3] == [C.c_uint32, C.c_int]


def test_null_context_is_invalid_without_a_device():
    lib = abi.load_hip()
    traced, ms = C.c_uint32(), C.c_float()
    assert lib.rtx_update_shadows_async(None, 1) == abi.RTX_E_INVALID
    assert lib.rtx_update_shadows_async(None, 0) == abi.RTX_E_INVALID
    assert lib.rtx_refresh_shadows_async(None, C.byref(traced)) == abi.RTX_E_INVALID
    assert lib.rtx_refresh_shadows_async(None, None) == abi.RTX_E_INVALID
    assert lib.rtx_time_shadows_update(None, 1, 1, C.byref(ms)) == abi.RTX_E_INVALID
    assert lib.rtx_time_shadows_update(None, 1, 0, C.byref(ms)) == abi.RTX_E_INVALID
    assert lib.rtx_time_shadows_update(None, 1, 1, None) == abi.RTX_E_INVALID


def test_the_cpp_mirror_compiles(tmp_path):
    abi_surface.cpp_mirror_compiles(tmp_path, [("std::vector<uint32_t> (rtx::Renderer::*)(uint32_t)", "UpdateShadows"),
                                               ("std::vector<uint32_t> (rtx::Renderer::*)(uint32_t*)", "RefreshShadows")])


@pytest.mark.parametrize("arg", [None, "", "1", "1,2,3", "1,2,3,4,5", "x,1,2,3", "1,a,2,3", "-1,0,0,0", "1,2,3,4x",
                                 "3,0,0,0", "99,1,1,1"],
                         ids=["missing", "empty", "one", "three", "five", "no_index", "no_number", "negative", "tail",
                              "light_3_of_3", "light_99"])
@pytest.mark.parametrize("relight", [False, True])
def test_cli_refuses_a_bad_move_light_before_device_work(tmp_path, arg, relight):
    """(W4_Bunny has three lights: 3 and 99 name none.)"""
    args = ["--move-light"] + ([arg] if arg is not None else [])
    if relight:
        args = ["--relight", "--aov", "planes"] + args
    abi_surface.cli_refuses(tmp_path, "--move-light", args)


def test_host_light_set_origin():
    hs = HostScene("W4_Bunny")
    lib = abi.load_host()
    o = (C.c_float * 3)(1.5, 6.0, 3.0)
    assert lib.rtx_host_light_set_origin(hs._h, 3, o) == abi.RTX_E_INVALID
    assert lib.rtx_host_light_set_origin(hs._h, 0, None) == abi.RTX_E_INVALID
    assert lib.rtx_host_light_set_origin(None, 0, o) == abi.RTX_E_INVALID
    before = sus.light_keys(hs.view()[0])
    assert lib.rtx_host_light_set_origin(hs._h, 2, o) == abi.RTX_OK
    after = sus.light_keys(hs.view()[0])
    assert sus.dirty_mask(before, after) == 0b100
    assert list(hs.view()[0].lights[2].origin) == [1.5, 6.0, 3.0]


# ---- bit l depends on light l alone ----------------------------------------------------------------------

# The words that differ per bit, as the checker counted them when the scenes were chosen: {variant: {bit: count}}
COUNTS = {
    "room": {"move0": {0: 14}, "move1_out": {1: 820}, "move12": {1: 62, 2: 103}, "type2": {2: 695}, "added": {3: 90},
             "removed": {2: 56}},
    "open": {"move0": {0: 60}, "move1_out": {1: 109}, "move12": {1: 102, 2: 144}, "type2": {2: 632}, "added": {3: 148},
             "removed": {2: 73}},
}


@pytest.mark.parametrize("geometry", ["room", "open"])
def test_a_bit_depends_on_its_own_light_only(checker, tmp_path, geometry):
    base = sus.file_scene(tmp_path, geometry, "base")
    s0, cam0 = base.view()
    bits0, hit0 = relight_ref.plane(checker, s0, cam0, W, H)
    assert int(hit0.sum()) == 851
    keys0 = sus.light_keys(s0)
    for name, (_, may_change) in sus.VARIANTS.items():
        if name == "base":
            continue
        hs = sus.file_scene(tmp_path, geometry, name)
        s, cam = hs.view()
        assert bytes(cam) == bytes(cam0)
        bits, hit = relight_ref.plane(checker, s, cam, W, H)
        if s.n_lights:
            assert np.array_equal(hit, hit0)
        for l in range(s.n_lights):   # every light decides something in every variant
            b = ((bits >> np.uint32(l)) & 1)[hit]
            assert b.any() and not b.all(), (geometry, name, l)
        # the lights whose key changed, from the light arrays: the bits the variant is meant to touch
        n_min = min(s.n_lights, s0.n_lights)
        dirty = sus.dirty_mask(keys0, sus.light_keys(s)) | sum(1 << l for l in range(s.n_lights, s0.n_lights))
        assert dirty == may_change, (geometry, name, bin(dirty))
        changed = sus.changed_per_bit(bits, bits0, 4)
        for l in range(4):
            if (may_change >> l) & 1:
                assert changed[l] > 0, (geometry, name, l)
            else:
                assert changed[l] == 0, (geometry, name, l, changed[l])
        assert {l: c for l, c in enumerate(changed) if c} == COUNTS[geometry][name], (geometry, name, changed)
        assert n_min >= 2
