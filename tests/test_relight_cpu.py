"""Relighting (include/rtx.h: rtx_render_shadows_async, rtx_relight) without a GPU: the entry points are declared,
exported and bound and refuse a NULL context without a device; the C++ mirror compiles; the command-line program
refuses --relight in a bad combination before any device work; the checker tests/relight_ref.c, which shades from
(ray, t, normal, material, primitive) plus one occlusion bit per light, equals tests/shade_ref.c on the same rays
word for word when the bits are Scene::DoesHit's answers; and the new kernels' code-object metadata: the shadow
pass (PHASE 9) is instantiated where deferred shading (PHASE 8) is, nothing uses scratch, and the relight kernel
uses no LDS."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import abi_surface
import aov_ref
import rayq_ref
import relight_ref
import scene_fuzz
import shade_ref
from checkers import checker  # noqa: F401
from gp1_raytracer_2223_amd import abi
from gp1_raytracer_2223_amd.scene import HostScene

W, H = 37, 23
PIN = ["W4_Bunny", "W3", "W4_Reference", "W1"]


def test_header_declares_and_abi_binds_the_symbols(tmp_path):
    """Every entry point is declared as the contract states it, exported and bound, and the ABI version stays 2."""
    abi_surface.declared_exported_and_bound(tmp_path, {
        "rtx_render_shadows_async": "int (*)(rtx_ctx*)",
        "rtx_download_shadows": "int (*)(rtx_ctx*, uint32_t*)",
        "rtx_gather_shadows_async": "int (*)(rtx_ctx*, uint32_t*)",
        "rtx_device_shadow_buffer": "int (*)(rtx_ctx*, uint32_t**)",
        "rtx_relight_async": "int (*)(rtx_ctx*, const rtx_render_params*, int)",
        "rtx_relight": "int (*)(rtx_ctx*, const rtx_render_params*, uint32_t*, float*)",
    }, {
        "rtx_time_shadows": "int (*)(rtx_ctx*, int, float*)",
        "rtx_time_relight": "int (*)(rtx_ctx*, const rtx_render_params*, int, int, float*)",
    }, ["RTX_ABI_VERSION == 2", "RTX_AOV_ALL == 15"])
    lib = abi.load_hip()
    assert lib.rtx_abi_version() == 2
    a = lib.rtx_relight.argtypes
    assert a[1]._type_ is abi.RenderParams and a[2]._type_ is C.c_uint32 and a[3]._type_ is C.c_float
    assert lib.rtx_relight_async.argtypes[2:] == [C.c_int]
    assert lib.rtx_download_shadows.argtypes[1]._type_ is C.c_uint32


def test_null_context_is_invalid_without_a_device():
    lib = abi.load_hip()
    p = abi.make_params(8, 8)
    px = np.zeros(64, np.uint32)
    up = px.ctypes.data_as(C.POINTER(C.c_uint32))
    d = C.POINTER(C.c_uint32)()
    ms = C.c_float()
    assert lib.rtx_render_shadows_async(None) == abi.RTX_E_INVALID
    assert lib.rtx_download_shadows(None, up) == abi.RTX_E_INVALID
    assert lib.rtx_gather_shadows_async(None, up) == abi.RTX_E_INVALID
    assert lib.rtx_device_shadow_buffer(None, C.byref(d)) == abi.RTX_E_INVALID
    assert lib.rtx_relight_async(None, C.byref(p), 0) == abi.RTX_E_INVALID
    assert lib.rtx_relight(None, C.byref(p), up, None) == abi.RTX_E_INVALID
    assert lib.rtx_time_shadows(None, 1, C.byref(ms)) == abi.RTX_E_INVALID
    assert lib.rtx_time_relight(None, C.byref(p), 0, 1, C.byref(ms)) == abi.RTX_E_INVALID
    assert lib.rtx_time_relight(None, C.byref(p), 0, 1, None) == abi.RTX_E_INVALID


def test_the_cpp_mirror_compiles(tmp_path):
    abi_surface.cpp_mirror_compiles(tmp_path, [("std::vector<uint32_t> (rtx::Renderer::*)()", "RenderShadows"),
                                               ("void (rtx::Renderer::*)()", "Relight")])


@pytest.mark.parametrize("extra", [["--ss", "2"], ["--adaptive", "2,32"], ["--rays", "rays.f32"], ["--benchmark"],
                                   ["--benchmark", "2"], ["--sequence", "0.5,1.0"], ["--deferred"]],
                         ids=["ss", "adaptive", "rays", "benchmark", "benchmark_n", "sequence", "deferred"])
def test_cli_refuses_relight_in_a_bad_combination_before_device_work(tmp_path, extra):
    abi_surface.cli_refuses(tmp_path, "--relight", ["--relight"] + extra, extra + ["--relight", "--aov", "planes"])


# ---- the checker: the record, the ray and one bit per light are enough -------------------------------

def _equals_shade_ref(checker, s, cam, what):
    rays = rayq_ref.primary(checker, cam, W, H)
    rec = rayq_ref.trace(checker, s, rays)
    bits, hit = relight_ref.plane(checker, s, cam, W, H)
    assert not bits[rec["primitive"] == 0].any(), what   # a miss is 0
    if s.n_lights < 32:
        assert not (bits >> np.uint32(s.n_lights)).any(), what   # and so are the bits past the lights
    if s.n_lights:
        assert np.array_equal(hit, rec["primitive"] != 0), what
    for mode in range(4):
        for shadows in (0, 1):
            p = abi.make_params(W, H, mode, shadows)
            px, rgb = relight_ref.shade(checker, s, rays, rec, bits, p)
            wpx, wrgb, flags = shade_ref.shade(checker, s, rays, p)
            assert shade_ref.same(px, rgb, wpx, wrgb), (what, mode, shadows)
            if shadows and s.n_lights:   # a pixel the checker calls occluded has a bit set, and only such a pixel
                assert np.array_equal((flags & shade_ref.OCCLUDED) != 0, bits != 0), (what, mode)
    return bits, rec["primitive"] != 0


@pytest.mark.parametrize("name", PIN)
def test_the_record_the_ray_and_the_bits_give_shade_refs_pixels(checker, name):
    """Primary rays at 37x23, records from rayq_ref_trace, bits from rayq_ref_shadow + rayq_ref_occluded:
    relight_ref.c equals shade_ref_rays word for word, pixels and rgb, in all 8 mode/shadow configurations."""
    s, cam = HostScene(name).view()
    bits, hit = _equals_shade_ref(checker, s, cam, name)
    if name != "W1":
        assert hit.any() and bits.any()
        for l in range(s.n_lights):   # every light decides something: occluded somewhere, lit somewhere
            b = ((bits >> np.uint32(l)) & 1)[hit]
            assert b.any() and not b.all(), (name, l)


@pytest.mark.parametrize("family,seed", scene_fuzz.COMMITTED, ids=[f"{f}_{s}" for f, s in scene_fuzz.COMMITTED])
def test_the_same_on_the_committed_fuzz_views(checker, tmp_path, family, seed):
    keep, s, cam = aov_ref.golden_view(family, seed, tmp_path)
    assert s.n_lights <= 32
    _equals_shade_ref(checker, s, cam, (family, seed))
    del keep


# ---- the new kernels, from the code object's metadata only ---------------------------------------------

def _phase_kernels(notes: str, phase: int) -> dict:
    """(DEEP, SPEC, HSTK, CULLK) -> private segment bytes of the render kernel's instantiations of `phase`."""
    found = {}
    for block in notes.split("  - .")[1:]:
        m = re.search(rf"\.name:\s+_Z17rtx_render_kernelILb0ELi{phase}ELb([01])ELi(\d+)ELb([01])ELb([01])ELb0EE\w+", block)
        if m:
            found[tuple(int(x) for x in m.groups())] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
    return found


def test_the_new_kernels_metadata():
    import isa_tools
    lib = Path(abi.LIB_DIR) / "librtx_hip.so"
    assert lib.exists(), "librtx_hip.so is not built"
    _, notes = isa_tools.listing(str(lib))
    shade8, shadow9 = _phase_kernels(notes, 8), _phase_kernels(notes, 9)
    # the shadow pass walks as deferred shading does: the same (DEEP, SPEC, HSTK, CULLK) set, none with scratch
    assert len(shadow9) == 13 and set(shadow9) == set(shade8), (sorted(shadow9), sorted(shade8))
    for key, scratch in shadow9.items():
        assert scratch == 0, (key, scratch)
    relight = [b for b in notes.split("  - .")[1:] if re.search(r"\.name:\s+_Z18rtx_relight_kernel\w+", b)]
    assert len(relight) == 1
    assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", relight[0]).group(1)) == 0
    assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", relight[0]).group(1)) == 0
