"""Resolved relighting (include/rtx.h: rtx_relight_resolve*) without a GPU: the entry points are declared, exported
and bound and refuse a NULL context without a device; the C++ mirror's methods compile; the command-line program
refuses --resolve in a bad combination before any device work; the checkers agree on what the resolved frame is
(tests/ss_ref.py's box filter over tests/relight_ref.c's samples equals the same filter over tests/shade_ref.c's,
word for word); and the new kernel's code-object metadata: a name of its own beside the one rtx_relight_kernel, no
scratch, no LDS, and no more registers than the generic render kernel may use."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import abi_surface
import rayq_ref
import relight_ref
import shade_ref
import ss_ref
from checkers import checker  # noqa: F401
from gp1_raytracer_2223_amd import abi
from gp1_raytracer_2223_amd.scene import HostScene
from gpu_support import CONFIGS

ROOT = Path(__file__).resolve().parents[1]
EXE = ROOT / "gp1_raytracer_2223_amd" / "lib" / "rtx_render"
W, H = 37, 23


def test_header_declares_and_abi_binds_the_symbols(tmp_path):
    """Every entry point is declared as the issue states it, exported and bound, and the ABI version stays 2."""
    abi_surface.declared_exported_and_bound(tmp_path, {
        "rtx_relight_resolve_async": "int (*)(rtx_ctx*, const rtx_render_params*, uint32_t, int)",
        "rtx_relight_resolve": "int (*)(rtx_ctx*, const rtx_render_params*, uint32_t, uint32_t*, float*)",
    }, {"rtx_time_relight_resolve": "int (*)(rtx_ctx*, const rtx_render_params*, uint32_t, int, int, float*)"},
        ["RTX_ABI_VERSION == 2"])
    lib = abi.load_hip()
    assert lib.rtx_abi_version() == 2
    a = lib.rtx_relight_resolve.argtypes
    assert a[1]._type_ is abi.RenderParams and a[2] is C.c_uint32
    assert a[3]._type_ is C.c_uint32 and a[4]._type_ is C.c_float
    assert lib.rtx_relight_resolve_async.argtypes[2:] == [C.c_uint32, C.c_int]
    assert lib.rtx_time_relight_resolve.argtypes[2:5] == [C.c_uint32, C.c_int, C.c_int]


def test_null_context_is_invalid_without_a_device():
    lib = abi.load_hip()
    p = abi.make_params(8, 8)
    px = np.zeros(64, np.uint32)
    up = px.ctypes.data_as(C.POINTER(C.c_uint32))
    ms = C.c_float()
    for k in (2, 4, 8, 3):
        assert lib.rtx_relight_resolve_async(None, C.byref(p), k, 0) == abi.RTX_E_INVALID
        assert lib.rtx_relight_resolve(None, C.byref(p), k, up, None) == abi.RTX_E_INVALID
        assert lib.rtx_time_relight_resolve(None, C.byref(p), k, 0, 1, C.byref(ms)) == abi.RTX_E_INVALID
    assert lib.rtx_relight_resolve(None, C.byref(p), 2, None, None) == abi.RTX_E_INVALID
    assert lib.rtx_time_relight_resolve(None, C.byref(p), 2, 0, 1, None) == abi.RTX_E_INVALID
    assert lib.rtx_time_relight_resolve(None, C.byref(p), 2, 0, 0, C.byref(ms)) == abi.RTX_E_INVALID


def test_the_cpp_mirror_compiles(tmp_path):
    abi_surface.cpp_mirror_compiles(tmp_path, [("void (rtx::Renderer::*)(uint32_t)", "RenderSamplePasses"),
                                               ("void (rtx::Renderer::*)()", "RelightResolved")])


@pytest.mark.parametrize("args", [["--resolve", "2"], ["--resolve", "4", "--deferred"],
                                  ["--relight", "--resolve", "2", "--aov", "planes"],
                                  ["--relight", "--resolve", "3"], ["--relight", "--resolve", "1"],
                                  ["--relight", "--resolve", "16"], ["--relight", "--resolve", "2x"], ["--relight", "--resolve"]],
                         ids=["no_relight", "deferred_instead", "aov", "k3", "k1", "k16", "k2x", "no_k"])
def test_cli_refuses_resolve_in_a_bad_combination_before_device_work(tmp_path, args):
    abi_surface.cli_refuses(tmp_path, "--resolve", args, returncode=2)


def test_cli_still_refuses_relight_with_ss_and_names_resolve_in_its_usage(tmp_path):
    r = subprocess.run([str(EXE), "W4_Bunny", "64", "48", "--out", "o.bmp", "--relight", "--ss", "2"],
                       capture_output=True, text=True, cwd=tmp_path, timeout=60)
    assert r.returncode == 2 and "--relight" in r.stderr and list(tmp_path.iterdir()) == []
    r = subprocess.run([str(EXE)], capture_output=True, text=True, cwd=tmp_path, timeout=60)
    assert r.returncode == 2 and "--resolve K" in r.stderr


# ---- the checkers agree on the resolved frame ---------------------------------------------------------------

@pytest.mark.parametrize("k", [2, 4, 8])
@pytest.mark.parametrize("name", ["W4_Bunny", "W3"])
def test_resolved_relight_ref_equals_resolved_shade_ref(checker, name, k):
    """The kW x kH primary rays, their records and relight_ref.plane's bits: ss_ref.resolve + quantize over
    relight_ref.shade equals the same resolve over shade_ref.shade of those rays, word for word, in all 8
    mode / shadow configurations; and the resolve is exercised (pixels whose samples differ)."""
    s, cam = HostScene(name).view()
    rays = rayq_ref.primary(checker, cam, k * W, k * H)
    rec = rayq_ref.trace(checker, s, rays)
    bits, _ = relight_ref.plane(checker, s, cam, k * W, k * H)
    prim = rec["primitive"].reshape(H, k, W, k)
    assert (prim != prim[:, :1, :, :1]).any(axis=(1, 3)).any(), "no pixel has samples of two primitives"
    for mode, sh in CONFIGS:
        p = abi.make_params(k * W, k * H, mode, sh)
        _, rgb = relight_ref.shade(checker, s, rays, rec, bits, p)
        _, wrgb, _ = shade_ref.shade(checker, s, rays, p)
        got, want = ss_ref.resolve(rgb, W, H, k), ss_ref.resolve(wrgb, W, H, k)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, k, mode, sh)
        assert np.array_equal(ss_ref.quantize(got), ss_ref.quantize(want)), (name, k, mode, sh)


# ---- the new kernel, from the code object's metadata only ---------------------------------------------------

def test_the_resolve_kernels_metadata():
    import isa_tools
    lib = Path(abi.LIB_DIR) / "librtx_hip.so"
    assert lib.exists(), "librtx_hip.so is not built"
    _, notes = isa_tools.listing(str(lib))
    blocks = notes.split("  - .")[1:]
    resolve = [b for b in blocks if re.search(r"\.name:\s+_Z26rtx_relight_resolve_kernel\w+", b)]
    assert len(resolve) == 3, "one instantiation per factor: 2 x 2, 4 x 4, 8 x 8"

    def field(block, key):
        m = re.search(rf"\.{key}:\s+(\d+)", block)
        return int(m.group(1)) if m else 0

    for b in resolve:
        name = re.search(r"\.name:\s+(\S+)", b).group(1)
        assert field(b, "private_segment_fixed_size") == 0, name
        assert field(b, "group_segment_fixed_size") == 0, name
        # the bound tests/test_isa.py holds the generic render kernel to; this kernel does strictly less
        assert field(b, "vgpr_count") + field(b, "agpr_count") <= 80, (name, field(b, "vgpr_count"), field(b, "agpr_count"))
    relight = [b for b in blocks if re.search(r"\.name:\s+_Z18rtx_relight_kernel\w+", b)]
    assert len(relight) == 1
