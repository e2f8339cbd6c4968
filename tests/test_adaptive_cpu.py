"""Adaptive supersampling (include/rtx.h: rtx_render_adaptive) without a GPU: the entry points are declared,
exported and bound; the numpy checker (tests/adaptive_ref.py) has the contract's properties and gives the
pinned mask sizes on the oracle's frames; the C++ mirror compiles; the command-line program refuses a bad
--adaptive before any device work."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import abi_surface
import adaptive_ref
import oracle_bind
import ss_ref
from gp1_raytracer_2223_amd import abi
from gp1_raytracer_2223_amd.scene import HostScene

ROOT = Path(__file__).resolve().parents[1]
INC = ROOT / "include"
EXE = ROOT / "gp1_raytracer_2223_amd" / "lib" / "rtx_render"

_frames = {}


def _oracle(name, W, H):
    """The oracle's plain frame (computed once per case, never written to)."""
    if (name, W, H) not in _frames:
        s, cam = HostScene(name).view()
        px, rgb = oracle_bind.render(s, cam, abi.make_params(W, H))
        px.setflags(write=False)
        rgb.setflags(write=False)
        _frames[(name, W, H)] = (px, rgb)
    return _frames[(name, W, H)]


def test_header_declares_and_abi_binds_the_adaptive_symbols(tmp_path):
    """The three entry points and the timing twin are declared as the contract states them, exported and
    bound, and the ABI version stays 2."""
    abi_surface.declared_exported_and_bound(tmp_path, {
        "rtx_render_adaptive_async":
            "int (*)(rtx_ctx*, const rtx_camera*, const rtx_render_params*, int, uint32_t, uint32_t)",
        "rtx_render_adaptive":
            "int (*)(rtx_ctx*, const rtx_camera*, const rtx_render_params*, uint32_t, uint32_t, uint32_t*, float*)",
        "rtx_adaptive_refined": "int (*)(rtx_ctx*, uint32_t*)",
    }, {
        "rtx_time_adaptive_frames":
            "int (*)(rtx_ctx*, const rtx_camera*, const rtx_render_params*, uint32_t, uint32_t, int, float*)",
    }, ["RTX_ABI_VERSION == 2"])
    lib = abi.load_hip()
    assert lib.rtx_abi_version() == 2
    assert re.search(r"^#define RTX_ABI_VERSION 2$", (INC / "rtx.h").read_text(), re.M)
    a = lib.rtx_render_adaptive_async.argtypes
    assert a[1]._type_ is abi.Camera and a[2]._type_ is abi.RenderParams and a[3:] == [C.c_int, C.c_uint32, C.c_uint32]
    a = lib.rtx_render_adaptive.argtypes
    assert a[3:5] == [C.c_uint32, C.c_uint32] and a[5]._type_ is C.c_uint32 and a[6]._type_ is C.c_float
    assert lib.rtx_adaptive_refined.argtypes[1]._type_ is C.c_uint32


def test_null_arguments_are_refused_without_a_device():
    lib = abi.load_hip()
    n = C.c_uint32()
    p = abi.make_params(8, 8)
    assert lib.rtx_render_adaptive_async(None, None, C.byref(p), 0, 2, 32) == abi.RTX_E_INVALID
    assert lib.rtx_render_adaptive(None, None, C.byref(p), 2, 32, None, None) == abi.RTX_E_INVALID
    assert lib.rtx_adaptive_refined(None, C.byref(n)) == abi.RTX_E_INVALID
    assert lib.rtx_time_adaptive_frames(None, None, C.byref(p), 2, 32, 1, None) == abi.RTX_E_INVALID


def test_the_cpp_mirror_compiles(tmp_path):
    abi_surface.cpp_mirror_compiles(tmp_path, [
        ("void (rtx::Renderer::*)(const rtx_camera&, uint32_t, uint32_t)", "RenderAdaptive"),
        ("void (rtx::Renderer::*)(rtx_host_scene*, uint32_t, uint32_t, bool)", "RenderAdaptive"),
        ("uint32_t (rtx::Renderer::*)()", "AdaptiveRefined")])


# the mask sizes measured on the oracle's frames, XRGB8888
PINNED = [("W4_Bunny", 37, 23, 0, 851), ("W4_Bunny", 37, 23, 32, 87), ("W4_Bunny", 37, 23, 255, 0),
          ("W3", 37, 23, 32, 147), ("W2", 37, 23, 32, 452), ("W4_Bunny", 160, 120, 8, 1976)]


@pytest.mark.parametrize("name,W,H,tau,want", PINNED)
def test_mask_sizes_on_the_oracles_frames(name, W, H, tau, want):
    px, _ = _oracle(name, W, H)
    E = adaptive_ref.edges(px, W, H, tau)
    assert E.dtype == bool and E.shape == (W * H,)
    assert int(E.sum()) == want


def _edges_by_definition(px, W, H, tau, fmt):
    """E pixel by pixel, as rtx.h words it (the slow form of adaptive_ref.edges)."""
    w = np.asarray(px, np.uint32).reshape(H, W)
    ch = lambda v: [(int(v) >> s) & 255 for s in fmt[:3]]   # noqa: E731
    E = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            for nx, ny in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)):
                if 0 <= nx < W and 0 <= ny < H:
                    if any(abs(a - b) > tau for a, b in zip(ch(w[y, x]), ch(w[ny, nx]))):
                        E[y, x] = True
    return E.reshape(-1)


@pytest.mark.parametrize("fmt", [adaptive_ref.XRGB8888, (0, 8, 16, 0xFF000000)])
@pytest.mark.parametrize("tau", [0, 8, 32, 254])
def test_edges_is_the_definition_and_symmetric(fmt, tau):
    W, H = 37, 23
    _, rgb = _oracle("W3", W, H)
    px = ss_ref.quantize(rgb, fmt)
    E = adaptive_ref.edges(px, W, H, tau, fmt)
    assert np.array_equal(E, _edges_by_definition(px, W, H, tau, fmt))
    # symmetric: a pixel of E has a 4-neighbour in E that differs from it by more than tau
    c = adaptive_ref.channels(px, fmt).reshape(H, W, 3)
    e = E.reshape(H, W)
    for y, x in zip(*np.nonzero(e)):
        nb = [(y, x - 1), (y, x + 1), (y - 1, x), (y + 1, x)]
        assert any(0 <= b < H and 0 <= a < W and e[b, a] and (np.abs(c[y, x] - c[b, a]) > tau).any() for b, a in nb)


def test_edges_reads_the_channels_through_the_format():
    """Two words that differ only in bits 24-31: a channel under XRGB8888's alpha, none at shifts 0/8/16."""
    px = np.array([0x00102030, 0xFF102030], np.uint32)
    assert not adaptive_ref.edges(px, 2, 1, 0, (16, 8, 0, 0)).any()
    assert adaptive_ref.edges(px, 2, 1, 0, (24, 8, 0, 0)).all()
    assert adaptive_ref.edges(px, 1, 2, 254, (24, 8, 0, 0)).all() and not adaptive_ref.edges(px, 1, 2, 255, (24, 8, 0, 0)).any()


def test_a_single_pixel_frame_has_no_neighbours():
    assert not adaptive_ref.edges(np.array([0xFFFFFF], np.uint32), 1, 1, 0).any()


def test_compose_with_an_empty_and_a_full_mask():
    W, H, k = 37, 23, 2
    P_px, P_rgb = _oracle("W4_Bunny", W, H)
    _, hi = _oracle("W4_Bunny", k * W, k * H)
    S_px, S_rgb = adaptive_ref.supersampled(hi, W, H, k)
    assert not np.array_equal(P_px, S_px)
    none, every = np.zeros(W * H, bool), np.ones(W * H, bool)
    for P, S in ((P_px, S_px), (P_rgb, S_rgb)):
        a, b = adaptive_ref.compose(P, S, none), adaptive_ref.compose(P, S, every)
        assert a.dtype == P.dtype and np.array_equal(a.view(np.uint32), P.view(np.uint32))
        assert b.dtype == P.dtype and np.array_equal(b.view(np.uint32), S.view(np.uint32))
    # tau = 255 is the empty mask, tau = 0 on this frame the full one
    assert not adaptive_ref.edges(P_px, W, H, 255).any() and adaptive_ref.edges(P_px, W, H, 0).all()
    E = adaptive_ref.edges(P_px, W, H, 32)
    A = adaptive_ref.compose(P_rgb, S_rgb, E).reshape(-1, 3)
    assert np.array_equal(A[E].view(np.uint32), S_rgb.reshape(-1, 3)[E].view(np.uint32))
    assert np.array_equal(A[~E].view(np.uint32), P_rgb.reshape(-1, 3)[~E].view(np.uint32))


@pytest.mark.parametrize("arg", ["3,32", "2", "2,256", "2,-1", "4,8x", "x"])
def test_cli_refuses_a_bad_pair_before_device_work(tmp_path, arg):
    assert EXE.exists(), "lib/rtx_render is not built"
    r = subprocess.run([str(EXE), "W4_Bunny", "64", "48", "--adaptive", arg, "--out", str(tmp_path / "o.bmp")],
                       capture_output=True, text=True, cwd=tmp_path, timeout=60)
    assert r.returncode != 0
    assert "--adaptive" in r.stderr and "2, 4 or 8" in r.stderr
    assert "rtx_create" not in r.stderr and "scene" not in r.stderr
    assert not (tmp_path / "o.bmp").exists()


@pytest.mark.parametrize("extra", [["--ss", "2"], ["--aov", "p"], ["--benchmark"], ["--sequence", "0.5"], ["--rays", "r.bin"]])
def test_cli_refuses_adaptive_with_the_other_frame_modes(tmp_path, extra):
    r = subprocess.run([str(EXE), "W4_Bunny", "64", "48", "--adaptive", "2,32", *extra, "--out", str(tmp_path / "o.bmp")],
                       capture_output=True, text=True, cwd=tmp_path, timeout=60)
    assert r.returncode != 0 and "--adaptive renders a single frame" in r.stderr
    assert "rtx_create" not in r.stderr and not (tmp_path / "o.bmp").exists()
