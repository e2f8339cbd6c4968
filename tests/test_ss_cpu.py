"""Supersampling without a GPU: the new entry points are declared, exported and bound; the numpy
restatement of the resolve (tests/ss_ref.py) has the contract's properties, the order of its
additions included; the command-line program refuses a bad factor before any device work."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ss_ref
from gp1_raytracer_2223_amd import abi

ROOT = Path(__file__).resolve().parents[1]
EXE = ROOT / "gp1_raytracer_2223_amd" / "lib" / "rtx_render"
NAMES = ("rtx_set_supersample", "rtx_group_set_supersample")


@pytest.mark.parametrize("name", NAMES)
def test_entry_point_declared_exported_and_bound(name):
    txt = (ROOT / "include" / "rtx.h").read_text()
    assert re.search(r"^int\s+%s\s*\(" % name, txt, re.M), f"{name} is not declared in rtx.h"
    lib = abi.load_hip()   # loads without a GPU; no compute call is made here
    assert hasattr(lib, name)
    assert name in abi.HIP_SYMBOLS
    assert getattr(lib, name).argtypes is not None


def test_set_supersample_rejects_a_null_context():
    lib = abi.load_hip()
    assert lib.rtx_set_supersample(None, 2) == abi.RTX_E_INVALID
    assert lib.rtx_group_set_supersample(None, 2) == abi.RTX_E_INVALID


def test_resolve_k1_is_identity():
    rng = np.random.default_rng(7)
    a = rng.random(5 * 3 * 3, dtype=np.float32)
    out = ss_ref.resolve(a, 5, 3, 1)
    assert out.dtype == np.float32 and np.array_equal(out.view(np.uint32), a.view(np.uint32))


@pytest.mark.parametrize("k", [2, 4, 8])
def test_resolve_constant_frame_is_exact(k):
    W, H = 3, 2
    c = np.array([0.1, 0.7, 1.0], np.float32)   # sums of 2^n equal floats and the 2^-n scale are exact
    hi = np.tile(c, k * W * k * H)
    out = ss_ref.resolve(hi, W, H, k).reshape(-1, 3)
    assert np.array_equal(out.view(np.uint32), np.tile(c, W * H).reshape(-1, 3).view(np.uint32))


def _one_pixel(s00, s01, s10, s11):
    """A 1 x 1 frame with k = 2 whose samples are (sx, sy) = s00 s01 / s10 s11, grey."""
    v = np.array([s00, s01, s10, s11], np.float32)
    return np.repeat(v, 3)


def test_resolve_order_is_the_pair_tree_x_then_y():
    f = np.float32
    e = f(2.0 ** -24)
    # pair tree (1 + e) + (e + e) = 1 + 2e, sequential ((1 + e) + e) + e = 1: 1 + e ties to even, 1
    a = [f(1), e, e, e]
    tree = (a[0] + a[1]) + (a[2] + a[3])
    seq = ((a[0] + a[1]) + a[2]) + a[3]
    assert tree == f(1) + f(2.0 ** -23) and seq == f(1) and tree != seq
    out = ss_ref.resolve(_one_pixel(*a), 1, 1, 2)
    assert np.array_equal(out, np.full(3, tree * f(0.25), np.float32))
    # sx first: (1 + e) + (2e + 0) = 1 + 2e; sy first: (1 + 2e) + (e + 0) = 1 + 3e -> ties to even, 1 + 4e
    b = [f(1), e, f(2) * e, f(0)]
    x_first = (b[0] + b[1]) + (b[2] + b[3])
    y_first = (b[0] + b[2]) + (b[1] + b[3])
    assert x_first == f(1) + f(2.0 ** -23) and y_first == f(1) + f(2.0 ** -22)
    out = ss_ref.resolve(_one_pixel(*b), 1, 1, 2)
    assert np.array_equal(out, np.full(3, x_first * f(0.25), np.float32))


def test_resolve_k4_is_the_tree_of_k2():
    """The 4 x 4 tree is the 2 x 2 tree of 2 x 2 trees taken over sx first: resolving twice by 2
    differs from it only by the order (x, y, x, y against x, x, y, y), so on a frame whose rows are
    equal the two agree exactly, and in general the scale is the same power of two."""
    rng = np.random.default_rng(11)
    row = rng.random((1, 8, 3), dtype=np.float32)
    hi = np.repeat(row, 4, axis=0)                       # 2 x 1 pixels of 4 x 4 samples, equal rows
    once = ss_ref.resolve(hi.reshape(-1), 2, 1, 4)
    twice = ss_ref.resolve(ss_ref.resolve(hi.reshape(-1), 4, 2, 2), 2, 1, 2)
    assert np.array_equal(once.view(np.uint32), twice.view(np.uint32))


def test_quantize_is_q8_xrgb():
    rgb = np.array([0.0, 0.5, 1.0, 0.999, 0.004, 0.25], np.float32)
    assert ss_ref.quantize(rgb).tolist() == [(0 << 16) | (127 << 8) | 255, (254 << 16) | (1 << 8) | 63]
    assert ss_ref.quantize(rgb[:3], (0, 8, 16, 0xFF000000)).tolist() == [0xFF000000 | (255 << 16) | (127 << 8)]


@pytest.mark.parametrize("arg", ["3", "0", "16", "x"])
def test_cli_refuses_a_bad_factor_before_device_work(tmp_path, arg):
    assert EXE.exists(), "lib/rtx_render is not built"
    r = subprocess.run([str(EXE), "W4_Bunny", "64", "48", "--ss", arg, "--out", str(tmp_path / "o.bmp")],
                       capture_output=True, text=True, cwd=tmp_path, timeout=60)
    assert r.returncode != 0
    assert "--ss" in r.stderr and "1, 2, 4 or 8" in r.stderr
    # nothing after the argument check ran: no context was created (its failure has its own message
    # on a machine without a GPU), no scene built, no file written
    assert "rtx_create" not in r.stderr and "scene" not in r.stderr
    assert not (tmp_path / "o.bmp").exists()
