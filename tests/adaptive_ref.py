"""Adaptive supersampling (include/rtx.h: rtx_render_adaptive) restated in numpy — TEST INFRASTRUCTURE
(the checker of tests/test_adaptive_cpu.py and tests/test_gpu_adaptive.py), built on tests/ss_ref.py.

`edges` is the contract's mask E over the plain frame's uint32 plane: integer only, read through the
caller's pixel format; `compose` is the adaptive frame A = S where E holds, else P, in either plane."""
from __future__ import annotations

import numpy as np

import ss_ref

FACTORS = (2, 4, 8)
XRGB8888 = (16, 8, 0, 0)


def channels(px, fmt=XRGB8888) -> np.ndarray:
    """(n, 3) int32: channel c of a pixel word is (word >> shift_c) & 255."""
    w = np.asarray(px, dtype=np.uint32).reshape(-1)
    return np.stack([((w >> np.uint32(s)) & np.uint32(255)).astype(np.int32) for s in fmt[:3]], axis=1)


def edges(px, W: int, H: int, tau: int, fmt=XRGB8888) -> np.ndarray:
    """E as a flat bool array of W * H: some 4-neighbour inside the frame differs from the pixel by more
    than tau in some channel.  Both pixels of such a pair are in E."""
    c = channels(px, fmt).reshape(H, W, 3)
    e = np.zeros((H, W), bool)
    dx = (np.abs(c[:, 1:] - c[:, :-1]) > int(tau)).any(axis=2)   # (x, y) against (x + 1, y)
    dy = (np.abs(c[1:, :] - c[:-1, :]) > int(tau)).any(axis=2)   # (x, y) against (x, y + 1)
    e[:, 1:] |= dx
    e[:, :-1] |= dx
    e[1:, :] |= dy
    e[:-1, :] |= dy
    return e.reshape(-1)


def compose(P, S, E) -> np.ndarray:
    """A = S where E, else P.  P and S are planes of W * H elements (the uint32 plane) or 3 W * H
    (the float plane, selected bit for bit); E is edges()'s mask."""
    P, S = np.asarray(P), np.asarray(S)
    E = np.asarray(E, bool).reshape(-1)
    assert P.shape == S.shape and P.dtype == S.dtype and P.size % E.size == 0
    per = P.size // E.size
    bits = np.uint32
    out = np.where(np.repeat(E, per), S.reshape(-1).view(bits), P.reshape(-1).view(bits))
    return out.view(P.dtype)


def supersampled(rgb_hi, W: int, H: int, k: int, fmt=XRGB8888):
    """S from the kW x kH frame's colours: (uint32 plane, float plane), by ss_ref."""
    rgb = ss_ref.resolve(rgb_hi, W, H, k)
    return ss_ref.quantize(rgb, fmt), rgb
