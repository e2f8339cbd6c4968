"""The supersampling resolve of include/rtx.h (rtx_set_supersample) restated in float32 numpy —
TEST INFRASTRUCTURE (the checker of tests/test_ss_cpu.py and tests/test_gpu_ss.py).

The samples of a W x H frame with factor k are the pixels of the reference's kW x kH frame
(post-MaxToOne floats); `resolve` is the box filter in the contract's order of additions and
`quantize` the uint32 plane of the resolved colour."""
from __future__ import annotations

import numpy as np

FACTORS = (1, 2, 4, 8)


def _pair_tree(a: np.ndarray, axis: int) -> np.ndarray:
    """Adjacent-pair sums along `axis` until one entry is left: (s0+s1), (s2+s3), ..., then pairs of
    those.  float32 throughout (numpy adds two float32 arrays in float32, one rounding each)."""
    a = np.moveaxis(a, axis, -2)          # (..., n, 3)
    while a.shape[-2] > 1:
        a = a[..., 0::2, :] + a[..., 1::2, :]
    return a[..., 0, :]


def resolve(rgb_hi, W: int, H: int, k: int) -> np.ndarray:
    """rgb_hi: the kW x kH frame's colours (3 float32 per sample, row-major).  Returns the W x H
    frame's colours, flat like the renderer's float plane."""
    assert k in FACTORS
    a = np.ascontiguousarray(rgb_hi, dtype=np.float32).reshape(H, k, W, k, 3)
    assert a.dtype == np.float32
    rows = _pair_tree(a, 3)               # over sx -> (H, k, W, 3)
    px = _pair_tree(rows, 1)              # over sy -> (H, W, 3)
    out = px * np.float32(1.0 / (k * k))  # an exact power of two
    assert out.dtype == np.float32
    return out.reshape(-1)


def quantize(rgb, fmt=(16, 8, 0, 0)) -> np.ndarray:
    """q8 of each channel (static_cast<uint8_t>(c * 255): the float32 product truncated, low byte)
    packed with the caller's shifts and alpha mask; XRGB8888 by default."""
    c = np.asarray(rgb, dtype=np.float32).reshape(-1, 3)
    v = c * np.float32(255)
    with np.errstate(invalid="ignore"):
        in_range = np.abs(v) < np.float32(2.0 ** 31)   # cvttss2si: NaN and out of range give 0x80000000, low byte 0
    q = (np.where(in_range, v, np.float32(0)).astype(np.int32) & 255).astype(np.uint32)
    rs, gs, bs, amask = fmt
    return (q[:, 0] << np.uint32(rs)) | (q[:, 1] << np.uint32(gs)) | (q[:, 2] << np.uint32(bs)) | np.uint32(amask)
