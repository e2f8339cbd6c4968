"""The device frame buffer read and written behind the library's back — TEST INFRASTRUCTURE.

A context keeps one frame buffer (rtx_ctx::d_px, d_rgb) for every frame it renders and never clears
it, so a frame that repeats an earlier one lands on memory that already holds the right answer: a tile
the kernels never wrote would still read back correct.  `poison` fills the buffer with words no frame
can contain before the frame under test, and `check` reads it back raw (not through rtx_download,
which copies owned rows only) and demands that every word of a row the frame owns was written with the
expected value and that every other word still holds the sentinel.

Rules for callers:
  * the pointers are fetched afresh on every call (a larger frame reallocates the buffer);
  * poison and peek exactly n_views * width * height words;
  * only after at least one frame of that shape and view count (with want_rgb when the colour plane is
    poisoned) has been rendered on the context: the range is then inside the allocation;
  * the expected frame must not contain a sentinel (`assert_legal`): XRGB8888 pixels have a zero top
    byte, and pow-free finite scenes have no NaN colour.

The HIP runtime is the one librtx_hip.so already loaded, called through ctypes."""
from __future__ import annotations

import ctypes as C

import numpy as np

from gp1_raytracer_2223_amd import abi

PX_SENTINEL = 0xDEADBEEF    # top byte 0xDE: no pixel of a format with amask 0 and 8-bit channels below bit 24
RGB_SENTINEL = 0x7FC0DEAD   # a quiet NaN: no colour word of a finite frame

_hip = None


def hip() -> C.CDLL:
    global _hip
    if _hip is None:
        abi.load_hip()   # (librtx_hip.so brings the runtime in)
        try:
            lib = C.CDLL("libamdhip64.so")
        except OSError:
            lib = C.CDLL("/opt/rocm/lib/libamdhip64.so")
        lib.hipSetDevice.argtypes = [C.c_int]
        lib.hipMemsetD32.argtypes = [C.c_void_p, C.c_uint32, C.c_size_t]
        lib.hipDeviceSynchronize.argtypes = []
        lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        for f in (lib.hipSetDevice, lib.hipMemsetD32, lib.hipDeviceSynchronize, lib.hipMemcpy):
            f.restype = C.c_int
        _hip = lib
    return _hip


def _ok(rc: int, what: str) -> None:
    assert rc == 0, f"{what} failed with hipError {rc}"


def fill(ctx, d_ptr: int, n_words: int, word: int) -> None:
    """d_ptr[0:n_words] = word (32-bit), complete on return.  The caller has drained the context."""
    assert d_ptr and n_words > 0
    h = hip()
    _ok(h.hipSetDevice(ctx.device), "hipSetDevice")
    _ok(h.hipMemsetD32(d_ptr, word, n_words), "hipMemsetD32")
    _ok(h.hipDeviceSynchronize(), "hipDeviceSynchronize")


def read(ctx, d_ptr: int, n_words: int) -> np.ndarray:
    """A raw D2H copy of d_ptr[0:n_words] as uint32.  The caller has drained the context."""
    assert d_ptr and n_words > 0
    out = np.empty(n_words, np.uint32)
    h = hip()
    _ok(h.hipSetDevice(ctx.device), "hipSetDevice")
    _ok(h.hipMemcpy(out.ctypes.data, d_ptr, 4 * n_words, 2), "hipMemcpy D2H")
    return out


def pointers(ctx) -> tuple[int, int]:
    """(d_px, d_rgb) of the context's colour frame buffer, fetched afresh."""
    return ctx.device_buffers()


def poison(ctx, n_words: int, rgb: bool = False) -> None:
    """Join and drain the context, then fill d_px[0:n_words] (and d_rgb[0:3 n_words]) with the sentinels."""
    ctx.synchronize()
    d_px, d_rgb = pointers(ctx)
    fill(ctx, d_px, n_words, PX_SENTINEL)
    if rgb:
        fill(ctx, d_rgb, 3 * n_words, RGB_SENTINEL)


def peek(ctx, n_words: int, rgb: bool = False):
    """(pixels, colour words or None) as uint32, every row, after the context's queued work."""
    ctx.synchronize()
    d_px, d_rgb = pointers(ctx)
    return read(ctx, d_px, n_words), (read(ctx, d_rgb, 3 * n_words) if rgb else None)


def owned_rows(params, view: int) -> np.ndarray:
    """bool[height]: the rows view `view` of a frame of `params` owns (include/rtx.h: stripe s of
    stripe_rows rows belongs to view v iff s % stripe_step == (stripe_first - v) mod stripe_step)."""
    H = int(params.height)
    rows, first, step = int(params.stripe_rows), int(params.stripe_first), int(params.stripe_step)
    if rows == 0 or step <= 1:
        return np.ones(H, bool)
    s = np.arange(H) // rows
    return s % step == (first - view) % step


def assert_legal(want_px=None, want_rgb=None) -> None:
    """The sentinels cannot be output: every expected pixel has a zero top byte, no colour is a NaN."""
    if want_px is not None:
        assert not (np.asarray(want_px, np.uint32) >> np.uint32(24)).any(), "an expected pixel has a non-zero top byte"
    if want_rgb is not None:
        assert not np.isnan(np.asarray(want_rgb, np.float32)).any(), "an expected colour is a NaN"


def _views(a, n_views: int, per_view: int, dtype) -> list:
    if isinstance(a, (list, tuple)):
        out = [np.ascontiguousarray(x, dtype).reshape(-1) for x in a]
    else:
        flat = np.ascontiguousarray(a, dtype).reshape(-1)
        out = [flat[v * per_view:(v + 1) * per_view] for v in range(n_views)]
    assert len(out) == n_views and all(x.size == per_view for x in out)
    return out


def check(ctx, params, n_views: int, want_px, want_rgb=None, what: str = "") -> None:
    """Peek, then: every word of an owned row equals the expected frame's (one array per view, or the
    views concatenated), none is the sentinel, and every word of a row the frame does not own is still
    the sentinel.  With want_rgb the same for the colour plane, word for word."""
    W, H = int(params.width), int(params.height)
    n = W * H
    wpx = _views(want_px, n_views, n, np.uint32)
    wrgb = _views(want_rgb, n_views, 3 * n, np.float32) if want_rgb is not None else None
    got_px, got_rgb = peek(ctx, n_views * n, rgb=wrgb is not None)
    for v in range(n_views):
        own = owned_rows(params, v)
        planes = [("pixels", got_px[v * n:(v + 1) * n].reshape(H, W), wpx[v].reshape(H, W), PX_SENTINEL)]
        assert_legal(want_px=wpx[v].reshape(H, W)[own])
        if wrgb is not None:
            assert_legal(want_rgb=wrgb[v].reshape(H, 3 * W)[own])
            planes.append(("colours", got_rgb[3 * v * n:3 * (v + 1) * n].reshape(H, 3 * W),
                           wrgb[v].view(np.uint32).reshape(H, 3 * W), RGB_SENTINEL))
        for name, got, want, sentinel in planes:
            g, w = got[own], want[own]
            stale = int((g == np.uint32(sentinel)).sum())
            assert stale == 0, f"{what} view {v}: {stale} owned {name} words were never written " \
                               f"(first at row {int(np.flatnonzero(own)[np.argwhere(g == np.uint32(sentinel))[0][0]])})"
            bad = g != w
            assert not bad.any(), f"{what} view {v}: {int(bad.sum())} owned {name} words differ from the expected frame"
            other = got[~own]
            assert (other == np.uint32(sentinel)).all(), \
                f"{what} view {v}: {int((other != np.uint32(sentinel)).sum())} {name} words of rows the frame does " \
                f"not own were written"
