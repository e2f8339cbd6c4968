"""An arbitrary shadow plane written behind the library's back — TEST INFRASTRUCTURE, tests/shadowbuf.py's
counterpart for the incremental shadow pass (rtx_update_shadows_async, rtx_refresh_shadows_async).

An update READS the plane, so the plane cannot be poisoned whole before it as before a full pass.  Instead the test
forges it: a seeded pseudo-random word in every pixel of a row the pass owns, a sentinel in every other word.
After the update every owned word must be exactly

    (F & keep) | (want & trace)

with `want` the checker's plane of the scene uploaded now, and every other word still the sentinel.  One
comparison then proves that the traced bits were rewritten in every owned pixel, that the kept bits were carried
over verbatim, that every bit outside keep | trace (those at or above the light count among them) was cleared,
and that no other word was touched.

Rules for callers: those of tests/shadowbuf.py (write and peek exactly n_views * width * height words, only after
a shadow pass of that shape has run on the context).  The forged words are random, so the sentinel of unowned rows
cannot be told from them by value: it is recognised by position alone (the rows `devbuf.owned_rows` denies)."""
from __future__ import annotations

import numpy as np

import devbuf
import shadowbuf


def _views(a, n_views: int, n: int) -> np.ndarray:
    if isinstance(a, (list, tuple)):
        a = np.concatenate([np.asarray(x, np.uint32).reshape(-1) for x in a])
    a = np.asarray(a, np.uint32).reshape(-1)
    assert a.size == n_views * n
    return a


def forged(params, n_views: int, seed: int, sentinel: int = shadowbuf.SENTINEL, force: int = 0) -> np.ndarray:
    """The plane F of a pass of `params` and `n_views`: random words (OR `force`) in owned rows, the sentinel in
    the others."""
    W, H = int(params.width), int(params.height)
    rng = np.random.default_rng(seed)
    F = rng.integers(0, 1 << 32, size=(n_views, H, W), dtype=np.uint64).astype(np.uint32) | np.uint32(force)
    for v in range(n_views):
        F[v][~devbuf.owned_rows(params, v)] = np.uint32(sentinel)
    return F.reshape(-1)


def write(ctx, words: np.ndarray) -> None:
    """The device shadow plane = `words` (a raw host-to-device copy), complete on return."""
    words = np.ascontiguousarray(words, np.uint32)
    ctx.synchronize()
    d = ctx.device_shadow_buffer()
    assert d and words.size > 0
    h = devbuf.hip()
    devbuf._ok(h.hipSetDevice(ctx.device), "hipSetDevice")
    devbuf._ok(h.hipMemcpy(d, words.ctypes.data, 4 * words.size, 1), "hipMemcpy H2D")
    devbuf._ok(h.hipDeviceSynchronize(), "hipDeviceSynchronize")


def expected(params, n_views: int, F, want, trace: int, keep: int) -> np.ndarray:
    """(F & keep) | (want & trace) in owned rows, F (the sentinel) elsewhere."""
    W, H = int(params.width), int(params.height)
    n = W * H
    F = _views(F, n_views, n).reshape(n_views, H, W)
    want = _views(want, n_views, n).reshape(n_views, H, W)
    out = F.copy()
    for v in range(n_views):
        own = devbuf.owned_rows(params, v)
        out[v][own] = (F[v][own] & np.uint32(keep)) | (want[v][own] & np.uint32(trace))
    return out.reshape(-1)


def check(ctx, params, n_views: int, F, want, trace: int, keep: int, what: str = "") -> np.ndarray:
    """The standard check after an update that ran on the forged plane F.  Returns the plane read raw."""
    W, H = int(params.width), int(params.height)
    n = W * H
    exp = expected(params, n_views, F, want, trace, keep).reshape(n_views, H, W)
    got = shadowbuf.peek(ctx, n_views * n).reshape(n_views, H, W)
    Fv = _views(F, n_views, n).reshape(n_views, H, W)
    for v in range(n_views):
        own = devbuf.owned_rows(params, v)
        other = got[v][~own] != Fv[v][~own]
        assert not other.any(), f"{what} view {v}: {int(other.sum())} words of rows the pass does not own were written"
        bad = got[v][own] ^ exp[v][own]
        if bad.any():
            t, k = np.uint32(trace), np.uint32(keep)
            raise AssertionError(
                f"{what} view {v}: {int((bad != 0).sum())} owned words differ: {int(((bad & t) != 0).sum())} in a traced "
                f"bit, {int(((bad & k) != 0).sum())} in a kept bit, {int(((bad & ~(t | k)) != 0).sum())} in a bit that "
                f"must be clear")
    return got.reshape(-1)
