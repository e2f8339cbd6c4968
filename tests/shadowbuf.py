"""The device shadow plane (rtx_device_shadow_buffer) read and written behind the library's back — TEST
INFRASTRUCTURE, tests/devbuf.py's counterpart for the plane rtx_render_shadows_async writes.

The plane is never cleared, so a shadow pass that repeats an earlier one lands on the right answer: `poison`
fills it with a word before the pass under test, and `check` reads it back raw (rtx_download_shadows copies
owned rows only) and demands the expected word in every row the pass owns and the sentinel everywhere else.

Rules for callers: poison and peek exactly n_views * width * height words, only after a shadow pass of that
shape has run on the context (the range is then inside the allocation); the expected plane must not contain the
sentinel, which has bits 31, 30, 28, ... set: no word of a scene with fewer than 32 lights."""
from __future__ import annotations

import numpy as np

import devbuf

SENTINEL = 0xDEADBEEF


def poison(ctx, n_words: int) -> None:
    ctx.synchronize()
    devbuf.fill(ctx, ctx.device_shadow_buffer(), n_words, SENTINEL)


def peek(ctx, n_words: int) -> np.ndarray:
    ctx.synchronize()
    return devbuf.read(ctx, ctx.device_shadow_buffer(), n_words)


def check(ctx, params, n_views: int, want, what: str = "") -> None:
    """Every word of an owned row equals `want` (one array per view, or the views concatenated) and is not the
    sentinel; every word of a row the pass does not own is still the sentinel."""
    W, H = int(params.width), int(params.height)
    n = W * H
    if isinstance(want, (list, tuple)):
        want = np.concatenate([np.asarray(x, np.uint32).reshape(-1) for x in want])
    want = np.asarray(want, np.uint32).reshape(n_views, H, W)
    got = peek(ctx, n_views * n).reshape(n_views, H, W)
    for v in range(n_views):
        own = devbuf.owned_rows(params, v)
        assert not (want[v][own] == np.uint32(SENTINEL)).any(), "an expected word is the sentinel"
        stale = int((got[v][own] == np.uint32(SENTINEL)).sum())
        assert stale == 0, f"{what} view {v}: {stale} owned words of the shadow plane were never written"
        bad = got[v][own] != want[v][own]
        assert not bad.any(), f"{what} view {v}: {int(bad.sum())} owned words differ from the checker's"
        other = got[v][~own]
        assert (other == np.uint32(SENTINEL)).all(), \
            f"{what} view {v}: {int((other != np.uint32(SENTINEL)).sum())} words of rows the pass does not own were written"
