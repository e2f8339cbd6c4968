"""The XCD-affine re-deal of the dispatch order (rtx_sched_xcd, RTX_XCD_ORDER=1) as a numpy model —
TEST INFRASTRUCTURE.  Written from the pass's specification in csrc/rtx_sched.hip, not from the
kernel's three passes:

  * a tile's class is (i + 3 j) mod 8, where (i, j) is the block of the 8 x 8 grid over its view that
    holds it: i = bx * 8 // tiles_x, j = gy * 8 // tiles_y for the tile's column bx and row gy within
    the view (tile = view * tiles_x * tiles_y + gy * tiles_x + bx);
  * m is the smallest class count (0 when a class is empty: fewer than 8 tile columns or rows);
  * position 8 k + r holds the k-th tile of class r in input order, for k < m;
  * every other tile follows from position 8 m, in input order."""
from __future__ import annotations

import numpy as np


def region(tile, tiles_x: int, tiles_y: int) -> np.ndarray:
    t = np.asarray(tile, np.int64)
    rem = t % (tiles_x * tiles_y)
    bx, gy = rem % tiles_x, rem // tiles_x
    return (bx * 8 // tiles_x + 3 * (gy * 8 // tiles_y)) % 8


def smallest_class(order, tiles_x: int, tiles_y: int) -> int:
    return int(np.bincount(region(order, tiles_x, tiles_y), minlength=8).min())


def redeal(order, tiles_x: int, tiles_y: int) -> np.ndarray:
    order = np.asarray(order, np.uint32)
    r = region(order, tiles_x, tiles_y)
    m = smallest_class(order, tiles_x, tiles_y)
    rank = np.zeros(order.size, np.int64)   # a tile's rank among the tiles of its class, in input order
    for c in range(8):
        at = np.flatnonzero(r == c)
        rank[at] = np.arange(at.size)
    dealt = rank < m
    out = np.empty_like(order)
    out[8 * rank[dealt] + r[dealt]] = order[dealt]
    out[8 * m:] = order[~dealt]
    return out
