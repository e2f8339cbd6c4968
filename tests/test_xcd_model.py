"""The numpy model of the XCD-affine re-deal (tests/xcd_model.py) checked on its own, without a GPU:
tests/test_gpu_schedule.py compares the device's permutation with it."""
import numpy as np
import pytest

import xcd_model

# tiles_x, tiles_y, views: two scheduling chunks with the second partial, one tile past a chunk, fewer
# than 8 tile columns and rows (classes of 3 and of 2 tiles), three views, exactly one tile per scan
# thread, and a single tile (seven empty classes: m = 0, nothing is dealt)
SHAPES = [(41, 33, 1), (41, 25, 1), (5, 4, 1), (12, 9, 3), (64, 16, 1), (1, 1, 1)]


@pytest.mark.parametrize("tx,ty,views", SHAPES)
@pytest.mark.parametrize("seed", [0, 1])
def test_redeal_is_the_specified_permutation(tx, ty, views, seed):
    n = tx * ty * views
    order = np.random.default_rng(1000 * seed + n).permutation(n).astype(np.uint32)
    out = xcd_model.redeal(order, tx, ty)
    assert out.dtype == np.uint32 and out.shape == (n,)
    assert np.array_equal(np.sort(out), np.arange(n, dtype=np.uint32)), "not a permutation"
    m = xcd_model.smallest_class(order, tx, ty)
    cls = xcd_model.region(out, tx, ty)
    assert np.array_equal(cls[:8 * m], np.arange(8 * m) % 8), "a position below 8m holds the wrong class"
    where = np.empty(n, np.int64)   # a tile's position in the input order
    where[order] = np.arange(n)
    for r in range(8):   # within a class the dealt tiles keep the input order
        assert (np.diff(where[out[r:8 * m:8]]) > 0).all()
    rest = where[out[8 * m:]]
    assert (np.diff(rest) > 0).all(), "the tiles past 8m are not in input order"
    for r in range(8):   # ... and each is later in the input than every dealt tile of its class
        dealt, later = where[out[r:8 * m:8]], rest[cls[8 * m:] == r]
        assert not dealt.size or not later.size or dealt.max() < later.min()


def test_class_counts_of_small_views():
    """A view of one tile has seven empty classes (m = 0).  5 x 4 tiles: i takes the values 0, 1, 3,
    4, 6 and 3 j mod 8 the values 0, 6, 4, 2, so every class is reached: the even ones by three
    columns (3 tiles each... 12 tiles over 4 classes), the odd ones by two (2 tiles each)."""
    assert xcd_model.smallest_class(np.arange(1), 1, 1) == 0
    counts = np.bincount(xcd_model.region(np.arange(20), 5, 4), minlength=8)
    assert counts.tolist() == [3, 2, 3, 2, 3, 2, 3, 2] and xcd_model.smallest_class(np.arange(20), 5, 4) == 2
    # the Latin square: with 8 x 8 tiles every class holds exactly 8
    assert (np.bincount(xcd_model.region(np.arange(64), 8, 8), minlength=8) == 8).all()
