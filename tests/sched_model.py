"""The tile schedule (rtx_sched_count / _scan / _scatter, csrc/rtx_sched.hip) as an integer model — TEST
INFRASTRUCTURE.  Written from the schedule's specification, not from the kernels' three passes; plain
Python and numpy integers only, no float anywhere.

  * A tile's effective cost is saved[t] if was_heavy[t] and not `parts`, else cost[t].  saved_after is
    unchanged where was_heavy[t] and cost[t] elsewhere; cost_after is all zero.
  * class(c) = 31 - clamp(2 L + h - 12, 0, 31), L the bit length of c and h its bit L - 2 (0 for c < 2):
    class 31 below 48, a new class at 48, 64, 96, 128, 192, ... (3 * 2^(k-1) and 2^k in turn), class 1 from
    2^20 and class 0 from 3 * 2^19 up.
  * order: the tiles sorted by (class of the effective cost, tile index).
  * total: the sum of the effective costs.  threshold: 2^64 - 1 for slots == 0, 0 for slots == 0xffffffff
    (every tile heavy), else max(total * permille // (1000 * min(n, slots)), split_min); a tile is heavy
    when its effective cost is GREATER than the threshold.
  * heavy_n = [heavy tiles (not clamped), 0, largest effective cost,
               min(total // min(n, wave_slots), 2^32 - 1) or 0 for wave_slots == 0].
  * Flags and the first min(count, K_MAX_HEAVY_TILES) list entries hold the same set, the heavy tiles
    when the count is within the cap; the list's order is unspecified (an atomic appends to it)."""
from __future__ import annotations

import numpy as np

K_COST_BUCKETS = 32
K_MAX_HEAVY_TILES = 8192
FORCE = 0xFFFFFFFF
U32_MAX = 0xFFFFFFFF
U64_MAX = (1 << 64) - 1


def bit_length(c) -> np.ndarray:
    """Bits of each cost (0 for 0, 32 for 2^31 and up), by shifts alone."""
    c = np.asarray(c, np.uint64)
    bits = np.zeros(c.shape, np.int64)
    for k in range(32):
        bits += (c >> np.uint64(k)) != 0
    return bits


def cost_class(c) -> np.ndarray:
    """The class of each cost: two per octave, heavier first."""
    c = np.asarray(c, np.uint64)
    assert c.size == 0 or int(c.max()) <= U32_MAX
    bits = bit_length(c)
    half = np.where(bits >= 2, (c >> np.maximum(bits - 2, 0).astype(np.uint64)) & np.uint64(1), 0).astype(np.int64)
    return (K_COST_BUCKETS - 1) - np.clip(2 * bits + half - 12, 0, K_COST_BUCKETS - 1)


def class_edges() -> list[tuple[int, int]]:
    """The table of the specification, (first cost, class) from class 30 down to 0: 48, 64, 96, 128, ...,
    2^20 (class 1), 3 * 2^19 (class 0).  Below 48 is class 31.  Stated on its own, not through cost_class."""
    edges, k = [], 5
    while len(edges) < K_COST_BUCKETS - 1:
        edges.append((3 << (k - 1), K_COST_BUCKETS - 2 - len(edges)))
        if len(edges) < K_COST_BUCKETS - 1:
            edges.append((1 << (k + 1), K_COST_BUCKETS - 2 - len(edges)))
        k += 1
    return edges


def schedule(cost, saved, was_heavy=None, *, parts=0, split_slots, permille, split_min, wave_slots) -> dict:
    """The outputs of one schedule update for n tiles; `heavy` is the heavy tiles as a bool array."""
    cost = np.asarray(cost, np.uint64)
    saved = np.asarray(saved, np.uint64)
    n = cost.size
    was = np.zeros(n, bool) if was_heavy is None else np.asarray(was_heavy) != 0
    assert n > 0 and saved.size == n and was.size == n
    eff = np.where(was & (not parts), saved, cost)
    total = int(eff.sum(dtype=np.uint64))   # (n <= 2^20 costs below 2^32: no wrap)
    assert total * permille <= U64_MAX, "outside the 64-bit domain of the threshold"
    if split_slots == 0:
        threshold = U64_MAX
    elif split_slots == FORCE:
        threshold = 0
    else:
        threshold = max(total * permille // (1000 * min(n, split_slots)), split_min)
    heavy = np.ones(n, bool) if split_slots == FORCE else eff > np.uint64(threshold)
    per_slot = min(total // min(n, wave_slots), U32_MAX) if wave_slots else 0
    return {"order": np.lexsort((np.arange(n), cost_class(eff))).astype(np.uint32),
            "cost_after": np.zeros(n, np.uint32),
            "saved_after": np.where(was, saved, cost).astype(np.uint32),
            "effective": eff.astype(np.uint32), "total": total, "threshold": threshold, "heavy": heavy,
            "heavy_n": [int(heavy.sum()), 0, int(eff.max()), per_slot]}


def listed(heavy_list, count) -> np.ndarray:
    """The list's valid entries: the first min(count, K_MAX_HEAVY_TILES)."""
    return np.asarray(heavy_list)[:min(int(count), K_MAX_HEAVY_TILES)]
