"""The cost-ordered dispatch computed on the device by rtx_sched_count / _scan / _scatter
(three multi-workgroup launches): after a measured frame the dispatch order must be a
permutation of the tiles, heaviest cost class first and, within a class, in tile order
(a stable counting sort) — checked against the measured one-piece costs it was sorted by.

And the same launches on injected costs (rtx_schedule_run, which queues them through the one function
a frame's update queues them through): every output — the order, its XCD re-deal, the heavy threshold,
flags, list and counter words, the saved-cost fix-up, the cleared costs — is compared, integer for
integer, with the model of tests/sched_model.py, at the tile counts that reach every thread, workgroup,
chunk and scan-segment edge and on costs no rendered frame produces (zeros, class edges, 2^32 - 1).  Two
tests on rendered frames (rtx_schedule_heavy) cover what the harness cannot: the wiring in sched_update."""
import ctypes as C

import numpy as np
import pytest
import torch   # noqa: F401  (at collection, before librtx_hip.so is loaded)

import gpu_support as gs
import sched_model as sm
import xcd_model
from gp1_raytracer_2223_amd import abi
from gp1_raytracer_2223_amd.scene import HostScene
from gpu_support import ctx  # noqa: F401
from sched_model import cost_class

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,W,H,views", [("W4_Bunny", 1920, 1080, 1), ("Bunny8Lights", 3840, 2160, 1),
                                            ("W4_Optional", 1920, 1080, 1), ("W3", 1280, 720, 8)])
def test_dispatch_order_is_stable_counting_sort(gpu_ctx, name, W, H, views):
    hs = HostScene(name)
    s, cam = hs.view()
    gpu_ctx.upload(s)
    p = abi.make_params(W, H)
    cams = (abi.Camera * views)(*([cam] * views))
    lib = gpu_ctx.lib
    for _ in range(2):   # frame 1 measures; frame 2 runs in that order
        abi.check(lib.rtx_render_views_async(gpu_ctx.h, cams, views, C.byref(p), 0), "render", gpu_ctx.h)
    gpu_ctx.synchronize()
    n = C.c_uint32()
    abi.check(lib.rtx_schedule_state(gpu_ctx.h, None, None, 0, C.byref(n)), "schedule_state", gpu_ctx.h)
    ntiles = ((W + 7) // 8) * ((H + 7) // 8) * views
    assert n.value >= ntiles
    order = np.zeros(ntiles, np.uint32)
    cost = np.zeros(ntiles, np.uint32)
    abi.check(lib.rtx_schedule_state(gpu_ctx.h, order.ctypes.data_as(C.POINTER(C.c_uint32)),
                                     cost.ctypes.data_as(C.POINTER(C.c_uint32)), ntiles, C.byref(n)),
              "schedule_state", gpu_ctx.h)
    assert np.array_equal(np.sort(order), np.arange(ntiles, dtype=np.uint32)), "not a permutation"
    cls = cost_class(cost)
    expect = np.lexsort((np.arange(ntiles), cls)).astype(np.uint32)   # by class, then tile index
    assert np.array_equal(order, expect)
    assert cost.max() > 0


@pytest.fixture(scope="module")
def xcd_ctx():
    """A context that dispatches in the XCD-affine re-deal of the cost order (RTX_XCD_ORDER=1)."""
    import os
    from gp1_raytracer_2223_amd.renderer import DeviceContext
    os.environ["RTX_XCD_ORDER"] = "1"
    try:
        ctx = DeviceContext(int(os.environ.get("RTX_TEST_DEVICE", "0")))
    finally:
        del os.environ["RTX_XCD_ORDER"]
    yield ctx
    ctx.close()


# tiles_x, tiles_y, views (8 x 8 wave tiles): tests/test_xcd_model.py's shapes
XCD_SHAPES = [(41, 33, 1), (41, 25, 1), (5, 4, 1), (12, 9, 3), (64, 16, 1), (1, 1, 1)]


@pytest.mark.parametrize("tx,ty,views", XCD_SHAPES)
def test_xcd_order_is_the_model_redeal_of_the_cost_order(xcd_ctx, gpu_ctx, tx, ty, views):
    """rtx_sched_xcd's output, the permutation the render kernel consumes under RTX_XCD_ORDER=1, equals
    the numpy model (tests/xcd_model.py) applied to the cost order of the same measured frame."""
    import xcd_model
    hs = HostScene("W4_Bunny")
    s, cam = hs.view()
    xcd_ctx.upload(s)
    p = abi.make_params(8 * tx, 8 * ty)
    cams = (abi.Camera * views)(*([cam] * views))
    lib = xcd_ctx.lib
    ntiles = tx * ty * views
    got = np.full(ntiles, 0xDEADBEEF, np.uint32)
    up = C.POINTER(C.c_uint32)
    for _ in range(2):   # frame 1 measures; frame 2 runs in the re-dealt order
        abi.check(lib.rtx_render_views_async(xcd_ctx.h, cams, views, C.byref(p), 0), "render", xcd_ctx.h)
    xcd_ctx.synchronize()
    order = np.zeros(ntiles, np.uint32)
    cost = np.zeros(ntiles, np.uint32)
    n = C.c_uint32()
    abi.check(lib.rtx_schedule_state(xcd_ctx.h, order.ctypes.data_as(up), cost.ctypes.data_as(up), ntiles, C.byref(n)),
              "schedule_state", xcd_ctx.h)
    assert n.value >= ntiles
    assert np.array_equal(np.sort(order), np.arange(ntiles, dtype=np.uint32)), "the cost order is not a permutation"
    abi.check(lib.rtx_schedule_xcd_order(xcd_ctx.h, got.ctypes.data_as(up), ntiles), "schedule_xcd_order", xcd_ctx.h)
    assert np.array_equal(np.sort(got), np.arange(ntiles, dtype=np.uint32)), "the XCD order is not a permutation"
    assert np.array_equal(got, xcd_model.redeal(order, tx, ty))
    # a context without the knob has no XCD order
    assert lib.rtx_schedule_xcd_order(gpu_ctx.h, got.ctypes.data_as(up), 1) == abi.RTX_E_STATE


# ---- the schedule's launches on injected costs (rtx_schedule_run) -----------------------------------------

K = 1024   # kSchedChunk: tiles per workgroup of the count and the scatter (256 threads, 4 tiles each)
# thread (4), workgroup (256) and chunk (1024) edges; 31 K, 32 K, 32 K + 1: the scan's 1,024 threads go from
# one (class, chunk) entry each to two; the heavy cap, one past it and 8320
COUNTS = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2049, 31 * K, 32 * K, 32 * K + 1, 33 * K + 7, 8192, 8193, 8320]
SOME = [5, 257, 1025, 2049, 32 * K + 1]
SLOTS = 7168           # 28 waves on each of 256 CUs: below the larger counts, above the smaller
SEL = dict(split_slots=SLOTS, permille=1500, split_min=0, wave_slots=SLOTS)
U32 = sm.U32_MAX


def _log_uniform(n, seed):
    """Seeded, log-uniform over [0, 2^32): every class is hit."""
    u = np.random.default_rng(seed).uniform(0.0, 32.0, n)
    return (np.minimum(np.floor(2.0 ** u), float(1 << 32)) - 1).astype(np.uint64).astype(np.uint32)


def _ladder(n):
    """Every class edge e as e - 1, e, e + 1, with 0 and 2^32 - 1, tiled over the count."""
    rungs = [0] + [e + d for e, _ in sm.class_edges() for d in (-1, 0, 1)] + [U32]
    return np.array([rungs[t % len(rungs)] for t in range(n)], np.uint32)


def _one_huge(n, at):
    c = np.zeros(n, np.uint32)
    c[at] = U32
    return c


PATTERNS = {
    "zero": lambda n: np.zeros(n, np.uint32),
    "equal": lambda n: np.full(n, 1000, np.uint32),
    "max": lambda n: np.full(n, U32, np.uint32),
    "ascending": lambda n: (40 + 37 * np.arange(n)).astype(np.uint32),
    "descending": lambda n: (40 + 37 * np.arange(n))[::-1].astype(np.uint32),
    "two_classes": lambda n: np.where(np.arange(n) % 2 == 0, 1000, 100_000).astype(np.uint32),
    "two_classes_by_3": lambda n: np.where(np.arange(n) // 3 % 2 == 0, 100_000, 1000).astype(np.uint32),
    "ladder": _ladder,
    "log_uniform": lambda n: _log_uniform(n, 1000 + n),
    "huge_first": lambda n: _one_huge(n, 0),
    "huge_last": lambda n: _one_huge(n, n - 1),
}
PATTERN_CASES = [(name, n) for name in PATTERNS for n in (COUNTS if name in ("ladder", "log_uniform") else SOME)]


def _check(got, want, n):
    """Every output of one run against the model, integer for integer."""
    assert np.array_equal(got["order"], want["order"])
    assert not got["cost_after"].any()
    assert np.array_equal(got["saved_after"], want["saved_after"])
    assert got["threshold"] == want["threshold"]
    assert got["heavy_n"] == want["heavy_n"]
    count = got["heavy_n"][0]
    entries = sm.listed(got["heavy_list"], count)
    flagged = np.flatnonzero(got["heavy_flag"])
    assert set(np.unique(got["heavy_flag"]).tolist()) <= {0, 1}
    assert entries.size == 0 or int(entries.max()) < n
    assert np.unique(entries).size == entries.size, "a tile is listed twice"
    assert np.array_equal(np.sort(entries), flagged), "flags and list hold different sets"
    assert (got["heavy_list"][entries.size:] == U32).all(), "the list was written past the count"
    if count <= sm.K_MAX_HEAVY_TILES:
        assert np.array_equal(got["heavy_flag"] != 0, want["heavy"])
    else:
        assert flagged.size == sm.K_MAX_HEAVY_TILES


def _run(c, cost, saved=None, was=None, *, tiles=None, xcd=False, parts=0, **sel):
    """One case, run twice: the same order both times, and every output of both runs the model's."""
    n = cost.size
    saved = cost if saved is None else saved
    tx, ty = tiles or (n, 1)
    want = sm.schedule(cost, saved, was, parts=parts, **sel)
    runs = [c.schedule_run(cost, saved, was, tiles_x=tx, tiles_y=ty, parts=parts, xcd=xcd, **sel) for _ in range(2)]
    assert np.array_equal(runs[0]["order"], runs[1]["order"]), "two runs, two orders"
    for got in runs:
        _check(got, want, n)
        if xcd:
            assert np.array_equal(got["order_xcd"], xcd_model.redeal(want["order"], tx, ty))
    return runs[0], want


@pytest.mark.parametrize("name,n", PATTERN_CASES, ids=lambda v: str(v))
def test_injected_costs(ctx, name, n):   # noqa: F811
    cost = PATTERNS[name](n)
    got, want = _run(ctx, cost, **SEL)
    if name == "max" and n > SLOTS:
        assert got["heavy_n"][3] == U32 < want["total"] // SLOTS, "the cost per wave slot saturates"
    if name.startswith("huge") and n > 1:
        assert got["heavy_n"][0] == 1 and got["heavy_list"][0] == (0 if name == "huge_first" else n - 1)
    if name == "ladder" and n >= 95:
        assert set(cost_class(cost).tolist()) == set(range(32)), "the ladder visits every class"


def test_injected_costs_at_the_largest_count(ctx):   # noqa: F811
    """2^20 tiles, the most rtx_schedule_run accepts: 1,024 chunks, one per scan thread."""
    _run(ctx, _log_uniform(1 << 20, 20), **SEL)


T = 100_000   # the threshold the selection cases are built around


def _selection_costs(n, m, permille, seed):
    """Costs whose share, total * permille // (1000 m), is exactly T, with k tiles each at T, T + 1, T + 5,
    T + 6 (T + 5 is the `split_min` of the cases whose floor lies above the share) and 2 T, and the rest
    below T."""
    k = max(1, n // 100)
    total = -(-T * 1000 * m // permille)   # the least total whose share is T
    fixed = [T, T + 1, T + 5, T + 6, 2 * T] * k
    rest = total - sum(fixed)
    q, r = divmod(rest, n - 5 * k)
    assert 0 <= q < T - 1
    cost = np.array(fixed + [q + 1] * r + [q] * (n - 5 * k - r), np.uint32)
    assert int(cost.sum(dtype=np.uint64)) * permille // (1000 * m) == T
    return np.random.default_rng(seed).permutation(cost)


def _selection_cases():
    for n in (1025, 32 * K + 1):
        for slots in (n // 3, 4 * n + 1):
            for permille in (1000, 1500, 2600, 4000):
                for floor in ("none", "below", "above"):
                    yield n, slots, permille, floor
        for slots in (0, sm.FORCE):
            for floor in ("none", "above"):
                yield n, slots, 1500, floor


@pytest.mark.parametrize("n,slots,permille,floor", list(_selection_cases()), ids=lambda v: str(v))
def test_heavy_selection(ctx, n, slots, permille, floor):   # noqa: F811
    """The threshold, its split_min floor and the strict `>`: tiles that cost exactly the threshold are
    light, tiles that cost one more are heavy."""
    m = min(n, slots) if slots not in (0, sm.FORCE) else n
    cost = _selection_costs(n, m, permille, n + permille)
    split_min = {"none": 0, "below": T // 2, "above": T + 5}[floor]
    got, want = _run(ctx, cost, split_slots=slots, permille=permille, split_min=split_min, wave_slots=SLOTS)
    if slots == 0:
        assert got["threshold"] == sm.U64_MAX and got["heavy_n"][0] == 0
    elif slots == sm.FORCE:
        assert got["threshold"] == 0 and got["heavy_n"][0] == n
    else:
        thr = T + 5 if floor == "above" else T
        k = max(1, n // 100)
        assert got["threshold"] == thr
        assert (cost == thr).sum() == k and (cost == thr + 1).sum() == k
        assert not got["heavy_flag"][cost == thr].any() and got["heavy_flag"][cost == thr + 1].all()
        assert got["heavy_n"][0] == (2 * k if floor == "above" else 4 * k)


@pytest.mark.parametrize("n", [8192, 8193, 8320])
def test_heavy_cap(ctx, n):   # noqa: F811
    """Every tile forced heavy at the cap, one past it and 128 past it: the count is not clamped, exactly
    kMaxHeavyTiles flags are set, and the flagged tiles are the listed ones, each once and below n."""
    got, _ = _run(ctx, _log_uniform(n, 7), split_slots=sm.FORCE, permille=1500, split_min=0, wave_slots=SLOTS)
    entries = got["heavy_list"]
    assert got["heavy_n"][0] == n
    assert int((got["heavy_flag"] != 0).sum()) == sm.K_MAX_HEAVY_TILES == entries.size
    assert set(np.flatnonzero(got["heavy_flag"]).tolist()) == set(entries.tolist())
    assert np.unique(entries).size == entries.size and int(entries.max()) < n


def _was_heavy(which, n):
    t = np.arange(n)
    return {"null": None, "none": np.zeros(n, np.uint32), "all": np.ones(n, np.uint32),
            "third": (t % 3 == 0).astype(np.uint32),
            "one_chunk": ((t >= K) & (t < 2 * K)).astype(np.uint32)}[which]


@pytest.mark.parametrize("parts", [0, 1])
@pytest.mark.parametrize("which", ["null", "none", "all", "third", "one_chunk"])
@pytest.mark.parametrize("n", [1025, 2049, 32 * K + 1])
def test_saved_cost_fixup(ctx, n, which, parts):   # noqa: F811
    """A tile that was rendered split sorts and selects by its saved one-piece cost (static frames) or by its
    part sum (`parts`, motion mode), and keeps its saved cost either way."""
    cost = _log_uniform(n, 31 + n)
    saved = _log_uniform(n, 57 + n)
    # a saved cost of another class than the tile's cost: class 30 for a heavy tile, class 0 for a light one
    same = cost_class(saved) == cost_class(cost)
    other = np.where(cost_class(cost) < 16, 48 + np.arange(n) % 16, 3_000_000 + np.arange(n))
    saved = np.where(same, other, saved).astype(np.uint32)
    assert (cost_class(saved) != cost_class(cost)).all()
    was = _was_heavy(which, n)
    got, want = _run(ctx, cost, saved, was, parts=parts, **SEL)
    w = np.zeros(n, bool) if was is None else was != 0
    assert np.array_equal(got["saved_after"][w], saved[w]), "a split tile lost its saved one-piece cost"
    assert np.array_equal(got["saved_after"][~w], cost[~w])
    eff = np.where(w & (parts == 0), saved, cost)
    assert got["heavy_n"][2] == int(eff.max())
    assert np.array_equal(got["order"], np.lexsort((np.arange(n), cost_class(eff))))
    assert np.array_equal(got["heavy_flag"] != 0, eff > got["threshold"])
    if w.any() and parts == 0:
        assert not np.array_equal(want["order"], sm.schedule(cost, saved, None, **SEL)["order"]), "a vacuous case"


@pytest.mark.parametrize("tx,ty,views", XCD_SHAPES)
def test_injected_xcd_redeal(ctx, tx, ty, views):   # noqa: F811
    n = tx * ty * views
    got, _ = _run(ctx, _log_uniform(n, 77 + n), tiles=(tx, ty), xcd=True, **SEL)
    assert np.array_equal(np.sort(got["order_xcd"]), np.arange(n, dtype=np.uint32))


def _raw_run(c, n, **over):
    """rtx_schedule_run's return code for n tiles with valid arguments, but for `over`."""
    keep = [np.zeros(max(n, 1), np.uint32) for _ in range(8)]
    keep.append(np.zeros(abi.MAX_HEAVY_TILES, np.uint32))
    p = [a.ctypes.data_as(gs.UP) for a in keep]
    case = abi.ScheduleCase(p[0], p[1], p[2], n, max(n, 1), 1, 0, SLOTS, 1500, 0, SLOTS, 0)
    res = abi.ScheduleResult(p[3], p[4], p[5], p[6], p[7], p[8])
    for k, v in over.items():
        setattr(case if hasattr(case, k) else res, k, v)
    return c.lib.rtx_schedule_run(c.h, C.byref(case), C.byref(res))


def test_the_harness_refuses_and_leaves_the_context_alone(ctx):   # noqa: F811
    null = C.POINTER(C.c_uint32)()
    assert _raw_run(ctx, 16) == abi.RTX_OK and _raw_run(ctx, 16, was_heavy=null) == abi.RTX_OK
    assert _raw_run(ctx, 0) == abi.RTX_E_INVALID
    assert _raw_run(ctx, (1 << 20) + 1) == abi.RTX_E_INVALID
    for name in ("cost", "saved", "order", "cost_after", "saved_after", "heavy_flag", "heavy_list"):
        assert _raw_run(ctx, 16, **{name: null}) == abi.RTX_E_INVALID, name
    assert _raw_run(ctx, 16, order_xcd=null) == abi.RTX_OK
    assert _raw_run(ctx, 16, order_xcd=null, xcd=1) == abi.RTX_E_INVALID
    assert _raw_run(ctx, 16, tiles_x=0) == abi.RTX_E_INVALID and _raw_run(ctx, 16, tiles_y=0) == abi.RTX_E_INVALID
    assert _raw_run(ctx, 16, tiles_x=5, tiles_y=1, xcd=1) == abi.RTX_E_INVALID
    assert _raw_run(ctx, 16, tiles_x=5, tiles_y=1) == abi.RTX_OK   # (only the re-deal needs whole views)
    assert _raw_run(ctx, 16, tiles_x=4, tiles_y=2, xcd=1) == abi.RTX_OK
    assert ctx.lib.rtx_schedule_run(ctx.h, None, None) == abi.RTX_E_INVALID
    # no frame yet: nothing to read out, and a run changes that as little
    assert ctx.lib.rtx_schedule_heavy(ctx.h, None, 0, None, None, None, None) == abi.RTX_E_STATE
    s, cam = gs.view("Synthetic100k")
    p = abi.make_params(320, 180)
    n = 40 * 23
    ctx.upload(s)
    frames = [ctx.render(cam, p)[0] for _ in range(2)]   # a measured frame, a frame in its order

    def state():
        order, cost = ctx.schedule_state(n)
        h = ctx.schedule_heavy(n)
        return [order, cost, h.pop("heavy_flag"), h.pop("heavy_list")], (h, ctx.split_info(), ctx.split_tune_info()["factor"])

    before = state()
    for slots in (sm.FORCE, 0, SLOTS):
        _run(ctx, _log_uniform(1025, 3), split_slots=slots, permille=4000, split_min=7, wave_slots=3)
    after = state()
    assert before[1] == after[1]
    for a, b in zip(before[0], after[0]):
        assert np.array_equal(a, b)
    frames.append(ctx.render(cam, p)[0])
    assert np.array_equal(frames[0], frames[1]) and np.array_equal(frames[0], frames[2])


# ---- the real path's wiring: what sched_update passes and selects (rtx_schedule_heavy) -----------------------

def _model_of_measurement(c, n, was=None):
    """The schedule read back after a measurement and the model of it: the costs read are the saved one-piece
    costs, which are the effective costs of a static frame's update (a split tile sorts by its saved cost)."""
    order, cost = c.schedule_state(n)
    h = c.schedule_heavy(n)
    want = sm.schedule(cost, cost, None, split_slots=h["split_slots"], permille=h["permille"],
                       split_min=h["split_min"], wave_slots=h["wave_slots"])
    assert np.array_equal(order, want["order"])
    assert h["threshold"] == want["threshold"] and h["heavy_n"] == want["heavy_n"]
    assert np.array_equal(h["heavy_flag"] != 0, want["heavy"])
    assert want["heavy_n"][0] <= sm.K_MAX_HEAVY_TILES
    assert set(sm.listed(h["heavy_list"], h["heavy_n"][0]).tolist()) == set(np.flatnonzero(want["heavy"]).tolist())
    return cost, h, want


def test_measured_frame_selects_what_the_model_selects():
    """RTX_SPLIT_FACTOR=1 and RTX_SPLIT_MIN_US=0: the threshold is the mean tile cost (920 tiles, fewer than
    the wave slots), so a frame whose tiles do not all cost the same has heavy and light tiles."""
    _, dev = gs.torch_device()
    slots = 28 * torch.cuda.get_device_properties(dev).multi_processor_count
    c = gs.ctx_env(RTX_SPLIT_FACTOR="1", RTX_SPLIT_MIN_US="0")
    try:
        s, cam = gs.view("Synthetic100k")
        p = abi.make_params(320, 180)
        n = 40 * 23
        c.upload(s)
        for _ in range(2):
            c.render(cam, p)
        cost, h, want = _model_of_measurement(c, n)
        assert (h["permille"], h["split_min"], h["split_slots"], h["wave_slots"]) == (1000, 0, slots, slots)
        assert h["threshold"] == int(cost.sum(dtype=np.uint64)) // n
        assert c.split_info()[0] == h["heavy_n"][0]
        assert 0 < h["heavy_n"][0] < n
    finally:
        c.close()


def test_split_tiles_keep_their_saved_cost_across_measurements():
    """RTX_SCHED_PERIOD=2, a static camera: frame 1 measures, frame 2 splits what it selected, frame 3 is split
    and measured: its update keeps the saved one-piece cost of every tile that was split, word for word, and
    sorts and selects by it."""
    c = gs.ctx_env(RTX_SPLIT_FACTOR="1", RTX_SPLIT_MIN_US="0", RTX_SCHED_PERIOD="2")
    try:
        s, cam = gs.view("Synthetic100k")
        p = abi.make_params(320, 180)
        n = 40 * 23
        c.upload(s)
        first = c.render(cam, p)[0]
        c.render(cam, p)
        cost1, h1, _ = _model_of_measurement(c, n)
        split = h1["heavy_flag"] != 0
        assert 0 < split.sum() < n and c.split_info()[0] == split.sum()
        last = c.render(cam, p)[0]   # the second measurement, of a frame that split those tiles
        cost2, h2, _ = _model_of_measurement(c, n)
        assert np.array_equal(cost2[split], cost1[split]), "a split tile lost its saved one-piece cost"
        assert (cost2[~split] != cost1[~split]).any(), "no second measurement: the one-piece tiles' costs are the first's"
        assert np.array_equal(last, first)
    finally:
        c.close()
