"""The tile schedule's integer model (tests/sched_model.py) without a GPU: the class function against the
specification's table, the model's order against a literal serial counting sort, the threshold arithmetic at
its 64-bit end, and the two diagnostics entries the GPU tests drive (include/rtx_diag.h: rtx_schedule_run,
rtx_schedule_heavy): declared, exported, bound, their structs laid out as the C compiler lays them out, and a
NULL context refused without a device."""
import ctypes as C

import numpy as np

import abi_surface
import sched_model as sm
from gp1_raytracer_2223_amd import abi


def test_class_table_has_every_class_once():
    edges = sm.class_edges()
    assert [k for _, k in edges] == list(range(30, -1, -1))
    assert [e for e, _ in edges[:5]] == [48, 64, 96, 128, 192]
    assert edges[-2] == (1_048_576, 1) and edges[-1] == (1_572_864, 0)
    for (a, _), (b, _), (c, _) in zip(edges, edges[1:], edges[2:]):   # 3 * 2^(k-1) and 2^k in turn
        assert c == 2 * a and a < b < c


def test_class_at_every_edge():
    """e - 1 is the class above e's, e and e + 1 are e's; 0, 1 and 47 are class 31, 2^32 - 1 is class 0."""
    for e, k in sm.class_edges():
        assert sm.cost_class([e - 1, e, e + 1]).tolist() == [k + 1, k, k], e
    assert sm.cost_class([0, 1, 2, 3, 47, sm.U32_MAX - 1, sm.U32_MAX]).tolist() == [31, 31, 31, 31, 31, 0, 0]


def test_class_is_monotone():
    """Heavier never sorts later: over every cost up to 2^17, every power of two and its neighbours, and
    seeded costs over the whole range."""
    rng = np.random.default_rng(11)
    c = np.concatenate([np.arange(1 << 17, dtype=np.uint64),
                        np.array([(1 << k) + d for k in range(1, 32) for d in (-1, 0, 1)], np.uint64),
                        np.array([3 * (1 << k) + d for k in range(30) for d in (-1, 0, 1)], np.uint64),
                        rng.integers(0, 1 << 32, 50_000, dtype=np.uint64)])
    c.sort()
    k = sm.cost_class(c)
    assert np.all(np.diff(k) <= 0) and k[0] == 31 and k[-1] <= 1
    assert set(k.tolist()) == set(range(32))
    assert sm.bit_length([0, 1, 2, 3, 4, (1 << 31) - 1, 1 << 31, sm.U32_MAX]).tolist() == [0, 1, 2, 2, 3, 31, 32, 32]


def _counting_sort(classes):
    """The literal serial counting sort: count, exclusive prefix, then place the tiles in tile order."""
    count = [0] * sm.K_COST_BUCKETS
    for k in classes:
        count[k] += 1
    at, acc = [], 0
    for v in count:
        at.append(acc)
        acc += v
    out = [0] * len(classes)
    for t, k in enumerate(classes):
        out[at[k]] = t
        at[k] += 1
    return out


def test_order_is_the_serial_counting_sort():
    rng = np.random.default_rng(5)
    for n in (1, 5, 257, 1025, 4099):
        cost = (2.0 ** rng.uniform(0, 32, n)).astype(np.uint64).clip(0, sm.U32_MAX)
        saved = (2.0 ** rng.uniform(0, 32, n)).astype(np.uint64).clip(0, sm.U32_MAX)
        was = rng.integers(0, 2, n)
        for parts in (0, 1):
            m = sm.schedule(cost, saved, was, parts=parts, split_slots=7168, permille=1500, split_min=0, wave_slots=7168)
            eff = [int(s if w and not parts else c) for c, s, w in zip(cost, saved, was)]
            assert m["effective"].tolist() == eff
            assert m["order"].tolist() == _counting_sort(sm.cost_class(eff).tolist())
            assert m["saved_after"].tolist() == [int(s if w else c) for c, s, w in zip(cost, saved, was)]
            assert m["total"] == sum(eff) and m["heavy_n"][2] == max(eff)
            thr = max(sum(eff) * 1500 // (1000 * min(n, 7168)), 0)
            assert m["threshold"] == thr and m["heavy"].tolist() == [v > thr for v in eff]
            assert not m["cost_after"].any()


def test_threshold_arithmetic_stays_inside_64_bits():
    """The largest case of the GPU tests and beyond: 34,823 tiles of 2^32 - 1 at permille 4000."""
    n = 34_823
    cost = np.full(n, sm.U32_MAX, np.uint64)
    assert n * sm.U32_MAX * 4000 < 1 << 60
    m = sm.schedule(cost, cost, split_slots=7168, permille=4000, split_min=0, wave_slots=7168)
    assert m["total"] == n * sm.U32_MAX
    assert m["threshold"] == n * sm.U32_MAX * 4000 // (1000 * 7168) > sm.U32_MAX
    assert not m["heavy"].any() and m["heavy_n"] == [0, 0, sm.U32_MAX, sm.U32_MAX]   # the per-slot word saturates
    assert sm.schedule(cost, cost, split_slots=0, permille=4000, split_min=0, wave_slots=0)["threshold"] == sm.U64_MAX
    forced = sm.schedule(cost, cost, split_slots=sm.FORCE, permille=4000, split_min=9, wave_slots=0)
    assert forced["threshold"] == 0 and forced["heavy"].all() and forced["heavy_n"] == [n, 0, sm.U32_MAX, 0]


CASE_FIELDS = ["cost", "was_heavy", "saved", "n", "tiles_x", "tiles_y", "parts", "split_slots", "permille",
               "split_min", "wave_slots", "xcd"]
RESULT_FIELDS = ["order", "order_xcd", "cost_after", "saved_after", "heavy_flag", "heavy_list", "heavy_n", "threshold"]


def test_header_declares_and_abi_binds_the_schedule_diagnostics(tmp_path):
    prints = ['printf("case %zu\\n", sizeof(rtx_schedule_case));', 'printf("result %zu\\n", sizeof(rtx_schedule_result));',
              'printf("cap %d\\n", RTX_MAX_HEAVY_TILES);']
    prints += [f'printf("case.{f} %zu\\n", offsetof(rtx_schedule_case, {f}));' for f in CASE_FIELDS]
    prints += [f'printf("result.{f} %zu\\n", offsetof(rtx_schedule_result, {f}));' for f in RESULT_FIELDS]
    out = abi_surface.declared_exported_and_bound(tmp_path, {}, {
        "rtx_schedule_run": "int (*)(rtx_ctx*, const rtx_schedule_case*, rtx_schedule_result*)",
        "rtx_schedule_heavy": "int (*)(rtx_ctx*, uint32_t*, uint32_t, uint32_t*, uint32_t*, uint64_t*, uint32_t*)",
    }, ["RTX_ABI_VERSION == 2"], statements=prints)
    c = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    assert c["case"] == C.sizeof(abi.ScheduleCase) and c["result"] == C.sizeof(abi.ScheduleResult)
    assert c["cap"] == abi.MAX_HEAVY_TILES == sm.K_MAX_HEAVY_TILES
    assert [n for n, _ in abi.ScheduleCase._fields_] == CASE_FIELDS
    assert [n for n, _ in abi.ScheduleResult._fields_] == RESULT_FIELDS
    for f in CASE_FIELDS:
        assert c[f"case.{f}"] == getattr(abi.ScheduleCase, f).offset, f
    for f in RESULT_FIELDS:
        assert c[f"result.{f}"] == getattr(abi.ScheduleResult, f).offset, f
    lib = abi.load_hip()
    assert lib.rtx_schedule_run.argtypes[1]._type_ is abi.ScheduleCase
    assert lib.rtx_schedule_run.argtypes[2]._type_ is abi.ScheduleResult


def test_null_context_is_invalid_without_a_device():
    lib = abi.load_hip()
    case, res = abi.ScheduleCase(), abi.ScheduleResult()
    assert lib.rtx_schedule_run(None, C.byref(case), C.byref(res)) == abi.RTX_E_INVALID
    assert lib.rtx_schedule_heavy(None, None, 0, None, None, None, None) == abi.RTX_E_INVALID
