"""The cull decision of every adversarial case, pinned on the CPU: tests/pack_harness.cpp packs each of
tests/cull_cases.py's 59 scenes with min_sa=0 (the device tests' RTX_CULL_MIN_SA=0) and the packer's
cull_on and tri_fast must equal cull_cases.TABLE.  tests/test_gpu_cull_fuzz.py asserts the same table
against rtx_cull_info after each upload, so a device run in which the cull silently stayed off fails there,
and a table that drifted from the packer fails here."""
import pytest

import cull_cases as CC
import cull_domains as CD
import mesh_fuzz
from test_pack_cpu import build_harness, parse, run_harness


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("pack"))


@pytest.fixture(scope="module")
def packed(harness, tmp_path_factory):
    """label -> the harness's fields: every case with min_sa=0; the mesh cases after their first Update time
    too (`@t`); and every case under the product's ratio (`@product`)."""
    folder = tmp_path_factory.mktemp("cull_cases")
    script = [CC.harness_line(c, folder) for c in CC.CASES]
    script += [CC.harness_line(c, folder, f"t={mesh_fuzz.FIRST_TIME}").replace(f"scene {c.name} ", f"scene {c.name}@t ")
               for c in CC.MESH]
    script += [CC.harness_line(c, folder).replace(" min_sa=0", "").replace(f"scene {c.name} ", f"scene {c.name}@product ")
               for c in CC.CASES]
    return {d["label"]: d for d in map(parse, run_harness(harness, script))}


def test_the_table_has_every_case():
    assert len(CC.CASES) == len(CC.TABLE) == 59
    assert (len(CC.FUZZ), len(CC.MESH), len(CC.WALK)) == (20, 30, 9)
    assert sorted(c.name for c in CC.CASES if not c.cull_on) == ["fuzz_room2_0", "fuzz_room2_1"]
    assert sorted(c.name for c in CC.CASES if not c.tri_fast) == sorted(
        ["mesh_overflow_0", "mesh_overflow_1", "over_none", "over_back", "needle"])


@pytest.mark.parametrize("case", CC.CASES, ids=lambda c: c.name)
def test_cull_decision(packed, case):
    labels = [case.name] + ([case.name + "@t"] if case.family == "mesh" else [])
    for label in labels:
        got = packed[label]
        assert (int(got["cull_on"]), int(got["tri_fast"])) == (int(case.cull_on), int(case.tri_fast)), label
        if not case.cull_on:   # a scene without a mesh has no cull section at all
            assert got["cull_T"] == "" and got["n"][9] == "0", label


def test_needle_lights_are_never_culled(packed):
    """`needle`'s mesh is 2^90 away: every light's T = 4 R + 1 is at least 2^60 and stored as 0 (rtx_pack.cpp,
    cull_tmax), so no shadow lane passes `mag <= cull_T`.  The meshes scaled by 1e19 (overflow_*) are the only
    other cases beyond 2^60; every other culled case has a positive T for every light."""
    words = packed["needle"]["cull_T"].split(",")
    assert len(words) == 2 and set(words) == {"00000000"}
    zero = [c.name for c in CC.CASES if c.cull_on and "00000000" in packed[c.name]["cull_T"].split(",")]
    assert sorted(zero) == sorted(CC.ZERO_T)


def test_the_product_ratio_culls_few_of_them(packed):
    """Why the device tests force the ratio to 0: under the product's SAH ratio only these 17 cases cull."""
    on = sorted(c.name for c in CC.CASES if packed[c.name + "@product"]["cull_on"] == "1")
    want = (["fuzz_room3_0", "fuzz_room4_0", "fuzz_room4_1", "fuzz_nonfinite_0"] +
            [f"mesh_negative_{s}" for s in range(5)] + ["mesh_negative_x_0", "mesh_negative_x_1", "mesh_flat_grid_0"] +
            [f"mesh_caps_{s}" for s in range(4)] + ["mesh_mixed_0"])
    assert on == sorted(want)


def test_the_bound_scenes_cull_and_stay_tri_fast(harness, tmp_path):
    """tests/cull_domains.py's scenes: a vertex coordinate at 2^40 and one float above leaves tri_fast on (legs of
    2^27: |e1||e2| = 2^54.5, (|v0|_1 + 2^40)(|e1|_1 + |e2|_1) < 2^71), so the culled walks run on them; and the
    straddle scene's wall stands where its docstring says."""
    names = [*CD.COORD, CD.BT]
    script = [f"scene {n} file:{CD.write(n, tmp_path)} {tmp_path / n} min_sa=0" for n in names]
    got = {d["label"]: d for d in map(parse, run_harness(harness, script))}
    for n in names:
        assert (got[n]["cull_on"], got[n]["tri_fast"]) == ("1", "1"), n
        assert all(int(w, 16) != 0 for w in got[n]["cull_T"].split(",")), n
    assert 45.0 < CD.bt_bound() < 45.1
