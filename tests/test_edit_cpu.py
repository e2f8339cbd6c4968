"""The in-place edits' packer functions (csrc/rtx_pack.h: edit_inputs, pack_light_edit, pack_material_edit) on
the CPU: tests/edit_harness.cpp, compiled here with csrc/rtx_pack.cpp under the address and undefined-behaviour
sanitizers and run as a child process.  For each scene A and each edit, the harness packs the edited scene B
from scratch, applies the edit's byte ranges to A's emitted image and compares: the image byte for byte, and
the retained room_fact, room_M and spec with B's.  This file asserts that, and first that A's and B's images
differ in every section the edit is meant to touch: an edit that changes nothing proves nothing.

Also here, because the GPU test relies on them: the moves of tests/edit_cases.py flip the room-skip fact, and
its seeded material bit patterns hold a denormal, a magnitude above 2^100 and both zeros."""
from __future__ import annotations

import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import edit_cases as EC
from gp1_raytracer_2223_amd.scene import HostScene

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "gp1_raytracer_2223_amd" / "csrc"
LIB = ROOT / "gp1_raytracer_2223_amd" / "lib"
ASSETS = ROOT / "gp1_raytracer_2223_amd" / "assets"
# W4_Bunny (one mesh, Lambert, exact-cull inputs), W3 (no mesh: no cull bounds; Cook-Torrance) and a five-plane
# room from a scene file
SCENES = {"W4_Bunny": "W4_Bunny", "W3": "W3", "room_file": f"file:{ROOT / 'scenes' / 'w4_bunny.rtxscene'}"}
HAS_MESH = {"W4_Bunny": True, "W3": False, "room_file": True}
INVALID, UNSUPPORTED = -1, -5


def build_harness(folder: Path) -> Path:
    exe = folder / "edit_harness"
    rocm = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                    f"-I{ROOT / 'include'}", f"-I{CSRC}", f"-isystem{rocm / 'include'}",
                    str(ROOT / "tests" / "edit_harness.cpp"), str(CSRC / "rtx_pack.cpp"), "-o", str(exe),
                    f"-L{LIB}", "-lrtx_host", f"-Wl,-rpath,{LIB}"], check=True)
    return exe


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("edit"))


def run(exe: Path, label: str, name: str, steps: list[str], opts: str = "") -> list[dict]:
    line = f"edit {label} {name} {ASSETS} {opts} -- " + " ".join(steps)
    r = subprocess.run([str(exe)], input=line + "\n", capture_output=True, text=True,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0, r.stderr[-2000:]
    out = []
    for ln in r.stdout.splitlines():
        head, _, err = ln.partition(" err=")
        d = dict(x.split("=", 1) for x in head.split()[1:])
        d["err"] = err
        d["differ"] = set(filter(None, d["differ"].split(",")))
        out.append(d)
    assert len(out) == len(steps)
    return out


def good(d: dict) -> None:
    assert (d["rc"], d["equal"], d["facts"]) == ("0", "1", "1"), d


@pytest.fixture(scope="module")
def scenes():
    """label -> (its lights, its materials), copied out of the host scene."""
    out = {}
    for label, name in SCENES.items():
        s, _ = HostScene(name).view()
        out[label] = (EC.lights_of(s), EC.materials_of(s))
    return out


@pytest.mark.parametrize("label", sorted(SCENES))
def test_value_edits_of_lights(harness, scenes, label):
    lights, _ = scenes[label]
    every = [EC.recolour(l, i) for i, l in enumerate(lights)]
    tail = [EC.recolour(l, i, 3) for i, l in enumerate(lights)][1:]   # first > 0, n reaching the last record
    a, b = run(harness, label, SCENES[label], [EC.step_lights(0, every), EC.step_lights(1, tail)])
    for d in (a, b):
        good(d)
        assert d["differ"] == {"lights"} and (d["moved"], d["ranges"]) == ("0", "1")   # two float4 a light, nothing else
    assert int(a["words"]) == 8 * len(lights) and int(b["words"]) == 8 * (len(lights) - 1)


@pytest.mark.parametrize("label", sorted(SCENES))
def test_a_light_moved_within_the_room(harness, scenes, label):
    lights, _ = scenes[label]
    (d,) = run(harness, label, SCENES[label], [EC.step_lights(0, [EC.moved(lights[0], EC.MOVE_IN)])])
    good(d)
    assert d["differ"] == {"lights", "planes"} | ({"cull_T"} if HAS_MESH[label] else set())
    assert (d["room_fact"], d["moved"]) == ("1", "1") and int(d["ranges"]) == (3 if HAS_MESH[label] else 2)


@pytest.mark.parametrize("label", sorted(SCENES))
def test_a_light_moved_out_of_the_room_and_back(harness, scenes, label):
    """The fact flips both ways; the last light, so first > 0 and n reaches the last record."""
    lights, _ = scenes[label]
    k = len(lights) - 1
    steps = [EC.step_lights(k, [EC.moved(lights[k], EC.MOVE_OUT)]), EC.step_lights(k, [lights[k]])]
    out, back = run(harness, label, SCENES[label], steps)
    for d in (out, back):
        good(d)
        assert {"lights", "planes"} <= d["differ"] and d["moved"] == "1"
    assert (out["room_fact"], int(out["room_M"], 16)) == ("0", 0)
    assert back["room_fact"] == "1" and int(back["room_M"], 16) != 0
    # RTX_ROOM_SKIP=0: the fact stays false, the record empty
    off = run(harness, label, SCENES[label], steps, opts="room_skip_off=1")
    for d in off:
        good(d)
        assert d["room_fact"] == "0" and "planes" not in d["differ"]


@pytest.mark.parametrize("label", sorted(SCENES))
def test_moves_and_values_in_one_range(harness, scenes, label):
    lights, _ = scenes[label]
    recs = [EC.recolour(l, i) for i, l in enumerate(lights)][1:]
    recs[-1] = EC.moved(recs[-1], EC.MOVE_IN)
    (d,) = run(harness, label, SCENES[label], [EC.step_lights(1, recs)])
    good(d)
    assert {"lights", "planes"} <= d["differ"] and d["moved"] == "1"


@pytest.mark.parametrize("label", sorted(SCENES))
def test_material_edits(harness, scenes, label):
    _, mats = scenes[label]
    every = [EC.revalue(m, i) for i, m in enumerate(mats)]
    tail = [EC.revalue(m, i, 5) for i, m in enumerate(mats)][1:]
    a, b = run(harness, label, SCENES[label], [EC.step_materials(0, every), EC.step_materials(1, tail)])
    for d in (a, b):
        good(d)
        assert d["differ"] == {"materials"} and d["ranges"] == "1"
    assert int(a["words"]) == 12 * len(mats) and int(b["words"]) == 12 * (len(mats) - 1)


def test_all_256_materials(harness):
    s, _ = HostScene("W4_Bunny").view()
    mats = EC.many_materials(s)
    steps = [EC.step_materials(0, [EC.revalue(m, i) for i, m in enumerate(mats)])]
    values = EC.random_material_values()
    steps += [EC.step_materials(0, EC.value_materials(mats, values[r])) for r in (0, 15)]   # (every finite pattern)
    for d in run(harness, "mats256", "mats256:W4_Bunny", steps):
        good(d)
        assert d["differ"] == {"materials"} and int(d["words"]) == 12 * EC.N_MANY


def test_refusals_change_nothing(harness, scenes):
    lights, mats = scenes["W4_Bunny"]
    n, m = len(lights), len(mats)
    other_type = [EC.copy_light(l) for l in lights]
    other_type[-1].type = 1 - other_type[-1].type          # the LAST record of the range is the illegal one
    other_kind = [EC.revalue(x, i) for i, x in enumerate(mats)]
    other_kind[-1].kind = (other_kind[-1].kind + 1) % 4
    steps = [EC.step_lights(0, [EC.recolour(l, i) for i, l in enumerate(other_type)], types=True),
             EC.step_lights(1, [EC.recolour(l, i) for i, l in enumerate(lights)]),          # first + n = count + 1
             EC.step_lights(n + 1, [lights[0]]),
             EC.step_materials(0, other_kind, kinds=True),
             EC.step_materials(m, [mats[0]]),
             # ... and after them an edit of each kind still gives the edited scene's image: nothing was touched
             EC.step_lights(0, [EC.moved(EC.recolour(lights[0], 0), EC.MOVE_IN)]),
             EC.step_materials(0, [EC.revalue(mats[0], 0)])]
    out = run(harness, "refusals", "W4_Bunny", steps)
    assert [d["rc"] for d in out] == [str(c) for c in (UNSUPPORTED, INVALID, INVALID, UNSUPPORTED, INVALID, 0, 0)]
    assert f"light {n - 1} " in out[0]["err"] and f"material {m - 1} " in out[3]["err"]
    for d in out[:5]:
        assert (d["ranges"], d["words"]) == ("0", "0")
    good(out[5])
    good(out[6])


def test_the_material_bit_patterns_hold_what_they_are_for():
    v = EC.random_material_values()
    assert v.shape == (16, EC.N_MANY, 8) and np.isfinite(v).all()
    mag = np.abs(v.astype(np.float64))
    assert ((mag > 0) & (mag < 2.0 ** -126)).any(), "no denormal"
    assert (mag > 2.0 ** 100).any(), "no magnitude above 2^100"
    bits = v.view(np.uint32)
    assert (bits == 0).any() and (bits == 0x80000000).any(), "both zeros"
    with np.errstate(all="ignore"):   # ... and products that overflow, and that underflow to a denormal
        prod = v[:, :, :3] * v[:, :, 3:4]
    assert np.isinf(prod).any() and ((np.abs(prod) > 0) & (np.abs(prod) < np.float32(2.0 ** -126))).any()
