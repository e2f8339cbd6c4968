"""The adversarial cases the exact cull is tested on, and what the packer decides for each — TEST
INFRASTRUCTURE (tests/test_cull_cases_cpu.py, tests/test_gpu_cull_fuzz.py).

The 59 cases are the committed sets of tests/scene_fuzz.py (20) and tests/mesh_fuzz.py (30), the scenes of
tests/walk_domains.py (8) and its `needle` scene in the frame variant.  TABLE holds, per case, the packer's
verdict under RTX_CULL_MIN_SA=0 (the harness's min_sa=0): `cull_on`, whether the scene renders with the
exact cull at all, and `tri_fast`, without which no wave takes the walks that test the records (pcull and
scull of the render kernel need a FAST batch).  tests/test_cull_cases_cpu.py holds the packer to the
table on the CPU, so the device tests' "the cull ran" is an expectation derived without the device.

cull_on is 0 for the two scenes without a mesh and 1 for every other one: with a ratio of 0 the worth
test always passes, every committed tree is left-then-right ordered and every mesh box is finite (1e19
and 2^90 included).  tri_fast is 0 where |e1||e2| exceeds 2^56 (mesh overflow_*, over_*) and on `needle`,
whose (|v0|_1 + 2^40)(|e1|_1 + |e2|_1) exceeds 2^126; needle's lights all get cull_T = 0 besides (its
mesh is 2^90 away: T = 4 R + 1 >= 2^60 is never culled)."""
from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path

import mesh_fuzz
import scene_fuzz
import walk_domains as WD

ASSETS = Path(__file__).resolve().parents[1] / "gp1_raytracer_2223_amd" / "assets"

NO_MESH = ("fuzz_room2_0", "fuzz_room2_1")
NOT_TRI_FAST = ("mesh_overflow_0", "mesh_overflow_1", "over_none", "over_back", "needle")
# every light's cull_T is 0 (the mesh box reaches beyond 2^60 / 4 from it): no shadow ray is culled
ZERO_T = ("mesh_overflow_0", "mesh_overflow_1", "needle")


@dataclass(frozen=True)
class CullCase:
    name: str
    family: str         # "fuzz", "mesh", "walk" or "needle"
    key: tuple          # the family module's own key
    cull_on: bool       # the packer's verdict with min_sa = 0
    tri_fast: bool


def _case(name, family, key):
    return CullCase(name, family, key, name not in NO_MESH, name not in NOT_TRI_FAST)


CASES = ([_case(f"fuzz_{f}_{s}", "fuzz", (f, s)) for f, s in scene_fuzz.COMMITTED] +
         [_case(f"mesh_{f}_{s}", "mesh", (f, s)) for f, s in mesh_fuzz.COMMITTED] +
         [_case(f"{g}_{c}", "walk", (g, c)) for g, c in WD.SCENES] +
         [_case("needle", "needle", ("none",))])
TABLE = {c.name: c for c in CASES}
FUZZ = [c for c in CASES if c.family == "fuzz"]
MESH = [c for c in CASES if c.family == "mesh"]
WALK = [c for c in CASES if c.family in ("walk", "needle")]


def write(case: CullCase, folder) -> tuple[Path, Path]:
    """Write the case's scene file (and OBJ files) below `folder`: (scene file, asset folder)."""
    d = Path(folder) / case.name
    d.mkdir(parents=True, exist_ok=True)
    if case.family == "fuzz":
        path = d / f"{case.name}.rtxscene"
        path.write_text(scene_fuzz.make(*case.key).text)
        return path, ASSETS
    if case.family == "mesh":
        return mesh_fuzz.make(*case.key).write(d), d
    if case.family == "walk":
        path = WD.write_scene(WD.GEO[case.key[0]], case.key[1], d)
    else:
        path = WD.write_needle(case.key[0], d, True)
    return path, path.parent


def harness_line(case: CullCase, folder, *opts) -> str:
    path, assets = write(case, folder)
    return " ".join([f"scene {case.name} file:{path} {assets}", "min_sa=0", *opts])


def host_scene(case: CullCase, folder):
    """The case's HostScene in its initial state (keep it alive while its view is in use)."""
    from gp1_raytracer_2223_amd.scene import HostScene
    path, assets = write(case, folder)
    return HostScene(f"file:{path}", asset_dir=str(assets))
