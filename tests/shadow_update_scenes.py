"""The file scenes of the incremental shadow pass's tests (tests/test_shadow_update_cpu.py,
tests/test_gpu_shadow_update.py) — TEST INFRASTRUCTURE.

Two geometries under one camera and three lights, and six variants of the lights.  `room` is the five-plane room
of tests/test_gpu_relight.py with the bunny; `open` has two planes that are no room, two spheres and the bunny, so
its shadow rays take the plane loop whose numerators the first traced light caches for the later ones."""
from __future__ import annotations

import numpy as np

from gp1_raytracer_2223_amd.scene import HostScene

CAMERA = "camera 0 3 -9 45"
MATS = ["material lambert 0.49 0.57 0.57 1", "material lambert 1 1 1 1", "material lambert 0.8 0.3 0.3 1",
        "material lambert 0.3 0.8 0.3 1"]   # (tests/test_gpu_relight.py's) + the default material 0: five
BUNNY = "mesh lowpoly_bunny2 2 back scale 2 2 2"
GEOMETRY = {
    "room": ["plane 0 0 10   0 0 -1  1", "plane 0 0 0    0 1 0   1", "plane 0 10 0   0 -1 0  1",
             "plane 5 0 0   -1 0 0   1", "plane -5 0 0   1 0 0   1", BUNNY],
    "open": ["plane 0 0 0  0 1 0  1", "plane 0 0 12  0.3 0 -1  2", "sphere -2.2 1 1  1  3", "sphere 2.4 1.2 2  1.2  4",
             BUNNY],
}
# intensity and colour of W4_Bunny's three lights
TAIL = ["50 1 0.61 0.45", "70 1 0.8 0.45", "50 0.34 0.47 0.68"]


def _point(l, xyz):
    return f"light point {xyz}  {TAIL[l]}"


BASE = [_point(0, "0 5 5"), _point(1, "-2.5 5 -5"), _point(2, "2.5 2.5 -5")]
# variant -> (its lights, the bits of the plane it may change)
VARIANTS = {
    "base": (BASE, 0),
    "move0": ([_point(0, "1.5 6 3"), BASE[1], BASE[2]], 0b001),
    "move1_out": ([BASE[0], _point(1, "8 5 -5"), BASE[2]], 0b010),
    "move12": ([BASE[0], _point(1, "-3.5 2 -3"), _point(2, "3 6 0")], 0b110),
    "type2": ([BASE[0], BASE[1], f"light directional 2.5 2.5 -5  {TAIL[2]}"], 0b100),
    "added": (BASE + ["light point 3 2 -3  40 0.6 0.8 1"], 0b1000),
    "removed": (BASE[:2], 0b100),
}


def file_scene(tmp_path, geometry: str, variant: str) -> HostScene:
    path = tmp_path / f"{geometry}_{variant}.rtxscene"
    path.write_text("\n".join([CAMERA, *MATS, *GEOMETRY[geometry], *VARIANTS[variant][0]]) + "\n")
    return HostScene(f"file:{path}")


def light_keys(scene) -> list:
    """Per light what its shadow rays depend on: the origin's and the type's bits (rtx.h)."""
    return [(np.array(list(scene.lights[l].origin), np.float32).tobytes(), int(scene.lights[l].type))
            for l in range(scene.n_lights)]


def dirty_mask(old_keys: list, new_keys: list) -> int:
    """The lights of `new_keys` whose key differs from the recorded one or that the record does not have."""
    return sum(1 << l for l, k in enumerate(new_keys) if l >= len(old_keys) or old_keys[l] != k)


def changed_per_bit(a: np.ndarray, b: np.ndarray, n_bits: int = 32) -> list:
    """How many words differ in bit l, for l < n_bits."""
    x = np.asarray(a, np.uint32) ^ np.asarray(b, np.uint32)
    return [int(((x >> np.uint32(l)) & np.uint32(1)).sum()) for l in range(n_bits)]
