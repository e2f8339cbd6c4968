"""The edits of the in-place scene-edit tests (tests/test_edit_cpu.py on the packer functions through
tests/edit_harness.cpp, tests/test_gpu_edit.py on the device) — TEST INFRASTRUCTURE.

Records are abi.Light / abi.Material; `step_lights` / `step_materials` write them as a harness step (binary32
bit patterns in hex).  The moves: MOVE_IN stays inside the five-plane room of the catalogue's room scenes
(x in (-5, 5), y in (0, 10), z < 10) one unit from two planes, nearer than any catalogue light, so the room-skip
record changes with it; MOVE_OUT lies beyond the plane x = 5, so the room-skip fact turns false."""
from __future__ import annotations

import ctypes as C

import numpy as np

from gp1_raytracer_2223_amd import abi

MOVE_IN = (4.0, 1.0, 3.0)
MOVE_OUT = (8.0, 5.0, -5.0)
N_MANY = 256          # the material limit of a scene
SEED = 20240611       # random_material_values: checked for its denormals and huge values by the CPU test


def f32hex(x) -> str:
    return f"{int(np.float32(x).view(np.uint32)):08x}"


def copy_light(l: abi.Light) -> abi.Light:
    out = abi.Light()
    C.memmove(C.byref(out), C.byref(l), C.sizeof(abi.Light))
    return out


def copy_material(m: abi.Material) -> abi.Material:
    out = abi.Material()
    C.memmove(C.byref(out), C.byref(m), C.sizeof(abi.Material))
    return out


def lights_of(scene) -> list:
    return [copy_light(scene.lights[i]) for i in range(scene.n_lights)]


def materials_of(scene) -> list:
    return [copy_material(scene.materials[i]) for i in range(scene.n_materials)]


def recolour(l: abi.Light, index: int, round_: int = 0) -> abi.Light:
    """Light `index` with another colour and intensity (exact binary32 values), its origin kept."""
    out = copy_light(l)
    out.color[:] = [0.25 + 0.125 * ((index + round_) % 5), 0.875 - 0.25 * (index % 3), 0.5 + 0.0625 * round_]
    out.intensity = 33.0 + 7.0 * index + round_
    return out


def moved(l: abi.Light, origin) -> abi.Light:
    out = copy_light(l)
    out.origin[:] = list(origin)
    return out


def revalue(m: abi.Material, index: int, round_: int = 0) -> abi.Material:
    """Material `index` with other values (its kind kept): every field changes."""
    out = copy_material(m)
    out.color[:] = [0.125 + 0.0625 * ((index + round_) % 11), 0.9375 - 0.0625 * (index % 7), 0.375 + 0.03125 * (index % 13)]
    out.kd = 0.5 + 0.03125 * ((index + round_) % 9)
    out.ks = 0.25 + 0.0625 * (index % 5)
    out.exponent = 10.0 + index % 50 + round_
    out.metalness = float((index + round_) % 2)
    out.roughness = 0.125 + 0.0625 * ((index + round_) % 12)
    return out


def many_materials(scene) -> C.Array:
    """`scene`'s materials, then Lambert ones up to N_MANY whose values follow from their index
    (tests/edit_harness.cpp's mats256: the same values, all exact in binary32 but for the divisions, which are
    computed in binary32 here as there)."""
    arr = (abi.Material * N_MANY)()
    for i in range(N_MANY):
        if i < scene.n_materials:
            C.memmove(C.byref(arr[i]), C.byref(scene.materials[i]), C.sizeof(abi.Material))
            continue
        f = np.float32
        arr[i].kind = abi.RTX_MAT_LAMBERT
        arr[i].color[:] = [float(f(0.25) + f(i) / f(512)), float(f(1) - f(i) / f(300)), 0.5]
        arr[i].kd = float(f(0.5) + f(i) / f(1024))
        arr[i].ks, arr[i].exponent, arr[i].metalness, arr[i].roughness = 0.25, 8.0 + i, 0.0, 0.5
    return arr


def step_lights(first: int, lights, types: bool = False) -> str:
    return f"L{first}:" + ";".join(
        ",".join([f32hex(v) for v in (*l.origin, *l.color, l.intensity)] + ([str(int(l.type))] if types else []))
        for l in lights)


def step_materials(first: int, materials, kinds: bool = False) -> str:
    return f"M{first}:" + ";".join(
        ",".join([f32hex(v) for v in (*m.color, m.kd, m.ks, m.exponent, m.metalness, m.roughness)]
                 + ([str(int(m.kind))] if kinds else []))
        for m in materials)


def random_material_values(seed: int = SEED, rounds: int = 16, n: int = N_MANY) -> np.ndarray:
    """(rounds, n, 8) float32 of seeded random BIT PATTERNS, the non-finite ones dropped: denormals, huge and tiny
    magnitudes of both signs; and both zeros, which a random pattern does not hit, at fixed places."""
    rng = np.random.default_rng(seed)
    need = rounds * n * 8
    bits = rng.integers(0, 1 << 32, size=2 * need + 64, dtype=np.uint64).astype(np.uint32)
    bits = bits[(bits & 0x7F800000) != 0x7F800000][:need]
    assert bits.size == need
    bits = bits.reshape(rounds, n, 8).copy()
    bits[:, 3, 0], bits[:, 3, 3] = 0x00000000, 0x80000000      # +0 colour, -0 kd
    bits[:, 5, 1], bits[:, 5, 3] = 0x80000000, 0x00000000
    return bits.view(np.float32)


def value_materials(template, values: np.ndarray) -> C.Array:
    """abi.Material records with `values` (n, 8: color[3], kd, ks, exponent, metalness, roughness) and the kinds of
    `template` (a sequence of abi.Material of at least that length)."""
    arr = (abi.Material * len(values))()
    for i, v in enumerate(values):
        arr[i].kind = template[i].kind
        arr[i].color[:] = [float(v[0]), float(v[1]), float(v[2])]
        arr[i].kd, arr[i].ks, arr[i].exponent, arr[i].metalness, arr[i].roughness = (float(x) for x in v[3:])
    return arr
