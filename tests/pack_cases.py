"""The scenes whose packed image is pinned (tests/golden/pack_pins.json) — TEST INFRASTRUCTURE of
tests/test_pack_cpu.py (the packer on the CPU, tests/pack_harness.cpp) and
tests/test_gpu_upload_image.py (the upload on the device).

A case is a label, the scene's name for the harness (a catalogue scene, file:PATH, chain:T, lights:N)
and its options.  `harness_line` gives the harness command; `device_image` uploads the same scene
with the same options through the C-ABI and returns what the pins hold.  The pins were recorded with
`device_image` from the library of the commit before the packer existed."""
from __future__ import annotations

import ctypes as C
import hashlib
import os
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

import mesh_fuzz
import scene_fuzz

ROOT = Path(__file__).resolve().parents[1]
ASSETS = ROOT / "gp1_raytracer_2223_amd" / "assets"
PINS = ROOT / "tests" / "golden" / "pack_pins.json"
SECTIONS = ("spheres", "sphere_mat", "planes", "tris", "nodes", "meshes", "lights", "materials", "parts", "cull_rng",
            "cull_T")

CATALOGUE = ("W1", "W2", "W3", "W3_Test", "W4_Reference", "W4_Bunny", "W4_Optional", "Synthetic100k",
             "Bunny8Lights")
W4 = ("W4_Reference", "W4_Bunny", "W4_Optional")   # (W4_Test cannot be built: the reference never allocates its nodes)
UPDATE_T = 1.3
MESH_FUZZ = (("tiny", 0), ("tiny", 2), ("negative", 0), ("dup", 0), ("caps", 1))   # T = 1, 3; ...; 3,137 triangles
# option -> the context knob that sets it on the device
KNOBS = {"parts": "RTX_SPLIT_PARTS", "nocull": "RTX_NO_CULL", "no_octant": "RTX_NO_OCTANT", "room_skip_off": "RTX_ROOM_SKIP",
         "refine": "RTX_PART_REFINE"}


@dataclass(frozen=True)
class Case:
    label: str
    name: str                       # catalogue name, chain:T, lights:N, or "" for a scene file
    text: str = ""                  # the scene file's text
    objs: dict = field(default_factory=dict)   # stem -> OBJ text beside it
    opts: tuple = ()                # (key, value) pairs of the harness command


def cases() -> list[Case]:
    out = [Case(n, n) for n in CATALOGUE]
    out += [Case(f"{n}@t", n, opts=(("t", repr(UPDATE_T)),)) for n in W4]
    out += [Case(p.stem, "", text=p.read_text()) for p in sorted((ROOT / "scenes").glob("*.rtxscene"))]
    out += [Case(f"fuzz_{f}", "", text=scene_fuzz.make(f, scene_fuzz_seed(f)).text) for f in scene_fuzz.FAMILIES]
    for fam, seed in MESH_FUZZ:
        mc = mesh_fuzz.make(fam, seed)
        out.append(Case(f"mesh_{mc.name}", "", text=mc.text, objs=dict(mc.objs)))
    out += [Case("chain_70", "chain:71"), Case("chain_1030", "chain:1031"), Case("lights_32", "lights:32"),
            Case("lights_33", "lights:33")]
    opt = "W4_Optional"
    out += [Case("opt_parts8", opt, opts=(("parts", "8"),)), Case("opt_nocull", opt, opts=(("nocull", "1"),)),
            Case("opt_no_octant", opt, opts=(("no_octant", "1"),)), Case("opt_room_skip_off", opt, opts=(("room_skip_off", "1"),)),
            Case("opt_refine", opt, opts=(("refine", "0,1"),)), Case("opt_reserve", opt, opts=(("reserve", "1"),)),
            Case("opt_uploads3", opt, opts=(("uploads", "3"),))]
    return out


def scene_fuzz_seed(family: str) -> int:
    """The first committed seed of a scene_fuzz family."""
    return min(s for f, s in scene_fuzz.COMMITTED if f == family)


def materialise(case: Case, folder: Path) -> tuple[str, Path]:
    """The name and asset folder of a case for rtx_host_scene_create (scene files are written to `folder`)."""
    if case.name:
        return case.name, ASSETS
    d = folder / case.label
    d.mkdir(parents=True, exist_ok=True)
    for stem, text in case.objs.items():
        (d / f"{stem}.obj").write_text(text)
    path = d / f"{case.label}.rtxscene"
    path.write_text(case.text)
    return f"file:{path}", (d if case.objs else ASSETS)


def harness_line(case: Case, folder: Path) -> str:
    name, assets = materialise(case, folder)
    return " ".join([f"scene {case.label} {name} {assets}"] + [f"{k}={v}" for k, v in case.opts])


def fnv(buf) -> str:
    """64-bit FNV-1a of the bytes, as the harness prints it (sequential by definition: ~0.1 s per MB)."""
    h, p, m = 0xcbf29ce484222325, 0x100000001b3, 0xFFFFFFFFFFFFFFFF
    for b in bytes(buf):
        h = ((h ^ b) * p) & m
    return f"{h:016x}"


def sha256(buf) -> str:
    """Of the bytes: the pins hold it beside the FNV for the images too large to hash in Python in a test."""
    return hashlib.sha256(bytes(buf)).hexdigest()


def max_edge_product(scene) -> float:
    """max |e1| |e2| over the triangles of an rtx_scene, NaN if any triangle's is NaN (DevScene::tri_fast is
    1 when this is <= 2^56): the edges v1 - v0, v2 - v0 in binary32 as the triangle records hold them,
    their lengths and the product in double.  numpy throughout; no shortcut."""
    worst = 0.0
    for i in range(scene.n_meshes):
        m = scene.meshes[i]
        if m.n_indices < 3:
            continue
        pos = np.ctypeslib.as_array(m.positions, shape=(m.n_positions * 3,)).reshape(-1, 3)
        idx = np.ctypeslib.as_array(m.indices, shape=(m.n_indices,)).reshape(-1, 3)
        with np.errstate(all="ignore"):
            e1 = (pos[idx[:, 1]] - pos[idx[:, 0]]).astype(np.float64)
            e2 = (pos[idx[:, 2]] - pos[idx[:, 0]]).astype(np.float64)
            ee = np.sqrt((e1 * e1).sum(axis=1)) * np.sqrt((e2 * e2).sum(axis=1))
        if np.isnan(ee).any():
            return float("nan")
        worst = max(worst, float(ee.max()))
    return worst


def many_lights(n: int):
    from gp1_raytracer_2223_amd import abi
    lights = (abi.Light * n)()
    for i in range(n):
        lights[i].origin[:] = [-2.0 + 0.125 * i, 5.0, -3.0 + 0.0625 * i]
        lights[i].color[:] = [1.0, 0.5 + i / 64.0, 0.25]
        lights[i].intensity = 2.0 + i
        lights[i].type = abi.RTX_LIGHT_POINT
    return lights


def host_scene(case: Case, folder: Path):
    """(HostScene, rtx_scene, whatever the scene's pointers refer to) of a case, before any option."""
    from gp1_raytracer_2223_amd.scene import HostScene
    name, assets = materialise(case, folder)
    hand = name.split(":")[0] in ("chain", "lights")
    hs = HostScene("W4_Bunny" if hand else name, asset_dir=str(assets))
    opts = dict(case.opts)
    if "t" in opts:
        hs.update(float(opts["t"]))
    s, _ = hs.view()
    keep = None
    if name.startswith("chain:"):
        from test_gpu_deep_bvh import deep_scene
        s, _, keep = deep_scene(int(name[6:]))
    elif name.startswith("lights:"):
        keep = many_lights(int(name[7:]))
        s.lights, s.n_lights = keep, len(keep)
    return hs, s, keep


def read_image(ctx) -> np.ndarray:
    from gp1_raytracer_2223_amd import abi
    n = C.c_size_t(0)
    abi.check(ctx.lib.rtx_scene_image(ctx.h, None, 0, C.byref(n)), "rtx_scene_image")
    buf = np.zeros(n.value, np.uint8)
    abi.check(ctx.lib.rtx_scene_image(ctx.h, buf.ctypes.data, n.value, C.byref(n)), "rtx_scene_image")
    return buf


def context_facts(ctx) -> dict:
    nb = C.c_uint64(0)
    ctx.lib.rtx_scene_bytes(ctx.h, C.byref(nb))
    room_fact, room_m = ctx.room_info()
    return {"total": int(nb.value), "spec": int(ctx.spec_info()[0]), "room_fact": int(room_fact),
            "room_M": f"{np.float32(room_m).view(np.uint32):08x}", "parts": int(ctx.split_info()[1]),
            "cull_on": int(ctx.cull_info()[0])}


def device_image(case: Case, folder: Path):
    """Upload the case on a fresh context with its options set through the context's knobs; returns the
    image (uint8 array) and the facts the C-ABI reports."""
    from gp1_raytracer_2223_amd.renderer import DeviceAnimation, DeviceContext
    opts = dict(case.opts)
    env = {KNOBS[k]: ("0" if k == "room_skip_off" else v) for k, v in opts.items() if k in KNOBS}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        ctx = DeviceContext(int(os.environ.get("RTX_TEST_DEVICE", "0")))
        hs, s, keep = host_scene(case, folder)
        anim = None
        if "reserve" in opts:
            anim = DeviceAnimation(hs, ctx)
        else:
            for _ in range(int(opts.get("uploads", 1))):
                ctx.upload(s)
        img, facts = read_image(ctx), context_facts(ctx)
        if anim is not None:
            anim.close()
        ctx.close()
        del keep
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    return img, facts
