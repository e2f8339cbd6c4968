"""What tests/test_gpu_deep_stack_fill.py relies on, asserted on the reference alone: the left-deep
chains of tests/deep_chain.py fill the per-wave DFS stack to the tree's level depth (the chain of
tests/test_gpu_deep_bvh.py never holds more than one entry), their rim rays hit the triangle they were
made for, the model's slab test and primary rays are the oracle's bit for bit, and the packer gives the
chains the depth, the stack variant and the split verdict the device tests assume."""
from __future__ import annotations

import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import aov_ref
import deep_chain as dc
import oracle_bind
import rayq_ref
from checkers import checker  # noqa: F401
from gp1_raytracer_2223_amd import abi

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "gp1_raytracer_2223_amd" / "csrc"
LIB = ROOT / "gp1_raytracer_2223_amd" / "lib"
SIZES = (64, 65, 300, 1024, 1025)   # depth 63 of 64 entries; 64: the deep stack; 1023 of 1024; 1024: the HBM stacks
CASES = [(T, layout) for T in SIZES for layout in dc.LAYOUTS]


# ---------------------------------------------------------------- the model is the oracle's arithmetic

def test_the_models_slab_test_is_the_oracles():
    """Every (ray, box) pair of both 65-triangle chains' nodes under primary rays of a central and a border
    tile, rim rays, the axis ray (two infinite inverses) and rays whose origin lies on a box face with a zero
    direction component there (0 * inf)."""
    lib = oracle_bind.lib()
    pairs = 0
    for layout in dc.LAYOUTS:
        s, cam = dc.view(65, layout)
        lo, hi, *_ = dc.node_arrays(s.meshes[0])
        p = abi.make_params(dc.W, dc.H)
        rays = np.concatenate([dc.camera_tile_rays(cam, p, 110)[::9], dc.camera_tile_rays(cam, p, 45)[::13],
                               dc.rim_rays(s, cam)[0][:12], dc.axis_waves(s, cam)[[0, 70]]])
        on_face = dc.axis_ray(cam).repeat(4, axis=0)
        on_face[0, 0], on_face[1, 0] = lo[0, 0], hi[0, 0]                 # x on the root's faces, dx = +0
        on_face[2, 1], on_face[2, 4] = lo[0, 1], np.float32(-0.0)         # y on a face, dy = -0
        on_face[3, 2], on_face[3, 5] = lo[3, 2], np.float32(0.0)          # z in a leaf's plane, dz = 0
        on_face[3, 3] = np.float32(0.25)
        rays = np.concatenate([rays, on_face])
        got = dc.slab_pass(rays, lo, hi)
        for i, r in enumerate(rays):
            for b in range(len(lo)):
                box = np.concatenate([lo[b], hi[b]]).astype(np.float32)
                want = lib.rtx_oracle_slab(oracle_bind.fptr(np.ascontiguousarray(r)), oracle_bind.fptr(box))
                assert bool(want) == bool(got[i, b]), (layout, i, b)
                pairs += 1
        assert got.any() and not got.all()
    assert pairs >= 300


@pytest.mark.parametrize("w,h,fov", [(dc.W, dc.H, dc.FOV), (37, 23, None)])
def test_the_models_primary_rays_are_the_oracles(checker, w, h, fov):
    _, cam = dc.view(65, "centred")
    c = abi.Camera.from_buffer_copy(cam)
    if fov is None:
        c.fov = float(np.tan(np.radians(45.0) / 2))
    want = rayq_ref.primary(checker, c, w, h).reshape(h, w, 8)
    p = abi.make_params(w, h)
    cols = -(-w // 8)
    for tile in range(cols * -(-h // 8)):
        x0, y0 = 8 * (tile % cols), 8 * (tile // cols)
        block = want[y0:y0 + 8, x0:x0 + 8].reshape(-1, 8)
        got = dc.camera_tile_rays(c, p, tile)
        assert got.shape == block.shape and np.array_equal(got.view(np.uint32), block.view(np.uint32)), tile


# ---------------------------------------------------------------- how full the stack gets

@pytest.mark.parametrize("T", [300, 1100])
def test_the_existing_chain_never_holds_more_than_one_entry(T):
    """The gap: test_gpu_deep_bvh.chain_mesh has the leaf on the left, so a walk pushes the rest of the
    chain, tests the leaf and pops again, in every tile of the 320 x 180 frames its tests render."""
    from test_gpu_deep_bvh import deep_scene
    s, cam, keep = deep_scene(T)
    hw = dc.frame_high_water(s, cam, 320, 180)
    assert hw.size == 40 * 23 and hw.max() == 1, hw.max()
    del keep


@pytest.mark.parametrize("T,layout", CASES)
def test_the_left_deep_chain_fills_the_stack(T, layout):
    s, cam = dc.view(T, layout)
    hw = dc.frame_high_water(s, cam)
    full = np.nonzero(hw == T - 1)[0]
    print(f"T={T} {layout}: {full.size} of {hw.size} tiles reach {T - 1}: {full.tolist()}")
    assert hw.max() == T - 1 and full.size >= 8
    assert (np.diff(full) == 1).sum() >= 2, "no two full tiles follow each other in tile order"


@pytest.mark.parametrize("T", SIZES)
def test_an_any_hit_axis_wave_pops_the_whole_stack(T):
    """Corner layout: the axis crosses every box and misses every triangle, so each axis wave pushes T - 1
    entries and pops every one of them.  Centred layout: triangle 0 occludes the axis and the wave leaves
    from its first leaf, T - 1 entries still pending."""
    s, cam = dc.view(T, "corner")
    waves = dc.axis_waves(s, cam)
    assert waves.shape[0] == 130
    for first in (0, 64, 128):
        assert dc.high_water_any(s, waves[first:first + 64]) == (T - 1, max(0, T - 1 - 64), T - 1), first
    s, cam = dc.view(T, "centred")
    assert dc.high_water_any(s, dc.axis_waves(s, cam)[:64]) == (T - 1, 0, 0)


# ---------------------------------------------------------------- the ray sets

@pytest.mark.parametrize("T,layout", CASES)
def test_every_rim_ray_hits_its_triangle(checker, T, layout):
    s, cam = dc.view(T, layout)
    rays, tri = dc.rim_rays(s, cam)
    assert rays.shape[0] == T + -(-T // 63) and rays.shape[0] % 64 != 0
    assert (tri[0::64] == -1).all() and np.array_equal(tri[tri >= 0], np.arange(T))
    prim = rayq_ref.trace(checker, s, rays)["primitive"]
    rim = tri >= 0
    assert (aov_ref.kind(prim[rim]) == abi.RTX_PRIM_TRIANGLE).all()
    bad = np.nonzero(aov_ref.index(prim[rim]) != tri[rim])[0]
    assert bad.size == 0, f"rim rays of triangles {bad[:8].tolist()} hit {aov_ref.index(prim[rim])[bad[:8]].tolist()}"
    # the axis: triangle 0, or past every triangle to the room's back wall
    want = (abi.RTX_PRIM_TRIANGLE << 30) if layout == "centred" else None
    axis = prim[~rim]
    assert (axis == want).all() if want is not None else (aov_ref.kind(axis) == abi.RTX_PRIM_PLANE).all()
    # a full wave of them holds T - 1 entries: lane 0 alone passes every box
    assert dc.high_water(s, rays[:64]) == T - 1 and dc.high_water(s, rays[-(rays.shape[0] % 64):]) <= T - 1
    occ = rayq_ref.occluded(checker, s, dc.axis_waves(s, cam))
    assert (occ[[0, 63, 64, 128, 129]] == (1 if layout == "centred" else 0)).all() and occ[65:128].all()


# ---------------------------------------------------------------- the packer's facts

def build_pack(folder: Path) -> Path:
    """test_pack_cpu.build_harness's command line with tests/deep_chain_pack.cpp (pack_harness.cpp plus the
    `mesh` command) in pack_harness.cpp's place."""
    exe = folder / "deep_chain_pack"
    rocm = Path(os.environ.get("ROCM_PATH", "/opt/rocm"))
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                    f"-I{ROOT / 'include'}", f"-I{CSRC}", f"-isystem{rocm / 'include'}",
                    str(ROOT / "tests" / "deep_chain_pack.cpp"), str(CSRC / "rtx_pack.cpp"), "-o", str(exe),
                    f"-L{LIB}", "-lrtx_host", f"-Wl,-rpath,{LIB}"], check=True)
    return exe


def test_the_packer_gives_the_chains_their_depth_and_stack(tmp_path):
    import test_pack_cpu as tp
    exe = build_pack(tmp_path)
    script = []
    for T, layout in CASES:
        path = tmp_path / f"{layout}_{T}.mesh"
        dc.write_mesh(path, *dc.left_deep_mesh(T, layout))
        script.append(f"mesh {layout}_{T} {path} {tp.PC.ASSETS}")
        if T == 64:   # (the device test's RTX_SPLIT_PARTS=8)
            script.append(f"mesh {layout}_{T}_parts8 {path} {tp.PC.ASSETS} parts=8")
    got = {d["label"]: d for d in map(tp.parse, tp.run_harness(exe, script))}
    assert len(got) == len(CASES) + 2
    for T, layout in CASES:
        d = got[f"{layout}_{T}"]
        facts = (int(d["max_depth"]), int(d["deep"]), int(d["hbm"]))
        assert facts == (T - 1, int(T - 1 >= 64), int(T - 1 >= 1024)), (T, layout, facts)
        assert int(d["sig"].split("/")[3]) == T
        if T == 64:
            for e in (d, got[f"{layout}_{T}_parts8"]):
                assert e["split_ok"] == "1" and int(e["n_parts"]) > 1, (layout, e["split_ok"], e["n_parts"])
        else:   # (a deep stack renders unsplit)
            assert d["split_ok"] == "0", (T, layout)
