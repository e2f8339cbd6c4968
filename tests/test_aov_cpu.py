"""The hit-record planes (include/rtx.h, rtx_aov_planes) on the CPU: the ABI additions, the checker
of tests/aov_ref.py against its committed goldens, and a pin of the checker to the reference-pinned
renderer that uses none of the checker's own C."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import abi_surface
import aov_ref
import oracle_bind
import scene_fuzz
from checkers import checker  # noqa: F401
from gp1_raytracer_2223_amd import abi
from gp1_raytracer_2223_amd.scene import HostScene

ROOT = Path(__file__).resolve().parents[1]
G = ROOT / "tests" / "golden" / "aov"
W, H = aov_ref.GOLDEN_W, aov_ref.GOLDEN_H
CASES = aov_ref.golden_cases()
IDS = [f"{f}_{s}" for f, s in CASES]


def test_header_declares_and_abi_binds_the_aov_symbols(tmp_path):
    """The header's struct, constants and macros as the C compiler sees them equal the ctypes mirror,
    every new entry point is declared in its header, exported and bound, and the ABI version stays 2."""
    names = ["RTX_AOV_DEPTH", "RTX_AOV_NORMAL", "RTX_AOV_MATERIAL", "RTX_AOV_PRIMITIVE", "RTX_AOV_ALL"]
    fields = ["depth", "normal", "material", "primitive"]
    prints = ['printf("size %zu\\n", sizeof(rtx_aov_planes));', 'printf("version %d\\n", RTX_ABI_VERSION);']
    prints += [f'printf("{f} %zu\\n", offsetof(rtx_aov_planes, {f}));' for f in fields]
    prints += [f'printf("{n} %d\\n", (int){n});' for n in names]
    prints += ['printf("kind %u\\n", RTX_PRIM_KIND(0xC0000005u));', 'printf("index %u\\n", RTX_PRIM_INDEX(0xC0000005u));']
    planes = "int (*)(rtx_ctx*, const rtx_aov_planes*)"
    out = abi_surface.declared_exported_and_bound(tmp_path, {   # the prototypes, used as the issue states them
        "rtx_render_aov_async": "int (*)(rtx_ctx*, const rtx_camera*, int, const rtx_render_params*, uint32_t)",
        "rtx_render_aov": "int (*)(rtx_ctx*, const rtx_camera*, const rtx_render_params*, uint32_t, const rtx_aov_planes*)",
        "rtx_download_aov": planes,
        "rtx_gather_aov_async": planes,
        "rtx_device_aov_buffers": "int (*)(rtx_ctx*, rtx_aov_planes*)",
        "rtx_group_render_aov":
            "int (*)(rtx_group*, const rtx_camera*, const rtx_render_params*, uint32_t, const rtx_aov_planes*)",
    }, {"rtx_time_aov_frames": "int (*)(rtx_ctx*, const rtx_camera*, const rtx_render_params*, uint32_t, int, float*)"},
        statements=prints)
    c = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    assert c["version"] == 2 and abi.load_hip().rtx_abi_version() == 2
    assert c["size"] == C.sizeof(abi.AovPlanes)
    assert [n for n, _ in abi.AovPlanes._fields_] == fields
    for f in fields:
        assert c[f] == getattr(abi.AovPlanes, f).offset, f
    for n in names:
        assert c[n] == getattr(abi, n), n
    assert (c["RTX_AOV_DEPTH"], c["RTX_AOV_NORMAL"], c["RTX_AOV_MATERIAL"], c["RTX_AOV_PRIMITIVE"],
            c["RTX_AOV_ALL"]) == (1, 2, 4, 8, 15)
    assert c["kind"] == 3 == abi.prim_kind(0xC0000005) and c["index"] == 5 == abi.prim_index(0xC0000005)
    assert (abi.RTX_PRIM_SPHERE, abi.RTX_PRIM_PLANE, abi.RTX_PRIM_TRIANGLE) == (1, 2, 3)
    assert abi.load_hip().rtx_render_aov.argtypes[4]._type_ is abi.AovPlanes


def test_goldens_exist_for_every_case():
    assert set(scene_fuzz.COMMITTED) <= set(CASES)
    assert sorted(p.stem for p in G.glob("*.npz")) == sorted(IDS)
    assert sorted(p.stem for p in (ROOT / "tests" / "golden" / "fuzz").glob("*.rtxscene")) == \
        sorted(f"{f}_{s}" for f, s in scene_fuzz.COMMITTED)


@pytest.mark.parametrize("family,seed", CASES, ids=IDS)
def test_checker_regenerates_the_goldens(checker, tmp_path, family, seed):
    keep, s, cam = aov_ref.golden_view(family, seed, tmp_path)
    got = aov_ref.planes(checker, s, cam, W, H)
    g = np.load(G / f"{family}_{seed}.npz")
    assert sorted(g.files) == sorted(aov_ref.NAMES)
    for k in aov_ref.NAMES:
        assert g[k].dtype == got[k].dtype and g[k].shape == got[k].shape, k
        assert np.array_equal(g[k].view(np.uint32), got[k].view(np.uint32)), k   # same machine: NaN bits too
    # the contract's miss values, and ids inside the scene
    miss = got["primitive"] == 0
    assert (got["depth"][miss] == aov_ref.FLT_MAX).all() and (got["material"][miss] == 0).all()
    assert (got["normal"].reshape(-1, 3)[miss].view(np.uint32) == 0).all()
    kind, idx = aov_ref.kind(got["primitive"]), aov_ref.index(got["primitive"])
    n_tri = sum(s.meshes[i].n_indices // 3 for i in range(s.n_meshes))
    for k, n in ((1, s.n_spheres), (2, s.n_planes), (3, n_tri)):
        assert (idx[kind == k] < n).all(), k
    assert (got["material"] < s.n_materials).all()
    del keep


def test_every_kind_occurs_across_the_goldens():
    seen = np.zeros(4, np.int64)
    for name in IDS:
        seen += np.bincount(aov_ref.kind(np.load(G / f"{name}.npz")["primitive"]), minlength=4)
    assert (seen > 0).all(), seen


def _prims_of_line(fs, s, line):
    """The primitive words of the directive at `line` of a fuzz scene's text: spheres, planes and
    meshes are numbered in the order of their lines, a mesh's triangles follow the earlier meshes'."""
    rows = fs.text.split("\n")
    word = rows[line].split()[0]
    nth = sum(1 for r in rows[:line] if r.split()[:1] == [word])
    if word == "sphere":
        return {(1 << 30) | nth}
    if word == "plane":
        return {(2 << 30) | nth}
    assert word == "mesh"
    tri0 = sum(s.meshes[i].n_indices // 3 for i in range(nth))
    return {(3 << 30) | (tri0 + k) for k in range(s.meshes[nth].n_indices // 3)}


@pytest.mark.parametrize("family,seed", [c for c in scene_fuzz.COMMITTED if c[0] == "ties"])
def test_tied_primitives_win_pixels(tmp_path, family, seed):
    fs = scene_fuzz.make(family, seed)
    assert len(fs.tied) == 3
    keep, s, _ = aov_ref.golden_view(family, seed, tmp_path)
    won = set(np.load(G / f"{fs.name}.npz")["primitive"].tolist())
    for line in fs.tied:
        assert won & _prims_of_line(fs, s, line), f"line {line} ({fs.text.splitlines()[line]!r}) wins no pixel"
    del keep


# ---- the independent pin: materials as ids through the reference-pinned renderer ------------------
PIN_SCENES = ["W1", "W2", "W3", "W4_Reference"]


def _id_materials(s: abi.Scene):
    """The scene with material i replaced by SOLID_COLOR ((i + 1) / 64, 0, 0)."""
    mats = (abi.Material * s.n_materials)()
    for i in range(s.n_materials):
        mats[i].kind = abi.RTX_MAT_SOLID_COLOR
        mats[i].color[0] = (i + 1) / 64.0
    t = abi.Scene()
    C.memmove(C.byref(t), C.byref(s), C.sizeof(abi.Scene))
    t.materials = mats
    return t, mats


def test_material_and_hit_planes_equal_the_oracles_id_frame(checker):
    """BRDF mode without shadows adds the hit's material colour once per light and nothing else, so
    with the id materials the red channel is L (i + 1) / 64 for L lights (exact in binary32 while
    L n_materials <= 64: every partial sum is a multiple of 1/64 up to 1, and MaxToOne leaves it) and
    0 on a miss.  A scene without lights decodes nothing (every pixel is 0), so the condition here is
    1 <= L and L n_materials <= 64: W1 (no light) drops out, the other three stay."""
    Wp, Hp = 64, 48
    kept = []
    for name in PIN_SCENES:
        hs = HostScene(name)
        s, cam = hs.view()
        L, n = s.n_lights, s.n_materials
        if not (L >= 1 and L * n <= 64):
            continue
        kept.append(name)
        t, mats = _id_materials(s)
        _, rgb = oracle_bind.render(t, cam, abi.make_params(Wp, Hp, abi.RTX_MODE_BRDF, False))
        red = rgb.reshape(-1, 3)[:, 0]
        assert (rgb.reshape(-1, 3)[:, 1:] == 0).all()
        code = red * np.float32(64) / np.float32(L)        # exact: (i + 1), a small integer
        assert (code == np.round(code)).all() and (code >= 0).all() and (code <= n).all(), name
        hit = code > 0
        p = aov_ref.planes(checker, s, cam, Wp, Hp)
        assert np.array_equal(p["primitive"] != 0, hit), name
        assert np.array_equal(p["material"][hit], (code[hit] - 1).astype(np.uint32)), name
        assert (p["material"][~hit] == 0).all(), name
        del mats
    assert len(kept) >= 3, kept
