"""Ray queries (include/rtx.h: rtx_trace_rays, rtx_occluded) on the CPU: the ABI additions, the ray
sets' own conditions (so that no GPU test of them is vacuous), the checker of tests/rayq_ref.py against
the hit pass's checker, and its committed goldens."""
import ctypes as C

import numpy as np
import pytest

import abi_surface
import aov_ref
import gpu_support as gs
import rayq_rays
import rayq_ref
from checkers import checker  # noqa: F401
from gp1_raytracer_2223_amd import abi

W, H = 37, 23
SEED = 7


def test_header_declares_and_abi_binds_the_query_symbols(tmp_path):
    """rtx_ray as the C compiler sees it equals the ctypes mirror (32 bytes), the four entry points are
    declared as the issue states them, exported and bound, and the ABI version stays 2."""
    fields = ["origin", "direction", "tmin", "tmax"]
    prints = ['printf("size %zu\\n", sizeof(rtx_ray));', 'printf("version %d\\n", RTX_ABI_VERSION);']
    prints += [f'printf("{f} %zu\\n", offsetof(rtx_ray, {f}));' for f in fields]
    trace = "int (*)(rtx_ctx*, const rtx_ray*, uint32_t, uint32_t, const rtx_aov_planes*)"
    occluded = "int (*)(rtx_ctx*, const rtx_ray*, uint32_t, uint8_t*)"
    out = abi_surface.declared_exported_and_bound(tmp_path, {
        "rtx_trace_rays": trace, "rtx_occluded": occluded, "rtx_trace_rays_device": trace, "rtx_occluded_device": occluded,
    }, {}, statements=prints)
    c = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    assert c["version"] == 2 and abi.load_hip().rtx_abi_version() == 2
    assert c["size"] == 32 == C.sizeof(abi.Ray)
    assert [n for n, _ in abi.Ray._fields_] == fields
    for f in fields:
        assert c[f] == getattr(abi.Ray, f).offset, f
    lib = abi.load_hip()
    assert lib.rtx_trace_rays.argtypes[1]._type_ is abi.Ray and lib.rtx_trace_rays.argtypes[4]._type_ is abi.AovPlanes


def test_the_cpp_mirror_compiles(tmp_path):
    abi_surface.cpp_mirror_compiles(tmp_path, [
        ("rtx::Renderer::AovFrame (rtx::Renderer::*)(const std::vector<rtx_ray>&, uint32_t)", "TraceRays"),
        ("std::vector<uint8_t> (rtx::Renderer::*)(const std::vector<rtx_ray>&)", "Occluded")])


def _shares(planes):
    kind = aov_ref.kind(planes["primitive"])
    n = float(kind.size)
    return {k: (kind == k).sum() / n for k in range(4)}


def test_ray_sets_shapes_and_recipes():
    s, _ = gs.view("W4_Bunny")
    for r in (rayq_rays.scatter(SEED), rayq_rays.aimed(s, SEED), rayq_rays.octant(s, SEED),
              rayq_rays.nonfinite(s, SEED)):
        assert r.dtype == np.float32 and r.ndim == 2 and r.shape[1] == 8 and 65 < r.shape[0] <= 2048
    sc = rayq_rays.scatter(SEED)
    length = np.linalg.norm(sc[:, 3:6].astype(np.float64), axis=1)
    for v in (1e-3, 0.5, 1, 3, 1e3):
        assert (np.abs(length / v - 1) < 1e-5).any(), v
    assert set(sc[:, 6].tolist()) == {np.float32(1e-4), 0.0, -1.0, 0.5}
    assert set(sc[:, 7].tolist()) == {float(rayq_rays.FLT_MAX), float("inf"), 2.0, 6.0}
    oc = rayq_rays.octant(s, SEED).reshape(10, 64, 8)
    for k in range(8):   # block k: one sign per axis, octant k; every component inside rcp3_exact's domain
        neg = oc[k, :, 3:6] < 0
        assert (neg == [bool((k >> a) & 1) for a in range(3)]).all(), k
        assert (np.abs(oc[k, :, 3:6]) >= 1e-3).all()
    assert len({tuple(r) for r in (oc[8, :, 3:6] < 0).tolist()}) > 1
    axis = oc[9, :, 3:6] == 0
    assert axis.any(axis=1).sum() == 1 and np.signbit(oc[9, 17, 3]) and not np.signbit(oc[9, 17, 4])
    nf = rayq_rays.nonfinite(s, SEED)[0::4]
    for f in range(8):
        col = nf[3 * f:3 * f + 3, f]
        assert np.isnan(col[0]) and col[1] == np.inf and col[2] == -np.inf, f
    assert (nf[24, 3:6] == 0).all() and nf[25, 7] < nf[25, 6]
    lo, hi = rayq_rays.mesh_box(s)
    assert nf[26, 0] == lo[0] and nf[28, 0] == hi[0] and nf[26, 3] == 0 and nf[30, 1] == lo[1]
    t = rayq_rays.wave_tiles(16, 8)
    assert sorted(t.tolist()) == list(range(128)) and t[:9].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 16] and t[64] == 8


def test_floors_aimed_bunny(checker):
    s, _ = gs.view("W4_Bunny")
    rays = rayq_rays.aimed(s, SEED)
    p = rayq_ref.trace(checker, s, rays)
    sh = _shares(p)
    tri = aov_ref.kind(p["primitive"]) == 3
    assert sh[3] >= 0.25 and sh[2] >= 0.10 and sh[0] >= 0.10, sh
    assert np.unique(p["primitive"][tri]).size >= 100
    occ = rayq_ref.occluded(checker, s, rays).mean()
    assert 0.10 <= occ <= 0.90, occ


def test_floors_aimed_optional(checker):
    s, _ = gs.view("W4_Optional")
    sh = _shares(rayq_ref.trace(checker, s, rayq_rays.aimed(s, SEED)))
    assert sh[3] >= 0.25 and sh[0] >= 0.05, sh


def test_floors_scatter(checker):
    s, _ = gs.view("W1")
    rays = rayq_rays.scatter(SEED)
    sh = _shares(rayq_ref.trace(checker, s, rays))
    assert sh[1] >= 0.03 and sh[2] >= 0.25 and sh[0] >= 0.25, sh
    occ = rayq_ref.occluded(checker, s, rays).mean()
    assert 0.10 <= occ <= 0.90, occ


@pytest.mark.parametrize("name", ["W4_Bunny", "W4_Reference"])
def test_floors_shadow(checker, name):
    s, cam = gs.view(name)
    rays, pixel = rayq_ref.shadow(checker, s, cam, W, H, 0)
    assert rays.shape[0] == pixel.size > 64 and (np.diff(pixel.astype(np.int64)) > 0).all()
    occ = rayq_ref.occluded(checker, s, rays).mean()
    assert 0.10 <= occ <= 0.90, (name, occ)


@pytest.mark.parametrize("name", ["W1", "W3", "W4_Reference", "W4_Bunny"])
def test_primary_rays_give_the_hit_pass_planes(checker, name):
    """The checker on its own primary rays equals aov_ref.c's frame, word for word."""
    s, cam = gs.view(name)
    got = rayq_ref.trace(checker, s, rayq_ref.primary(checker, cam, W, H))
    want = aov_ref.planes(checker, s, cam, W, H)
    for k in aov_ref.NAMES:
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (name, k)


def test_goldens_exist_for_every_case():
    assert sorted(p.stem for p in rayq_ref.GOLDEN.glob("*.npz")) == sorted(rayq_ref.GOLDEN_CASES)
    assert {"W1", "W4_Bunny", "open_12", "ties_0", "nonfinite_0"} <= set(rayq_ref.GOLDEN_CASES)


@pytest.mark.parametrize("case", rayq_ref.GOLDEN_CASES)
def test_checker_regenerates_the_goldens(checker, tmp_path, case):
    keep, s, _ = rayq_ref.golden_view(case, tmp_path)
    g = np.load(rayq_ref.GOLDEN / f"{case}.npz")
    assert sorted(g.files) == sorted(aov_ref.NAMES + ("rays", "occluded"))
    rays = g["rays"]
    assert rays.dtype == np.float32 and rays.shape[1] == 8 and rays.shape[0] <= 2048
    assert np.array_equal(rays.view(np.uint32), rayq_ref.golden_rays(s).view(np.uint32))
    got = rayq_ref.trace(checker, s, rays)
    for k in aov_ref.NAMES:
        assert g[k].dtype == got[k].dtype and np.array_equal(g[k].view(np.uint32), got[k].view(np.uint32)), k
    occ = rayq_ref.occluded(checker, s, rays)
    assert g["occluded"].dtype == np.uint8 and np.array_equal(g["occluded"], occ)
    assert 0.10 <= occ.mean() <= 0.90, occ.mean()
    # the contract's miss values
    miss = got["primitive"] == 0
    assert miss.any() and (got["depth"][miss] == aov_ref.FLT_MAX).all() and (got["material"][miss] == 0).all()
    assert (got["normal"].reshape(-1, 3)[miss].view(np.uint32) == 0).all()
    del keep
