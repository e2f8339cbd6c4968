"""The ray kernels and the frame path at the edges of every fast-path domain (*Fast-path
domains* (1)-(5)): tests/walk_domains.py's rays exactly at each operand bound and one float past it, on
scenes whose triangles sit exactly at the |e1||e2| = 2^56 bound of `tri_fast` and one float past it, in
waves wholly inside a domain, wholly outside, and inside but for one lane.  Every output word equals the
CPU checkers' (a NaN float equals any NaN); nothing is measured, the tolerance is zero.
tests/test_walk_domains_cpu.py proves on the CPU that these sets hit, are occluded and not, and take each
walk; without it a comparison here could be vacuous."""
import os

import numpy as np
import pytest
import torch   # noqa: F401  (at collection, before librtx_hip.so is loaded)

import aov_ref
import oracle_bind
import rayq_ref
import relight_ref
import shade_ref
import walk_domains as WD
from checkers import checker  # noqa: F401
from gp1_raytracer_2223_amd import abi
from gp1_raytracer_2223_amd.renderer import AOV_ALL, DeviceContext
from gpu_support import DEV
from gpu_support import ctx  # noqa: F401
from test_gpu_adaptive import _compose, _oracle_ps, _same
from test_gpu_rayq import _check

pytestmark = pytest.mark.gpu

FW, FH = 64, 48
MODES = (abi.RTX_MODE_OBSERVED_AREA, abi.RTX_MODE_COMBINED)


@pytest.fixture(scope="module")
def generic_ctx():
    os.environ["RTX_NO_SPEC"] = "1"   # read once, at context creation
    try:
        c = DeviceContext(DEV)
    finally:
        del os.environ["RTX_NO_SPEC"]
    yield c
    c.close()


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    return tmp_path_factory.mktemp("wd_scenes")


_scenes = {}


def _scene(folder, name, cull):
    """`needle`: its frame variant (walk_domains.needle_texts)."""
    if (name, cull) not in _scenes:
        _scenes[(name, cull)] = (WD.needle_scene(cull, folder, True) if name == "needle" else
                                 WD.host_scene(WD.GEO[name], cull, folder))
    return _scenes[(name, cull)][1:]


# ---- queries ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,cull", WD.SCENES)
def test_queries(ctx, checker, folder, name, cull):
    """trace_rays and occluded on every class's waves and tail set, whole and on the prefixes 1, 63, 64
    and 65, against the checker: the four planes and the occlusion bytes, word for word."""
    s, _ = _scene(folder, name, cull)
    ctx.upload(s)
    for key, rays in WD.all_sets(WD.GEO[name]).items():
        assert 65 < rays.shape[0] <= 2048
        _check(ctx, rays, rayq_ref.trace(checker, s, rays), rayq_ref.occluded(checker, s, rays), f"{name}/{cull}/{key}")


@pytest.mark.parametrize("cull", WD.CULLS)
def test_queries_on_thin_triangles_far_away(ctx, checker, folder, cull):
    """`needle`: |e1||e2| = 2^56 exactly, but `(o - v0) x e1` overflows for every origin.  Rays inside
    every ray domain must still get the reference's answer (a NaN t that DoesHit accepts): the scene is
    not tri_fast.  Queries and shaded rays."""
    hs, s, _ = WD.needle_scene(cull, folder)
    ctx.upload(s)
    rays = WD.needle_rays()
    _check(ctx, rays, rayq_ref.trace(checker, s, rays), rayq_ref.occluded(checker, s, rays), f"needle/{cull}")
    p = shade_ref.params(abi.RTX_MODE_COMBINED, True)
    wpx, wrgb, _ = shade_ref.shade(checker, s, rays, p)
    gpx, grgb = ctx.shade_rays(rays, p)
    assert shade_ref.same(gpx, grgb, wpx, wrgb), f"needle/{cull}: shaded rays differ"
    del hs


# ---- shaded rays --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cull", WD.CULLS)
@pytest.mark.parametrize("cls", ["onto_plane", "far", "omax"])
def test_shaded_rays(ctx, checker, folder, cull, cls):
    """shade_rays in ObservedArea and Combined with shadows, on `giant`: hit points (the shadow rays'
    origins) on either side of 2^40 on the far plane, with the light beyond the mesh; the NaN-occluder
    class; and primary origins at the 2^40 bound.  Pixel and rgb words against shade_ref."""
    s, _ = _scene(folder, "giant", cull)
    ctx.upload(s)
    geo = WD.GEO["giant"]
    for key, rays in ((f"{cls}/waves", WD.waves(geo, cls)), (f"{cls}/tail", WD.tail(geo, cls))):
        for mode in MODES:
            p = shade_ref.params(mode, True)
            wpx, wrgb, _ = shade_ref.shade(checker, s, rays, p)
            for n in (rays.shape[0], 1, 63, 64, 65):
                gpx, grgb = ctx.shade_rays(rays[:n], p)
                assert shade_ref.same(gpx, grgb, wpx[:n], wrgb[:3 * n]), \
                    f"giant/{cull}/{key} mode {mode} n = {n}: pixels {np.nonzero(gpx != wpx[:n])[0][:8].tolist()} differ"


# ---- adaptive -----------------------------------------------------------------------------------------------

def test_adaptive(ctx, folder):
    """render_adaptive with k = 2 on `giant` from its camera 2^20 before a triangle, every pixel refined
    that differs from a neighbour (threshold 0): the composition of the oracle's plain and supersampled frames."""
    s, cam = _scene(folder, "giant", "none")
    W, H = 37, 23
    P, S = _oracle_ps(("wd_giant_none", -1.0), s, cam, W, H, 2)
    wpx, wrgb, E = _compose(P, S, W, H, 0)
    assert 0 < E.sum()
    ctx.upload(s)
    got = ctx.render_adaptive(cam, abi.make_params(W, H), 2, 0)
    assert ctx.adaptive_refined() == int(E.sum())
    _same(got, (wpx, wrgb), "giant, k = 2, threshold 0, against the oracle")


# ---- the frame path at the tri_fast bound -------------------------------------------------------------------

_want = {}


def _frame_refs(checker, folder, name, cull):
    """The oracle's colour frames of both modes, the checker's hit-pass planes and its shadow plane: once."""
    if (name, cull) not in _want:
        s, cam = _scene(folder, name, cull)
        frames = {m: oracle_bind.render(s, cam, abi.make_params(FW, FH, m, 1)) for m in MODES}
        planes = aov_ref.planes(checker, s, cam, FW, FH)
        bits, hit = relight_ref.plane(checker, s, cam, FW, FH)
        for a in [bits, *planes.values()] + [x for f in frames.values() for x in f]:
            a.setflags(write=False)
        _want[(name, cull)] = (frames, planes, bits)
    return _want[(name, cull)]


def _words(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("generic", [False, True], ids=["spec", "no_spec"])
@pytest.mark.parametrize("name,cull", [("giant", "none"), ("giant", "back"), ("over", "none"), ("sliver", "none"),
                                       ("needle", "none"), ("needle", "back")])
def test_frames(ctx, generic_ctx, checker, folder, name, cull, generic):
    """The 64 x 48 colour frame in both modes, the hit pass, the shadow pass and the relight of `giant`
    (tri_fast at its bound), `over` (one float past it), `sliver` and `needle` (a quarter of whose shadow
    words are the NaN-accepting triangle's: the frame path's exact walk takes Vector3::Cross as written),
    on the default context and on an RTX_NO_SPEC=1 one, against the oracle and the CPU references."""
    c = generic_ctx if generic else ctx
    s, cam = _scene(folder, name, cull)
    frames, planes, bits = _frame_refs(checker, folder, name, cull)
    c.upload(s)
    for m in MODES:
        gpx, grgb = c.render(cam, abi.make_params(FW, FH, m, 1))
        assert np.array_equal(gpx, frames[m][0]), f"{name}/{cull} mode {m}: {(gpx != frames[m][0]).sum()} pixels differ"
        assert _words(grgb, frames[m][1]), f"{name}/{cull} mode {m}: colour words differ"
    got = c.render_aov(cam, abi.make_params(FW, FH), AOV_ALL)
    bad = aov_ref.diff(got, planes)
    assert not bad, f"{name}/{cull}: hit pass planes {bad} differ"
    c.render_shadows_async()
    gbits = c.download_shadows()
    assert np.array_equal(gbits, bits), f"{name}/{cull}: {(gbits != bits).sum()} shadow words differ"
    for m in MODES:
        gpx, grgb = c.relight(abi.make_params(1, 1, m, 1))
        assert np.array_equal(gpx, frames[m][0]), f"{name}/{cull} mode {m}: the relight's pixels differ"
        assert _words(grgb, frames[m][1]), f"{name}/{cull} mode {m}: the relight's colour words differ"
