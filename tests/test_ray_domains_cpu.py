"""The conditions that keep tests/test_gpu_ray_domains.py honest, on the CPU: tests/ray_domains.py's rays
and cameras, recomputed in binary32 in the reference's operation order, really lie where their class says
(the squared length zero, a denormal, just below and exactly 2^-96, at and above 2^120; the smallest
component before and after the normalisation at 2^-60 and one float below), every class is present, the
inside waves are wholly inside, the outside waves wholly outside, and each mixed wave is inside but for its
one lane.  A case set that misses a class fails here, not silently on the GPU."""
import numpy as np
import pytest

import ray_domains as RD
import shade_ref
from checkers import checker  # noqa: F401
from gp1_raytracer_2223_amd import abi

F32 = np.float32
P2 = RD.P2


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    return tmp_path_factory.mktemp("rd_scenes")


def _facts(scene):
    rays, names = RD.waves(scene)
    l, t = RD.shadow_l(scene, rays)
    return rays, names, l, t, RD.domain_facts(l)


@pytest.mark.parametrize("scene", RD.SCENES)
def test_every_ray_hits_the_plane_and_starts_its_shadow_ray_where_it_says(checker, folder, scene):
    """t = 0.0001f, the shadow origin (x0, y0, 0) exactly, l = (-x0, -y0, Lz); and the checker agrees that
    every ray hits (its HIT flag): the light loop runs in every lane."""
    rays, names, l, t, _ = _facts(scene)
    assert rays.shape[0] % 64 == 0 and rays.shape[0] <= 1024
    assert (t == F32(0.0001)).all()
    assert np.array_equal(l[:, 0], -rays[:, 0]) and np.array_equal(l[:, 1], -rays[:, 1])
    assert (l[:, 2] == RD.LZ[scene]).all()
    hs, s, _ = RD.host_scene(scene, folder)
    _, _, flags = shade_ref.shade(checker, s, rays, shade_ref.params(abi.RTX_MODE_COMBINED, True))
    assert (flags & shade_ref.HIT).all()
    del hs


def test_every_class_is_populated_and_is_what_its_name_says():
    seen = {}
    for scene in RD.SCENES:
        _, names, l, _, f = _facts(scene)
        for c in np.unique(names):
            m = names == c
            seen[c] = int(m.sum())
            assert (f["inside"][m] == RD.CLASSES[c][2]).all(), c
            s, lo, dlo = f["s"][m], f["lo"][m], f["dlo"][m]
            if c == "s_at_2m96":
                assert (s == P2(-96)).all() and f["l_ok"][m].all() and f["d_ok"][m].all()
            elif c == "s_below_2m96":   # the test on s alone puts it outside
                assert ((s < P2(-96)) & (s >= P2(-97))).all() and f["l_ok"][m].all() and f["d_ok"][m].all()
            elif c == "l_below_2m60":   # ... the test on the components alone
                assert (lo == RD.dn(P2(-60))).all() and f["s_ok"][m].all() and f["d_ok"][m].all()
            elif c == "low_in":
                assert (lo == P2(-60)).all()   # the smallest |l_k| sits AT the bound in every inside ray
            elif c in ("s_at_2p120", "s_at_2p120_in"):
                assert (s == P2(120)).all() and f["s_ok"][m].all() and f["l_ok"][m].all() and not f["d_ok"][m].any()
            elif c == "s_above_2p120":
                assert (s > P2(120)).all() and np.isfinite(s).all()
            elif c == "s_2p124":
                assert (s >= P2(124)).all()
            elif c == "d_at_2m60":
                assert (dlo == P2(-60)).all() and f["s_ok"][m].all() and f["l_ok"][m].all()
            elif c == "d_below_2m60":   # ... the test on the normalised components alone
                assert (dlo == RD.dn(P2(-60))).all() and f["s_ok"][m].all() and f["l_ok"][m].all()
            elif c == "s_denormal":
                assert ((s > 0) & (s < np.finfo(np.float32).tiny)).all()
            elif c == "s_zero_vector":
                assert (s == 0).all() and (l[m] == 0).all()
            elif c == "s_zero_underflow":
                assert (s == 0).all() and (l[m][:, 0:2] != 0).all()
            elif c == "light_far":
                assert (s >= P2(120)).all() and (np.abs(l[m][:, 2]) > P2(60)).all()
    assert sorted(seen) == sorted(RD.CLASSES), set(RD.CLASSES) - set(seen)
    assert all(n >= 3 for n in seen.values()), seen


@pytest.mark.parametrize("scene", RD.SCENES)
def test_waves_are_inside_outside_and_mixed_as_laid_out(scene):
    _, names, _, _, f = _facts(scene)
    ins = f["inside"].reshape(-1, 64)
    if scene not in RD.INSIDE_OF:
        assert not ins.any()          # wholly outside, wave after wave
        return
    assert ins.shape[0] == len(RD.LAYOUT)
    assert ins[0].all() and not ins[1].any()
    assert len(set(names[64:128])) == len(RD.OUTSIDE_OF[scene])   # the outside wave shows every outside class
    for j, lane in enumerate(RD.MIXED_LANES):
        w = ins[2 + j]
        assert not w[lane] and w.sum() == 63, (scene, lane)


@pytest.mark.parametrize("name,W,H", [("plain", 8, 8), ("plain", 16, 8), ("thin8", 8, 8), ("thin16", 16, 8),
                                      ("small", 8, 8), ("huge", 16, 8)])
def test_cameras_put_the_primary_direction_where_they_say(name, W, H):
    cam, all_in, some_in = RD.cameras()[name]
    f = RD.domain_facts(RD.primary_l(cam, W, H))
    for lanes in RD.wave_lanes(W, H):
        w = f["inside"][lanes]
        assert w.all() == all_in and w.any() == some_in, (name, int(w.sum()))
        if name.startswith("thin"):   # outside by the component tests alone: whole columns beside the centre
            assert f["s_ok"][lanes].all()         # (and where |d| shrinks the next column's d_x below the bound)
            cols = (~f["l_ok"][lanes]).reshape(8, 8)
            assert (cols == cols[0]).all() and 0 < cols[0].sum() < 8
            assert not w[~f["l_ok"][lanes]].any() and 8 <= w.sum() <= 64 - 8 * cols[0].sum()
    if name == "small":
        assert (f["s"] < P2(-96)).all() and (f["s"] > 0).all()
    if name == "huge":
        assert (f["s"] > P2(120)).all()
