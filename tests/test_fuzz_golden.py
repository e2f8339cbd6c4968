"""Pin the oracle to the reference on the seeded adversarial scenes of tests/scene_fuzz.py
(tests/golden/fuzz/, written by `make_goldens.py --fuzz-only`): kd != 1, Phong exponents 0 and
200, roughness 0, metalness 0.5, non-unit plane normals, mirrored and front- / no-cull meshes,
ties between primitive kinds, and frames that contain NaN and inf.  The GPU tests
(tests/test_gpu_fuzz.py) compare the device with the oracle on these scenes and further seeds; this
module is what makes the oracle the authority there, and it checks that the committed set covers
what it claims."""
from pathlib import Path

import numpy as np
import pytest

import oracle_bind
import scene_fuzz
from gp1_raytracer_2223_amd import abi
from gp1_raytracer_2223_amd.scene import HostScene

G = Path(__file__).resolve().parent / "golden" / "fuzz"
W, H = 44, 28
FRAMES = [(3, 1), (2, 0)]
IDS = [f"{f}_{s}" for f, s in scene_fuzz.COMMITTED]


def _view(name):
    hs = HostScene(f"file:{G / (name + '.rtxscene')}")
    return hs.view()


_counts = {}


def _count(name):
    """The oracle's work counters of the (3,1) frame (computed once per scene)."""
    if name not in _counts:
        s, cam = _view(name)
        c = oracle_bind.count(s, cam, abi.make_params(W, H, 3, 1))
        _counts[name] = dict(zip(oracle_bind.COUNTER_NAMES, (int(x) for x in c)))
    return _counts[name]


def test_committed_set_is_the_generators():
    """Exactly the files of scene_fuzz.COMMITTED: two seeds of every family, four of open and nonfinite."""
    assert sorted(p.stem for p in G.glob("*.rtxscene")) == sorted(IDS)
    assert sorted(p.stem for p in G.glob("*.npz")) == sorted(IDS)
    per_family = {f: sum(1 for g, _ in scene_fuzz.COMMITTED if g == f) for f in scene_fuzz.FAMILIES}
    assert per_family == {f: 4 if f in ("open", "nonfinite") else 2 for f in scene_fuzz.FAMILIES}


@pytest.mark.parametrize("family,seed", scene_fuzz.COMMITTED, ids=IDS)
def test_generator_regenerates_the_committed_text(family, seed):
    fs = scene_fuzz.make(family, seed)
    assert (G / f"{fs.name}.rtxscene").read_bytes() == fs.text.encode()
    assert scene_fuzz.make(family, seed, camera=True).text == fs.text


@pytest.mark.parametrize("name", IDS)
@pytest.mark.parametrize("mode,sh", FRAMES)
def test_oracle_equals_the_reference(name, mode, sh):
    """Both planes as uint32 words: NaN payloads and the q8(NaN) = 0 pixels included."""
    g = np.load(G / f"{name}.npz")
    s, cam = _view(name)
    px, rgb = oracle_bind.render(s, cam, abi.make_params(W, H, mode, sh))
    gpx, grgb = g[f"pixels_m{mode}s{sh}"], g[f"rgb_m{mode}s{sh}"]
    assert px.shape == gpx.shape and rgb.shape == grgb.shape
    assert np.array_equal(px, gpx), f"{(px != gpx).sum()} pixels differ"
    bad = rgb.view(np.uint32) != grgb.view(np.uint32)
    assert not bad.any(), f"{bad.sum()} colour words differ, first at {np.argmax(bad)}"


@pytest.mark.parametrize("name", IDS)
def test_every_scene_is_hit(name):
    c = _count(name)
    assert c["pixels"] == W * H
    assert c["hit"] * 5 >= c["pixels"], c


def test_the_set_shades_every_kind_and_occludes():
    total = {k: sum(_count(n)[k] for n in IDS) for k in ("shade_lambert", "shade_phong", "shade_ct", "occluded")}
    assert all(v > 0 for v in total.values()), total


def test_room_families_shade_cook_torrance_where_they_claim():
    for name in IDS:
        if name.startswith("room0"):
            assert _count(name)["shade_ct"] == 0 and _count(name)["shade_phong"] == 0, name
        elif name.startswith("room"):
            assert _count(name)["shade_ct"] > 0 and _count(name)["shade_phong"] == 0, name


@pytest.mark.parametrize("name", [n for n in IDS if n.startswith("nonfinite")])
@pytest.mark.parametrize("mode,sh", FRAMES)
def test_nonfinite_frames_hold_nan_and_finite_values(name, mode, sh):
    rgb = np.load(G / f"{name}.npz")[f"rgb_m{mode}s{sh}"]
    assert np.isnan(rgb).mean() >= 0.003, np.isnan(rgb).mean()
    assert np.isfinite(rgb).mean() >= 0.5, np.isfinite(rgb).mean()


@pytest.mark.parametrize("family,seed", [c for c in scene_fuzz.COMMITTED if c[0] == "ties"],
                         ids=[n for n in IDS if n.startswith("ties")])
def test_tied_primitives_win_pixels(tmp_path, family, seed):
    """Removing a tied primitive (the quad in the floor plane, the tangent sphere, the first of the two
    identical spheres) changes the closest hit of at least one pixel: BRDF mode without shadows, where
    a pixel depends on nothing but its own closest hit."""
    fs = scene_fuzz.make(family, seed)
    assert len(fs.tied) == 3
    p = abi.make_params(W, H, 2, 0)
    s, cam = _view(fs.name)
    base, _ = oracle_bind.render(s, cam, p, want_rgb=False)
    assert np.array_equal(base, np.load(G / f"{fs.name}.npz")["pixels_m2s0"])
    for line in fs.tied:
        f = tmp_path / f"without_{line}.rtxscene"
        f.write_text(fs.without(line))
        s2, cam2 = HostScene(f"file:{f}").view()
        px, _ = oracle_bind.render(s2, cam2, p, want_rgb=False)
        assert (px != base).any(), f"line {line} ({fs.text.splitlines()[line]!r}) wins no pixel"
