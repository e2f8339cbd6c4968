"""The host's two BVH builders on the adversarial meshes of tests/mesh_fuzz.py, pinned to the
reference (tests/golden/meshfuzz/, written by golden/make_mesh_goldens.py from the reference built
in place): after every prefix of a case's Update list the per-mesh digests equal the reference's,
and the oracle's frames of the host-updated scene equal the reference's own frames word for word.
The GPU tests (tests/test_gpu_anim_fuzz.py) compare the device builder with the host on these cases;
this module is what makes the host the authority there, and it asserts on the goldens that the
committed set reaches the corners it claims (a generator edit cannot quietly lose one).

Both builders are checked, each in its own process (the builder is chosen once per process): the
default fast one and the direct restatement (RTX_HOST_BVH=direct)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import mesh_fuzz

G = Path(__file__).resolve().parent / "golden" / "meshfuzz"
ROOT = G.parents[2]
W, H = 44, 28
FRAMES = [(3, 1), (0, 1)]
IDS = [f"{f}_{s}" for f, s in mesh_fuzz.COMMITTED]
STACK_DEPTH = 64    # kStackDepth (csrc/rtx_kernels.h): the render kernel's DFS stack
FRESH = [(f, 11) for f in mesh_fuzz.FAMILIES if f != "mixed"]    # seeds outside the goldens

_CHILD = r"""
import sys, json
sys.path[:0] = [sys.argv[1], sys.argv[1] + '/tests']
import numpy as np
import oracle_bind
from gp1_raytracer_2223_amd import abi
from gp1_raytracer_2223_amd.scene import HostScene
from test_host_sequence import _digest
scene, assets, times, frames, out = sys.argv[2], sys.argv[3], json.loads(sys.argv[4]), json.loads(sys.argv[5]), sys.argv[6]
hs = HostScene(scene, asset_dir=assets)
digests = []
for t in times:
    hs.update(t)
    digests.append([_digest(m) for m in hs.arrays()["meshes"]])
s, cam = hs.view()
planes = {}
for mode, sh in frames:
    px, rgb = oracle_bind.render(s, cam, abi.make_params(%d, %d, mode, sh))
    planes[f"pixels_m{mode}s{sh}"], planes[f"rgb_m{mode}s{sh}"] = px, rgb
np.savez(out, **planes)
print(json.dumps(digests))
""" % (W, H)


def _host_run(case, folder, builder, frames=FRAMES):
    """(digests per Update per mesh, frames after the list) of one builder, in its own process."""
    scene = case.write(folder)
    env = dict(os.environ)
    env.pop("RTX_HOST_BVH", None)
    if builder == "direct":
        env["RTX_HOST_BVH"] = "direct"
    out = folder / f"frames_{builder}.npz"
    r = subprocess.run([sys.executable, "-c", _CHILD, str(ROOT), f"file:{scene}", str(folder), json.dumps(case.times),
                        json.dumps(frames), str(out)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1]), np.load(out)


def _golden(name):
    return np.load(G / f"{name}.npz")


def test_committed_set_is_the_generators():
    assert sorted(p.stem for p in G.glob("*.npz")) == sorted(IDS)
    assert {f for f, _ in mesh_fuzz.COMMITTED} == set(mesh_fuzz.FAMILIES)
    for family, seed in mesh_fuzz.COMMITTED:
        case, g = mesh_fuzz.make(family, seed), _golden(f"{family}_{seed}")
        assert case.times[0] == float(np.float32(mesh_fuzz.FIRST_TIME)) and len(case.times) >= 4, case.name
        assert np.array_equal(np.array(case.times, np.float32), g["times"]), case.name
        # the spinning meshes first, in the generator's order (a static mesh after them)
        assert list(g["first_triangles"]) == list(case.triangles.values()), case.name


@pytest.mark.parametrize("builder", ["fast", "direct"])
@pytest.mark.parametrize("family,seed", mesh_fuzz.COMMITTED, ids=IDS)
def test_host_builders_match_reference(tmp_path, family, seed, builder):
    case = mesh_fuzz.make(family, seed)
    g = _golden(case.name)
    digests, frames = _host_run(case, tmp_path, builder)
    for k, got in enumerate(digests, 1):
        assert got == [str(x) for x in g[f"after{k}"]], f"after {k} updates"
    for mode, sh in FRAMES:
        px, rgb = frames[f"pixels_m{mode}s{sh}"], frames[f"rgb_m{mode}s{sh}"]
        gpx, grgb = g[f"pixels_m{mode}s{sh}"], g[f"rgb_m{mode}s{sh}"]
        assert np.array_equal(px, gpx), f"mode {mode}: {(px != gpx).sum()} pixels differ"
        assert np.array_equal(rgb.view(np.uint32), grgb.view(np.uint32)), f"mode {mode}: colour words differ"


@pytest.mark.parametrize("family,seed", FRESH, ids=[f"{f}_{s}" for f, s in FRESH])
def test_fresh_seed_builders_agree(tmp_path, family, seed):
    """A seed outside the goldens: the two host builders against each other."""
    assert (family, seed) not in mesh_fuzz.COMMITTED
    case = mesh_fuzz.make(family, seed)
    fast, _ = _host_run(case, tmp_path, "fast", [])
    direct, _ = _host_run(case, tmp_path, "direct", [])
    assert fast == direct


# ---- coverage conditions, on the reference's own trees
def _cases(family):
    return [(s, _golden(f"{f}_{s}")) for f, s in mesh_fuzz.COMMITTED if f == family]


def _leaves():
    """(name, largest leaf) of every committed single-mesh tree, first and last Update."""
    for f, s in mesh_fuzz.COMMITTED:
        g = _golden(f"{f}_{s}")
        for when in ("first", "last"):
            for leaf in g[f"{when}_leaf"]:
                yield f"{f}_{s}", int(leaf)


def test_tiny_counts_indices():
    """`idxCount <= 8` counts indices: two triangles never split, three do."""
    for seed, g in _cases("tiny"):
        T = int(g["first_triangles"][0])
        assert T == mesh_fuzz.TINY_T[seed]
        for when in ("first", "last"):
            nodes = int(g[f"{when}_nodes"][0])
            if T <= 2:
                assert nodes == 1
            elif T == 3:
                assert nodes == 3
            else:
                assert nodes >= 3
    assert sorted(int(g["first_triangles"][0]) for _, g in _cases("tiny")) == sorted(mesh_fuzz.TINY_T)


def test_dup_has_a_leaf_above_every_capacity_under_a_split_root():
    assert any(int(g["first_nodes"][0]) == 3 and int(g["first_leaf"][0]) > 4096 and
               int(g["last_nodes"][0]) == 3 and int(g["last_leaf"][0]) > 4096 for _, g in _cases("dup"))
    assert any(int(g["first_triangles"][0]) < 100 and int(g["first_leaf"][0]) >= 40 for _, g in _cases("dup"))


def test_negative_barely_splits():
    """All centroids negative: the FLT_MIN maximum.  One large case has a few nodes and a leaf of
    thousands, one is a root that stays the only leaf, above the device builder's LDS capacity."""
    big = [g for _, g in _cases("negative") if int(g["first_triangles"][0]) >= 3000]
    assert any(1 < int(g["first_nodes"][0]) <= 16 and int(g["first_leaf"][0]) > 2000 for g in big)
    assert any(int(g["first_nodes"][0]) == 1 and int(g["first_leaf"][0]) > 3136 for g in big)
    for seed, g in _cases("negative"):
        if seed != 4:
            assert int(g["first_nodes"][0]) <= 16 and int(g["last_nodes"][0]) <= 16
    # on one axis only, the other two axes still split
    for _, g in _cases("negative_x"):
        assert int(g["first_nodes"][0]) > int(g["first_triangles"][0])


def test_negative_slabs_give_a_level_of_128_triangle_nodes(tmp_path):
    """`negative` seed 4 at yaw 0: the x axis cuts the mesh into its eight slabs, so one level holds
    eight nodes of exactly 128 triangles whose y centroids are all negative — the most a one-wave
    node of the device builder holds (every lane pair taken), on a level wide enough for one wave
    per node.  Read from the host tree, which test_host_builders_match_reference pins to the golden."""
    from gp1_raytracer_2223_amd.scene import HostScene
    case = mesh_fuzz.make("negative", 4)
    hs = HostScene(f"file:{case.write(tmp_path)}", asset_dir=str(tmp_path))
    hs.update(case.times[0])
    m = hs.arrays()["meshes"][0]
    links = m["node_links"].reshape(-1, 3)

    def count(k):
        return int(links[k, 1]) // 3 if links[k, 1] else count(links[k, 2]) + count(links[k, 2] + 1)
    level = [0]
    for _ in range(3):
        assert all(links[k, 1] == 0 for k in level)
        level = [c for k in level for c in (links[k, 2], links[k, 2] + 1)]
    assert [count(k) for k in level] == [128] * 8
    P, I = m["tpositions"].reshape(-1, 3), m["indices"].reshape(-1, 3)
    assert (P[I][:, :, 1] < 0).all()


def test_medium_and_large_leaves_exist():
    leaves = list(_leaves())
    assert any(65 <= n <= 128 for _, n in leaves)
    assert any(129 <= n <= 700 for _, n in leaves)
    assert any(n == 24 for name, n in leaves if name.startswith("dup_grid"))
    for seed, g in _cases("geometric"):
        assert int(g["first_leaf"][0]) >= 90, seed


def test_overflow_partitions_without_a_cost():
    """An infinite area makes `splitCost >= noSplitCost` false; the tree is far from a SAH tree."""
    for _, g in _cases("overflow"):
        for when in ("first", "last"):
            assert 1 < int(g[f"{when}_nodes"][0]) < int(g[f"{when}_triangles"][0]) / 4
            assert int(g[f"{when}_inf"][0]) == 0    # the bounds themselves are finite: the area overflows


def test_every_tree_is_shallower_than_the_render_stack():
    for name in IDS:
        g = _golden(name)
        assert int(g["first_depth"].max()) < STACK_DEPTH and int(g["last_depth"].max()) < STACK_DEPTH, name


def test_flat_grid_ties_resolve_into_a_complete_tree():
    """At yaw 0 the 8 x 8 grid, centred or with a corner at the origin, splits down to 64 leaves of two
    triangles (127 nodes, 7 levels): every tie between planes and between x and z went the
    reference's way.  (Away from the origin the centroid rounding breaks the ties: seed 2.)"""
    complete = 0
    for seed, g in _cases("flat_grid"):
        assert int(g["first_triangles"][0]) == 128 and int(g["first_leaf"][0]) == 2
        if seed in (0, 1):
            assert (int(g["first_nodes"][0]), int(g["first_depth"][0])) == (127, 7), seed
            complete += 1
        else:
            assert int(g["first_nodes"][0]) > 127, seed
    assert complete == 2


def test_caps_sizes():
    assert [int(g["first_triangles"][0]) for _, g in _cases("caps")] == list(mesh_fuzz.CAPS_T)


def test_mixed_scene_holds_a_large_and_a_tiny_mesh():
    (_, g), = _cases("mixed")
    T = [int(x) for x in g["first_triangles"]]
    assert 7 <= len(T) <= 9 and max(T) > 3136 and min(T) <= 4
    assert mesh_fuzz.make("mixed", 0).text.count(" spin") == len(T) - 1    # one static mesh


def test_no_signed_zero_reached_the_world_positions():
    """The scene grammar cannot produce a -0 position or bound (TransformPoint ends by adding the
    translation term); recorded per case, so a generator that does produce one shows here."""
    for name in IDS:
        g = _golden(name)
        assert int(g["first_negzero"].sum()) == 0 and int(g["last_negzero"].sum()) == 0, name


def test_frames_show_the_meshes(tmp_path):
    """The golden frames look at the meshes: the CPU hit-plane checker finds triangle pixels in every
    case's final frame (of at least two triangles where the mesh has nine or more) — but for `overflow`, where
    Moller-Trumbore itself overflows at 1e19 and no ray hits a triangle, in the reference either."""
    import aov_ref
    import checkers
    from gp1_raytracer_2223_amd.scene import HostScene
    lib = checkers.lib()
    for family, seed in mesh_fuzz.COMMITTED:
        case = mesh_fuzz.make(family, seed)
        d = tmp_path / case.name
        d.mkdir()
        hs = HostScene(f"file:{case.write(d)}", asset_dir=str(d))
        for t in case.times:
            hs.update(t)
        s, cam = hs.view()
        prim = aov_ref.planes(lib, s, cam, W, H)["primitive"]
        tri = aov_ref.kind(prim) == 3
        if family == "overflow":
            assert not tri.any(), case.name
        else:
            assert tri.sum() >= 4, (case.name, int(tri.sum()))
            assert len(np.unique(prim[tri])) >= (2 if sum(case.triangles.values()) >= 9 else 1), case.name
