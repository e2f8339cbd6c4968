"""Known-answer vectors of the reference's primitive functions (GeometryUtils::HitTest_*,
SlabTest_BVH, Material::Shade), captured from the reference build, against the oracle: seeded ordinary
operands (prims.npz: origins in +-3, unit directions) and the rows of tests/walk_domains.py at the edges
of the ray kernels' fast-path domains (prims_domains.npz: directions of 2^+-60, origins of 2^40 to 2^120,
triangles with |e1||e2| = 2^56, where Vector3::Cross's `0 *` terms turn an infinity into NaN)."""
from pathlib import Path

import ctypes as C
import numpy as np

import oracle_bind
from gp1_raytracer_2223_amd import abi

G = np.load(Path(__file__).resolve().parent / "golden" / "prims.npz")
F = oracle_bind.fptr


def _rows(name, w):
    return G[name].reshape(-1, w).astype(np.float32)


def _eq(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _eq_nan(a, b):
    """Bit for bit, a NaN equal to any NaN (x86 and the reference build may differ in NaN payloads)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def _hold(G, _eq):
    """The oracle's four primitive tests, closest and any, against the vectors of G under _eq."""
    def _rows(name, w):
        return G[name].reshape(-1, w).astype(np.float32)
    L = oracle_bind.lib()
    rays, sph, pl, tri = _rows("rays", 8), _rows("spheres", 4), _rows("planes", 6), _rows("triangles", 12)
    cull, aabb = G["tri_cull"], _rows("aabbs", 6)
    exp_s, exp_p, exp_t = _rows("sphere_hit", 8), _rows("plane_hit", 8), _rows("tri_hit", 8)
    out = np.zeros(8, np.float32)
    bad = []
    for i in range(len(rays)):
        r = np.ascontiguousarray(rays[i])
        for fn, prim, exp, anyv in ((L.rtx_oracle_hit_sphere, sph, exp_s, G["sphere_any"]),
                                    (L.rtx_oracle_hit_plane, pl, exp_p, G["plane_any"])):
            hit = fn(F(r), F(np.ascontiguousarray(prim[i])), 0, F(out))
            if hit and not _eq(out, exp[i]) or bool(hit) != bool(exp[i, 0]):
                bad.append((fn.__name__, i))
            if bool(fn(F(r), F(np.ascontiguousarray(prim[i])), 1, F(out))) != bool(anyv[i]):
                bad.append((fn.__name__ + "/any", i))
        hit = L.rtx_oracle_hit_triangle(F(r), F(np.ascontiguousarray(tri[i])), int(cull[i]), 0, F(out))
        if bool(hit) != bool(exp_t[i, 0]) or (hit and not _eq(out, exp_t[i])):
            bad.append(("tri", i))
        if bool(L.rtx_oracle_hit_triangle(F(r), F(np.ascontiguousarray(tri[i])), int(cull[i]), 1, F(out))) != \
                bool(G["tri_any"][i]):
            bad.append(("tri/any", i))
        if bool(L.rtx_oracle_slab(F(r), F(np.ascontiguousarray(aabb[i])))) != bool(G["slab"][i]):
            bad.append(("slab", i))
    assert not bad, bad[:10]
    # the vectors exercise both outcomes of every test
    for k in ("sphere_any", "plane_any", "tri_any", "slab"):
        assert 0 < G[k].sum() < len(G[k]), k


def test_sphere_plane_triangle_slab():
    _hold(G, _eq)


def test_the_same_at_the_edges_of_the_fast_path_domains():
    """prims_domains.npz is what the reference answers on walk_domains.prim_rows(): the rows are the
    committed ones, some triangle hits carry the NaN t that Vector3::Cross's `0 *` terms make, and the
    oracle answers the same everywhere, bit for bit with a NaN equal to any NaN."""
    import walk_domains
    D = np.load(Path(__file__).resolve().parent / "golden" / "prims_domains.npz")
    rows = walk_domains.prim_rows()
    assert 200 <= rows.shape[0] <= 600
    assert _eq(D["rays"].reshape(-1, 8), rows[:, 0:8]) and _eq(D["triangles"].reshape(-1, 12)[:, 0:9], rows[:, 8:17])
    assert np.array_equal(D["tri_cull"], rows[:, 17].astype(np.int32)) and set(D["tri_cull"].tolist()) == {0, 1, 2}
    assert _eq(D["aabbs"].reshape(-1, 6), rows[:, 18:24]) and _eq(D["planes"].reshape(-1, 6), rows[:, 24:30])
    assert _eq(D["spheres"].reshape(-1, 4), rows[:, 30:34])
    th = D["tri_hit"].reshape(-1, 8)
    nan_hits = (th[:, 0] == 1) & np.isnan(th[:, 1])
    assert nan_hits.sum() >= 8 and np.isnan(th[nan_hits, 2:5]).all()
    assert ((th[:, 0] == 1) & np.isfinite(th[:, 1])).sum() >= 50
    _hold(D, _eq_nan)


def test_shade_materials():
    L = oracle_bind.lib()
    kinds, ins, outs = G["shade_kind"], _rows("shade_in", 17), _rows("shade_out", 3)
    o = np.zeros(3, np.float32)
    bad = []
    for i in range(len(kinds)):
        n, l, v = ins[i, 0:3].copy(), ins[i, 3:6].copy(), ins[i, 6:9].copy()
        m = abi.Material()
        m.kind = int(kinds[i])
        m.color[0], m.color[1], m.color[2] = map(float, ins[i, 9:12])
        m.kd, m.ks, m.exponent, m.metalness, m.roughness = map(float, ins[i, 12:17])
        L.rtx_oracle_shade(C.byref(m), F(n), F(l), F(v), F(o))
        if not _eq(o, outs[i]):
            bad.append((i, int(kinds[i]), o.tolist(), outs[i].tolist()))
    assert not bad, bad[:5]
