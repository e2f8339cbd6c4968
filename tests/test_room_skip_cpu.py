"""The room skip's condition against the reference's own plane test, in numpy binary32 (no GPU, no
reference tree).

The render kernel runs no shadow-ray room-plane test in a wave whose shadow origins all satisfy the
lane condition below while the uploaded scene has the host fact (csrc/rtx_hip.hip room_clear,
csrc/rtx_pack.cpp room_skip).  That is only allowed where HitTest_Plane (Utils.h:82-98) on the
reference's shadow ray (Renderer.cpp:128-140: l = L - o, tmax = l.Normalize(), tmin = 1e-4) fails
for every room plane.  Both are restated here and driven with the catalogue room and adversarial
origins and lights: no case that satisfies the condition may be a plane hit.
"""
import numpy as np

F = np.float32
# the catalogue room (Scene.cpp:263-267): plane k = (origin, normal), axis kRoomAxes[k]
PLANES = [((0, 0, 10), (0, 0, -1)), ((0, 0, 0), (0, 1, 0)), ((0, 10, 0), (0, -1, 0)),
          ((5, 0, 0), (-1, 0, 0)), ((-5, 0, 0), (1, 0, 0))]
AXES = [2, 1, 1, 0, 0]
LO = np.array([-5, 0, -40], F)    # the room's box (open down -z: the camera's side)
HI = np.array([5, 10, 10], F)
N = 400_000


def _step(x, k):
    """x moved by k floats (k an int array; the floats' own order, -0 next to +0)."""
    i = x.astype(F).view(np.int32).astype(np.int64)
    key = np.where(i < 0, -(i & 0x7fffffff), i) + k
    i = np.where(key < 0, (-key) | 0x80000000, key)
    return i.astype(np.uint32).view(F)


def _near_walls(rng, n, offsets):
    """Points of the room with each coordinate, with probability 1/2, put at a wall + an offset."""
    p = (LO + (HI - LO) * rng.random((n, 3))).astype(F)
    for a, walls in enumerate([(-5, 5), (0, 10), (10,)]):
        pick = rng.random(n) < 0.5
        w = rng.choice(np.array(walls, F), n)
        inward = np.where(w == F(walls[0]) if len(walls) == 2 else np.zeros(n, bool), F(1), F(-1))
        p[:, a] = np.where(pick, offsets(w, inward, n), p[:, a])
    return p


def _cases(seed):
    rng = np.random.default_rng(seed)
    n = N // 4
    ulps = lambda w, inward, m: _step(w, rng.integers(-6, 7, m))
    offs = lambda w, inward, m: (w + inward * (F(1e-4) * (2 * rng.random(m)).astype(F))).astype(F)
    o_uniform = (LO + (HI - LO) * rng.random((n, 3))).astype(F)
    o_far = o_uniform.copy()
    o_far[:, 2] = -(10.0 ** rng.uniform(0, 30, n)).astype(F)    # far down the open side
    o = np.concatenate([o_uniform, _near_walls(rng, n, ulps), _near_walls(rng, n, offs), o_far])
    L_uniform = (LO + (HI - LO) * rng.random((N, 3))).astype(F)
    L_walls = _near_walls(rng, N, ulps)     # within 6 ulps of a wall: some just outside
    L = np.where((rng.random(N) < 0.5)[:, None], L_uniform, L_walls)
    return o[rng.permutation(N)], L


def _plane_hits(o, L):
    """HitTest_Plane of every room plane on the reference's shadow ray: (N, 5) bool."""
    with np.errstate(all="ignore"):
        l = (L - o).astype(F)
        mag = np.sqrt((l[:, 0] * l[:, 0] + l[:, 1] * l[:, 1] + l[:, 2] * l[:, 2]).astype(F)).astype(F)
        d = (l / mag[:, None]).astype(F)
        hits = []
        for p0, nrm in PLANES:
            p0, nrm = np.array(p0, F), np.array(nrm, F)
            a = (p0 - o).astype(F)
            num = (a[:, 0] * nrm[0] + a[:, 1] * nrm[1] + a[:, 2] * nrm[2]).astype(F)
            den = (d[:, 0] * nrm[0] + d[:, 1] * nrm[1] + d[:, 2] * nrm[2]).astype(F)
            t = (num / den).astype(F)
            hits.append((t >= F(1e-4)) & (t < mag))
    return np.stack(hits, 1)


def _condition(o, L):
    """The host fact for the one light L, and the lane condition for the origin o."""
    m = np.stack([np.float64(nrm[A]) * (L[:, A].astype(np.float64) - np.float64(p0[A]))
                  for (p0, nrm), A in zip(PLANES, AXES)], 1)
    mmin, mmax = m.min(1), m.max(1)
    fact = np.isfinite(m).all(1) & (mmin > 0) & (mmax <= 2.0 ** 100 * mmin)
    Md = np.where(fact, 2.0 ** 20 * mmin, 0.0)
    M = Md.astype(F)
    M = np.where(M.astype(np.float64) > Md, np.nextafter(M, F(0)), M)     # rounded down
    a = np.stack([(F(p0[A]) - o[:, A]).astype(F) for (p0, _), A in zip(PLANES, AXES)], 1)
    s = np.array([nrm[A] for (_, nrm), A in zip(PLANES, AXES)], F)
    inside = ((a != 0) & (np.signbit(a) != np.signbit(s)[None, :])).all(1)
    return fact & (M > 0) & inside & (np.abs(a).max(1) <= M)


def test_no_qualifying_case_is_a_plane_hit():
    o, L = _cases(20240607)
    hit = _plane_hits(o, L).any(1)
    cond = _condition(o, L)
    print(f"cases {N}, qualifying {int(cond.sum())}, violations {int((cond & hit).sum())}, "
          f"hits among the rest {int((~cond & hit).sum())}")
    bad = np.flatnonzero(cond & hit)
    assert bad.size == 0, f"{bad.size} qualifying cases hit a room plane, first: o={o[bad[0]]!r} L={L[bad[0]]!r}"
    # not vacuous
    assert cond.mean() >= 0.05, f"only {cond.mean():.3%} of the cases satisfy the condition"
    assert (~cond & hit).sum() > 0, "no plane hit among the cases outside the condition"


def test_condition_rejects_what_it_must():
    """Spot checks of the condition itself: an origin on or behind a wall, a light on or behind one,
    a non-finite origin, and an origin too far for the light's margin."""
    L = np.array([[0, 5, 0]], F)
    ok = np.array([[1, 1e-4, 3]], F)
    assert _condition(ok, L)[0]
    for bad_o in ([5, 1, 3], [1, 0, 3], [1, -1e-4, 3], [1, 1, 10.5], [np.nan, 1, 3], [1, np.inf, 3], [1, 1, -np.inf]):
        assert not _condition(np.array([bad_o], F), L)[0], bad_o
    for bad_L in ([5, 5, 0], [0, 0, 0], [0, 5, 10], [0, 5, 11], [-6, 5, 0], [np.nan, 5, 0]):
        assert not _condition(ok, np.array([bad_L], F))[0], bad_L
    near = np.array([[np.nextafter(F(5), F(0)), 5, 0]], F)      # one ulp inside: M = 2^20 * 2^-21 = 0.5
    assert not _condition(ok, near)[0]
    assert not _condition(np.array([[1, 1, -2e7]], F), L)[0]     # |a_z| above 2^20 * 5
