"""Shaded rays (rtx_shade_rays*: rtx_shade_kernel) on the GPU against the checker of tests/shade_ref.py.
Bit-exact (a NaN float equals any NaN) wherever the reference calls no powf: the modes ObservedArea and
Radiance on every scene and every mode on the pow-free scenes, with every ray set of tests/rayq_rays.py
and the lengths around a wave boundary.  In Combined and BRDF on scenes with Phong or Cook-Torrance
materials the frames' bound (1e-4 per float channel, 1 LSB per 8-bit channel, test_gpu_parity._compare)
holds for the unit-direction sets `primary` and `shadow`; the other sets must run and equal the checker
wherever it reports a miss (no error bound is held on powf of an unnormalised view vector).  Also: equal
to a frame on the frame's own rays, the fuzz scenes and committed goldens, deep stacks in LDS and HBM,
launch chunking, the device variants, isolation from frames and passes, a device Update, the Python
Renderer, the error table and the CLI's --rays."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch   # at collection, before librtx_hip.so is loaded: imported after it, torch finds no device

import aov_ref
import gpu_support as gs
import oracle_bind
import rayq_rays
import rayq_ref
import shade_ref
from checkers import checker  # noqa: F401
from gp1_raytracer_2223_amd import abi
from gp1_raytracer_2223_amd.renderer import AOV_ALL, DeviceAnimation, DeviceContext, Renderer, aov_host_planes
from gp1_raytracer_2223_amd.scene import HostScene
from gpu_support import DEV
from gpu_support import ctx  # noqa: F401
from test_gpu_parity import POW_FREE, _compare
from test_gpu_rayq import PARITY

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
EXE = ROOT / "gp1_raytracer_2223_amd" / "lib" / "rtx_render"
W, H = 37, 23
SEED = 7
OA, RADIANCE, BRDF, COMBINED = (abi.RTX_MODE_OBSERVED_AREA, abi.RTX_MODE_RADIANCE, abi.RTX_MODE_BRDF,
                                abi.RTX_MODE_COMBINED)
ALL_CONFIGS = [(m, s) for m in range(4) for s in (1, 0)]
FEW_CONFIGS = [(COMBINED, 1), (OA, 0)]
UNIT_SETS = ("primary", "shadow")


_rays = {}
_want = {}


def _sets(checker, name, t=-1.0):
    """{set: rays} of a catalogue scene: every set that applies to it, made once and never written to."""
    key = (name, t)
    if key not in _rays:
        s, cam = gs.view(name, t)
        sets = {"primary": rayq_ref.primary(checker, cam, W, H), "scatter": rayq_rays.scatter(SEED, 512),
                "nonfinite": rayq_rays.nonfinite(s, SEED)}
        if s.n_lights:
            sets["shadow"] = rayq_ref.shadow(checker, s, cam, W, H, 0)[0]
        if s.n_meshes:
            sets["aimed"] = rayq_rays.aimed(s, SEED, 512)
            sets["octant"] = rayq_rays.octant(s, SEED)
        for a in sets.values():
            a.setflags(write=False)
        _rays[key] = sets
    return _rays[key]


def _ref(checker, name, t, k, mode, shadows):
    """The checker's (pixels, rgb, flags) of set k of a catalogue scene, computed once per configuration."""
    key = (name, t, k, mode, shadows)
    if key not in _want:
        out = shade_ref.shade(checker, gs.view(name, t)[0], _sets(checker, name, t)[k], shade_ref.params(mode, shadows))
        for a in out:
            a.setflags(write=False)
        _want[key] = out
    return _want[key]


def _lengths(n):
    return (n,) + tuple(k for k in rayq_rays.LENGTHS if k < n)


def _exact(c, rays, p, want_px, want_rgb, what):
    """The whole set and its four short prefixes, word for word."""
    for n in _lengths(rays.shape[0]):
        px, rgb = c.shade_rays(rays[:n], p)
        assert px.dtype == np.uint32 and rgb.dtype == np.float32 and px.shape == (n,) and rgb.shape == (3 * n,)
        bad = np.nonzero(px != want_px[:n])[0]
        assert bad.size == 0, f"{what}, n = {n}: pixels differ at rays {bad[:8].tolist()}"
        assert aov_ref.same(rgb, want_rgb[:3 * n]), f"{what}, n = {n}: rgb differs"


@pytest.mark.parametrize("name,t", PARITY)
def test_parity(ctx, checker, name, t):
    s, _ = gs.view(name, t)
    ctx.upload(s)
    for k, rays in _sets(checker, name, t).items():
        assert 65 < rays.shape[0] <= 2048, (k, rays.shape)
        for mode, shadows in (ALL_CONFIGS if k in ("primary", "aimed") else FEW_CONFIGS):
            want_px, want_rgb, flags = _ref(checker, name, t, k, mode, shadows)
            p = shade_ref.params(mode, shadows)
            what = f"{name}/t{t}/{k}/m{mode}/s{shadows}"
            if mode in (OA, RADIANCE) or name in POW_FREE:
                _exact(ctx, rays, p, want_px, want_rgb, what)
                continue
            for n in _lengths(rays.shape[0]):   # powf runs: Combined or BRDF with Phong / Cook-Torrance materials
                px, rgb = ctx.shade_rays(rays[:n], p)
                if k in UNIT_SETS:
                    d = np.abs(rgb - want_rgb[:3 * n])
                    print(f"{what}, n = {n}: max-abs {float(d.max(initial=0.0)):.3g}")
                    _compare(f"{what}, n = {n}", px, rgb, want_px[:n], want_rgb[:3 * n], exact=False)
                else:
                    miss = (flags[:n] & shade_ref.HIT) == 0
                    assert np.array_equal(px[miss], want_px[:n][miss]), what
                    assert aov_ref.same(rgb.reshape(-1, 3)[miss], want_rgb[:3 * n].reshape(-1, 3)[miss]), what


@pytest.mark.parametrize("name", ["W4_Bunny", "W3"])
def test_primary_rays_equal_the_frame(ctx, checker, name):
    """Both are the device's own arithmetic, powf included: word for word on every scene."""
    s, cam = gs.view(name)
    ctx.upload(s)
    rays = _sets(checker, name)["primary"]
    for mode, shadows in ALL_CONFIGS:
        p = abi.make_params(W, H, mode, shadows)
        fpx, frgb = ctx.render(cam, p)
        px, rgb = ctx.shade_rays(rays, p)
        assert np.array_equal(px, fpx), (name, mode, shadows, np.nonzero(px != fpx)[0][:8].tolist())
        assert aov_ref.same(rgb, frgb), (name, mode, shadows)


CASES = aov_ref.golden_cases()


@pytest.mark.parametrize("family,seed", CASES, ids=[f"{f}_{s}" for f, s in CASES])
def test_fuzz_scenes(ctx, checker, tmp_path, family, seed):
    keep, s, cam = aov_ref.golden_view(family, seed, tmp_path)
    ctx.upload(s)
    rays = np.concatenate([rayq_ref.golden_rays(s), rayq_ref.primary(checker, cam, aov_ref.GOLDEN_W, aov_ref.GOLDEN_H)[:448]])
    assert rays.shape[0] <= 2048
    for mode in (OA, RADIANCE):
        p = shade_ref.params(mode, True)
        want_px, want_rgb, _ = shade_ref.shade(checker, s, rays, p)
        _exact(ctx, rays, p, want_px, want_rgb, f"{family}_{seed}/m{mode}")
    del keep


@pytest.mark.parametrize("file,case,mode", shade_ref.GOLDEN_CASES, ids=[f for f, _, _ in shade_ref.GOLDEN_CASES])
def test_committed_goldens(ctx, tmp_path, file, case, mode):
    keep, s, _ = rayq_ref.golden_view(case, tmp_path)
    g = np.load(shade_ref.GOLDEN / f"{file}.npz")
    ctx.upload(s)
    px, rgb = ctx.shade_rays(g["rays"], shade_ref.params(shade_ref.MODES[mode], True))
    # (a fuzz scene with Phong or Cook-Torrance materials in Combined: the rays that miss)
    sel = np.ones(px.size, bool) if (mode in ("ObservedArea", "Radiance") or shade_ref.pow_free(s)) else \
        (g["flags"] & shade_ref.HIT) == 0
    assert sel.any()
    assert np.array_equal(px[sel], g["pixels"][sel]), file
    assert aov_ref.same(rgb.reshape(-1, 3)[sel], g["rgb"].reshape(-1, 3)[sel]), file
    del keep


@pytest.mark.parametrize("T", [300, 1100])
def test_deep_stack_variants(ctx, checker, T):
    """T = 300: the deep LDS stack (DEEP); 1100: the stacks in HBM (DEEP + HSTK)."""
    from test_gpu_deep_bvh import deep_scene
    s, cam, keep = deep_scene(T)
    ctx.upload(s)
    rays = np.concatenate([rayq_rays.aimed(s, SEED, 512), rayq_rays.octant(s, SEED), rayq_rays.nonfinite(s, SEED)])
    tri = aov_ref.kind(rayq_ref.trace(checker, s, rays)["primitive"]) == 3
    assert tri.mean() >= 0.05, tri.mean()
    p = shade_ref.params(OA, True)
    want_px, want_rgb, flags = shade_ref.shade(checker, s, rays, p)
    assert (want_px != 0).any()
    _exact(ctx, rays, p, want_px, want_rgb, f"chain of {T}")
    del keep


def test_hbm_stacks_cut_a_large_call_into_launches(ctx, checker):
    """A 2,500-level chain needs 60 KB of HBM stack per wave and a launch asks for at most 256 MB of
    stacks: 300,000 rays are two launches (286,208 + 13,792).  The rays are 2,048 distinct ones repeated,
    so the checker's outputs repeated are the expectation for every launch's part: the two output
    pointers advance by n and 3n."""
    from test_gpu_deep_bvh import deep_scene
    T, n = 2500, 300_000
    s, cam, keep = deep_scene(T)
    ctx.upload(s)
    base = rayq_rays.aimed(s, SEED, 2048)
    p = shade_ref.params(OA, True)
    bpx, brgb, flags = shade_ref.shade(checker, s, base, p)
    # (the base pattern is no constant: hits and misses, and several grey levels among the hits)
    assert 0.05 <= ((flags & shade_ref.HIT) != 0).mean() <= 0.95 and np.unique(bpx).size >= 8
    reps = -(-n // 2048)
    rays = np.tile(base, (reps, 1))[:n]
    px, rgb = ctx.shade_rays(rays, p)
    assert np.array_equal(px, np.tile(bpx, reps)[:n])
    assert aov_ref.same(rgb, np.tile(brgb.reshape(-1, 3), (reps, 1))[:n].reshape(-1))
    del keep


SENT = np.uint32(0xC0FFEE11)


def test_device_variant_and_output_subsets(ctx, checker):
    """Rays and outputs as torch tensors.  Pixels and rgb lie in one sentinel-filled buffer of 32-bit
    words with guard words around them: a call writes the outputs it was given and nothing else."""
    torch, dev = gs.torch_device()
    s, _ = gs.view("W4_Bunny")
    ctx.upload(s)
    rays = _sets(checker, "W4_Bunny")["aimed"]
    p = shade_ref.params(COMBINED, True)
    want_px, want_rgb, _ = _ref(checker, "W4_Bunny", -1.0, "aimed", COMBINED, 1)
    for n in (rays.shape[0], 65, 1):
        d_rays = torch.from_numpy(np.array(rays[:n])).to(dev)
        guard = 64
        off_px, off_rgb = guard, guard + n + guard
        total = off_rgb + 3 * n + guard
        for use_px, use_rgb in ((True, True), (True, False), (False, True)):
            buf = torch.full((total,), int(np.int32(SENT.view(np.int32))), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            ctx.shade_rays_device(d_rays.data_ptr(), n, p, buf.data_ptr() + 4 * off_px if use_px else 0,
                                  buf.data_ptr() + 4 * off_rgb if use_rgb else 0)
            ctx.synchronize()
            host = buf.cpu().numpy().view(np.uint32)
            keep = np.ones(total, bool)
            if use_px:
                assert np.array_equal(host[off_px:off_px + n], want_px[:n]), (n, use_px, use_rgb)
                keep[off_px:off_px + n] = False
            if use_rgb:
                assert aov_ref.same(host[off_rgb:off_rgb + 3 * n].view(np.float32), want_rgb[:3 * n]), (n, use_px, use_rgb)
                keep[off_rgb:off_rgb + 3 * n] = False
            assert (host[keep] == SENT).all(), (n, use_px, use_rgb)


def test_frames_and_passes_are_untouched(checker):
    torch, dev = gs.torch_device()
    s, cam = gs.view("W4_Bunny")
    rays = _sets(checker, "W4_Bunny")["aimed"]
    n = rays.shape[0]
    want_px, want_rgb, _ = _ref(checker, "W4_Bunny", -1.0, "aimed", COMBINED, 1)
    p = abi.make_params(W, H)
    c = DeviceContext(DEV)
    try:
        c.upload(s)
        gs.renders_correctly(c, s, cam, W, H)
        spec, sched = c.spec_info(), c.split_info()
        pass_planes = c.render_aov(cam, p)
        px, rgb = c.shade_rays(rays, p)
        assert shade_ref.same(px, rgb, want_px, want_rgb)
        # the hit pass's planes and its last-pass record, between the pass and its download
        again = c.download_aov(aov_host_planes(W, H, AOV_ALL))
        assert not aov_ref.diff(again, pass_planes)
        # the colour frame buffer and the last-frame record
        fpx = np.full(W * H, 0xDEADBEEF, np.uint32)
        c.gather_async(fpx)
        c.synchronize()
        assert np.array_equal(fpx, oracle_bind.render(s, cam, p)[0])
        gs.renders_correctly(c, s, cam, W, H)
        assert c.spec_info() == spec and c.split_info() == sched
        # a call between two frames in flight changes neither
        cam2 = abi.Camera()
        C.memmove(C.byref(cam2), C.byref(cam), C.sizeof(abi.Camera))
        cam2.origin[0] = cam.origin[0] + 0.5
        d_rays = torch.from_numpy(np.array(rays)).to(dev)
        d_px = torch.zeros(n, dtype=torch.int32, device=dev)
        d_rgb = torch.zeros(3 * n, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        pa, pb = np.zeros(W * H, np.uint32), np.zeros(W * H, np.uint32)
        c.render_async(cam, p)
        c.gather_async(pa)
        c.shade_rays_device(d_rays.data_ptr(), n, p, d_px.data_ptr(), d_rgb.data_ptr())
        c.render_async(cam2, p)
        c.gather_async(pb)
        c.synchronize()
        assert np.array_equal(pa, oracle_bind.render(s, cam, p)[0])
        assert np.array_equal(pb, oracle_bind.render(s, cam2, p)[0])
        assert shade_ref.same(d_px.cpu().numpy().view(np.uint32), d_rgb.cpu().numpy(), want_px, want_rgb)
        # shaded rays are not frames: a supersample factor does not matter
        c.set_supersample(2)
        assert shade_ref.same(*c.shade_rays(rays, p), want_px, want_rgb)
        c.set_supersample(1)
        gs.renders_correctly(c, s, cam, W, H)
    finally:
        c.close()


def test_device_update(checker):
    """After a device Update a call sees the rebuilt mesh: the checker runs on rtx_anim_download's geometry."""
    dev_scene = HostScene("W4_Bunny")
    s0, _ = dev_scene.view()
    c = DeviceContext(DEV)
    anim = DeviceAnimation(dev_scene, c)
    try:
        anim.update(1.3, c)
        assert list(anim.status(0)[:1]) == [0] and len(anim.mesh_ids) == 1 and s0.n_meshes == 1
        g = anim.download(0)
        used = int(anim.status(0)[2])
        nodes = (abi.BVHNode * used)()
        raw = np.ascontiguousarray(g["nodes"][:used], np.uint32)
        C.memmove(nodes, raw.ctypes.data, used * C.sizeof(abi.BVHNode))
        pos, idx, nrm = (np.ascontiguousarray(g[k]) for k in ("tpositions", "indices", "tnormals"))
        m = abi.Mesh()
        m.positions, m.n_positions = pos.ctypes.data_as(C.POINTER(C.c_float)), pos.size // 3
        m.indices, m.n_indices = idx.ctypes.data_as(C.POINTER(C.c_int32)), idx.size
        m.normals = nrm.ctypes.data_as(C.POINTER(C.c_float))
        m.nodes, m.n_nodes = nodes, used
        m.cull_mode, m.material = s0.meshes[0].cull_mode, s0.meshes[0].material
        meshes = (abi.Mesh * 1)(m)
        s = abi.Scene()
        C.memmove(C.byref(s), C.byref(s0), C.sizeof(abi.Scene))
        s.meshes = meshes
        rays = np.concatenate([rayq_rays.aimed(s, SEED, 512), rayq_rays.octant(s, SEED)])
        p = shade_ref.params(COMBINED, True)
        want_px, want_rgb, flags = shade_ref.shade(checker, s, rays, p)
        assert ((flags & shade_ref.HIT) != 0).mean() >= 0.25
        _exact(c, rays, p, want_px, want_rgb, "after a device Update")
        # ... and the turned mesh is not the uploaded one
        still_px, _, _ = shade_ref.shade(checker, s0, rays, p)
        assert not np.array_equal(still_px, want_px)
    finally:
        anim.close()
        c.close()


def test_renderer_follows_mode_and_shadows(checker):
    rays = _sets(checker, "W4_Bunny")["aimed"]
    r = Renderer(W, H, device=DEV)
    try:
        hs = HostScene("W4_Bunny")
        mode, shadows = COMBINED, 1
        px, rgb = r.ShadeRays(hs, rays)
        assert shade_ref.same(px, rgb, *_ref(checker, "W4_Bunny", -1.0, "aimed", mode, shadows)[:2])
        for step in range(4):   # Combined -> ObservedArea -> Radiance -> BRDF -> Combined, shadows toggled on the way
            r.CycleLightingMode()
            mode = (mode + 1) % 4
            if step % 2 == 0:
                r.ToggleShadows()
                shadows ^= 1
            px, rgb = r.ShadeRays(hs, rays, upload=False)
            assert shade_ref.same(px, rgb, *_ref(checker, "W4_Bunny", -1.0, "aimed", mode, shadows)[:2]), (mode, shadows)
        assert mode == COMBINED and shadows == 1
    finally:
        r.ctx.close()


def test_errors_leave_the_context_usable(checker):
    s, cam = gs.view("W4_Bunny")
    rays = _sets(checker, "W4_Bunny")["aimed"]
    want_px, want_rgb, _ = _ref(checker, "W4_Bunny", -1.0, "aimed", COMBINED, 1)
    n = rays.shape[0]
    c = DeviceContext(DEV)
    lib, h = c.lib, c.h
    rp = np.array(rays).ctypes.data_as(C.POINTER(abi.Ray))
    px, rgb = np.zeros(n, np.uint32), np.zeros(3 * n, np.float32)
    pp, rgbp = px.ctypes.data_as(C.POINTER(C.c_uint32)), rgb.ctypes.data_as(C.POINTER(C.c_float))
    p = shade_ref.params(COMBINED, True)
    P = C.byref(p)

    def still_works(after):
        assert shade_ref.same(*c.shade_rays(rays, p), want_px, want_rgb), after

    try:
        # no scene uploaded
        assert lib.rtx_shade_rays(h, rp, n, P, pp, rgbp) == abi.RTX_E_STATE
        assert b"no scene" in lib.rtx_last_error(h)
        assert lib.rtx_shade_rays_device(h, 256, n, P, 256, None) == abi.RTX_E_STATE
        c.upload(s)
        still_works("the calls without a scene")
        # NULL ctx, rays, params, and both outputs
        assert lib.rtx_shade_rays(None, rp, n, P, pp, rgbp) == abi.RTX_E_INVALID
        assert lib.rtx_shade_rays_device(None, 256, n, P, 256, 256) == abi.RTX_E_INVALID
        still_works("a NULL context")
        assert lib.rtx_shade_rays(h, None, n, P, pp, rgbp) == abi.RTX_E_INVALID
        assert lib.rtx_shade_rays_device(h, None, n, P, 256, 256) == abi.RTX_E_INVALID
        still_works("NULL rays")
        assert lib.rtx_shade_rays(h, rp, n, None, pp, rgbp) == abi.RTX_E_INVALID
        assert lib.rtx_shade_rays_device(h, 256, n, None, 256, 256) == abi.RTX_E_INVALID
        still_works("NULL params")
        assert lib.rtx_shade_rays(h, rp, n, P, None, None) == abi.RTX_E_INVALID
        assert b"output" in lib.rtx_last_error(h)
        assert lib.rtx_shade_rays_device(h, 256, n, P, None, None) == abi.RTX_E_INVALID
        still_works("no output")
        # the lighting mode, checked as rtx_render checks it
        for bad in (-1, 4):
            q = shade_ref.params(COMBINED, True)
            q.lighting_mode = bad
            assert lib.rtx_shade_rays(h, rp, n, C.byref(q), pp, rgbp) == abi.RTX_E_INVALID, bad
            assert b"lighting mode" in lib.rtx_last_error(h)
            assert lib.rtx_shade_rays_device(h, 256, n, C.byref(q), 256, 256) == abi.RTX_E_INVALID, bad
        assert (px == 0).all() and (rgb == 0).all()
        still_works("a bad lighting mode")
        # n == 0: nothing launched, nothing needed
        assert lib.rtx_shade_rays(h, None, 0, P, None, None) == abi.RTX_OK
        assert lib.rtx_shade_rays_device(h, None, 0, P, None, None) == abi.RTX_OK
        e_px, e_rgb = c.shade_rays(np.zeros((0, 8), np.float32), p)
        assert e_px.size == 0 and e_rgb.size == 0
        with pytest.raises(ValueError):
            c.shade_rays(np.zeros((4, 7), np.float32), p)
        still_works("the empty calls")
        # a good call through the raw entry point with one output fills only that one; width, height
        # and the stripe fields do not matter
        q = abi.make_params(4096, 3, COMBINED, True, stripe_rows=16, stripe_first=1, stripe_step=3)
        assert lib.rtx_shade_rays(h, rp, n, C.byref(q), pp, None) == abi.RTX_OK
        assert np.array_equal(px, want_px) and (rgb == 0).all()
        assert lib.rtx_shade_rays(h, rp, n, C.byref(q), None, rgbp) == abi.RTX_OK
        assert aov_ref.same(rgb, want_rgb)
        # the pixel format is the caller's
        q = shade_ref.params(COMBINED, True, (0, 8, 16, 0xFF000000))
        fpx, frgb = c.shade_rays(rays, q)
        w_px, w_rgb, _ = shade_ref.shade(checker, s, rays, q)
        assert shade_ref.same(fpx, frgb, w_px, w_rgb) and not np.array_equal(fpx, want_px)
        gs.renders_correctly(c, s, cam, W, H)
    finally:
        c.close()


def _bmp(path: Path) -> bytes:
    b = path.read_bytes()
    assert b[:2] == b"BM"
    return b


def test_cli_rays(checker, tmp_path):
    assert EXE.exists(), "rtx_render not built"
    w, h = 64, 48
    hs = HostScene("W4_Bunny")
    _, cam = hs.view()
    rayq_ref.primary(checker, cam, w, h).astype("<f4").tofile(tmp_path / "rays.f32")
    base = [str(EXE), "W4_Bunny", str(w), str(h)]
    subprocess.run(base + ["--out", str(tmp_path / "frame.bmp")], check=True, cwd=tmp_path, timeout=120)
    subprocess.run(base + ["--out", str(tmp_path / "rays.bmp"), "--rays", str(tmp_path / "rays.f32")], check=True,
                   cwd=tmp_path, timeout=120)
    assert _bmp(tmp_path / "rays.bmp") == _bmp(tmp_path / "frame.bmp")
    # single frames only: a usage error before any device work, and nothing written
    for extra in (["--benchmark", "1"], ["--sequence", "0.3,0.9"], ["--aov", str(tmp_path / "planes")], ["--ss", "2"]):
        r = subprocess.run(base + ["--out", str(tmp_path / "no.bmp"), "--rays", str(tmp_path / "rays.f32")] + extra,
                           cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "--rays" in r.stderr, (extra, r.returncode, r.stderr)
        assert sorted(q.name for q in tmp_path.iterdir()) == ["frame.bmp", "rays.bmp", "rays.f32"], extra
    # a file of another size is refused too
    (tmp_path / "short.f32").write_bytes((tmp_path / "rays.f32").read_bytes()[:-32])
    r = subprocess.run(base + ["--out", str(tmp_path / "no.bmp"), "--rays", str(tmp_path / "short.f32")], cwd=tmp_path,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and not (tmp_path / "no.bmp").exists()
