"""In-place scene edits (rtx_edit_lights, rtx_edit_materials and their _device forms: rtx_patch_kernel) on the GPU.

The contract under test: after any sequence of edits every entry point behaves word for word as if the scene
with those records replaced had been given to rtx_upload_scene.  So every case compares an EDITED context with a
FRESH context that uploaded the edited scene (`_same`): the scene image byte for byte, spec_info, room_info and
cull_info, a Combined + shadows frame in both planes, the hit pass followed by the shadow plane, and the relight in
all 8 mode / shadow configurations.  Frames are 64 x 48 unless a case says otherwise.

The edits are tests/edit_cases.py's; tests/test_edit_cpu.py shows on the CPU that its moves flip the room-skip
fact and that its material bit patterns hold denormals, huge values and both zeros."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch   # at collection, before librtx_hip.so is loaded: imported after it, torch finds no device

import edit_cases as EC
import gpu_support as gs
import oracle_bind
import pack_cases
import relight_ref
import shadow_update_scenes as sus
from checkers import checker  # noqa: F401
from gp1_raytracer_2223_amd import abi
from gp1_raytracer_2223_amd.renderer import AOV_ALL, DeviceAnimation, DeviceContext, Renderer
from gp1_raytracer_2223_amd.scene import HostScene
from gpu_support import CONFIGS, DEV, POW_FREE_MODES

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
LIB = ROOT / "gp1_raytracer_2223_amd" / "lib"
EXE = LIB / "rtx_render"
W, H = 64, 48
KMAXVIEWS = 8   # rtx_cull_dump: light l's anchor is record copy KMAXVIEWS + l


def _with(s, lights=None, materials=None):
    """A copy of the flat scene with its lights and / or materials replaced (sequences of records); the copy keeps
    its arrays."""
    s2 = abi.Scene()
    C.memmove(C.byref(s2), C.byref(s), C.sizeof(abi.Scene))
    keep = [s]
    if lights is not None:
        arr = (abi.Light * len(lights))(*lights)
        s2.lights, s2.n_lights = arr, len(lights)
        keep.append(arr)
    if materials is not None:
        arr = (abi.Material * len(materials))(*materials)
        s2.materials, s2.n_materials = arr, len(materials)
        keep.append(arr)
    s2._keep = keep
    return s2


def _bits(a):
    return a.view(np.uint32)


def _frame_eq(a, b, what):
    assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1])), what


def _info(c):
    return {"spec": c.spec_info(), "room": (c.room_info()[0], f"{np.float32(c.room_info()[1]).view(np.uint32):08x}"),
            "cull": c.cull_info()[0]}


def _same(c, s_edited, cam, what, oracle=True, w=W, h=H):
    """The edited context `c` against a fresh context that uploaded `s_edited`."""
    f = DeviceContext(DEV)
    try:
        f.upload(s_edited)
        assert np.array_equal(pack_cases.read_image(c), pack_cases.read_image(f)), f"{what}: scene image"
        assert c.room_info() == f.room_info() and c.cull_info()[0] == f.cull_info()[0], what
        p = abi.make_params(w, h)
        got, want = c.render(cam, p), f.render(cam, p)
        _frame_eq(got, want, f"{what}: frame")
        assert _info(c) == _info(f), what
        if oracle:   # the reference's own frame wherever it calls no powf
            for mode in POW_FREE_MODES:
                for sh in (0, 1):
                    q = abi.make_params(w, h, mode, sh)
                    _frame_eq(c.render(cam, q), oracle_bind.render(s_edited, cam, q), f"{what}: oracle mode {mode} shadows {sh}")
        planes = {}
        for x in (c, f):
            x.render_aov_async(cam, p, AOV_ALL)
            x.render_shadows_async()
            planes[x] = x.download_shadows()
        assert np.array_equal(planes[c], planes[f]), f"{what}: shadow plane"
        for mode, sh in CONFIGS:
            q = abi.make_params(w, h, mode, sh)
            _frame_eq(c.relight(q), f.relight(q), f"{what}: relight mode {mode} shadows {sh}")
        assert np.array_equal(pack_cases.read_image(c), pack_cases.read_image(f)), f"{what}: scene image afterwards"
        return got
    finally:
        f.close()


def _value_edit(s, round_=0):
    return ([EC.recolour(l, i, round_) for i, l in enumerate(EC.lights_of(s))],
            [EC.revalue(m, i, round_) for i, m in enumerate(EC.materials_of(s))])


# ---- 1. value edits ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["W4_Bunny", "W3", "W4_Reference"])
def test_value_edits(name):
    """Light colours and intensities and every material value, on a context whose schedule and cull view records
    are warm (a frame rendered before the edit), then again from first > 0 to the last record."""
    s, cam = gs.view(name)
    c = DeviceContext(DEV)
    try:
        c.upload(s)
        before = c.render(cam, abi.make_params(W, H))
        lights, mats = _value_edit(s)
        c.edit_lights(0, lights)
        c.edit_materials(0, mats)
        got = _same(c, _with(s, lights, mats), cam, f"{name} values")
        assert not np.array_equal(got[0], before[0]), "the edit changes nothing"
        lights2, mats2 = _value_edit(s, 4)
        c.edit_lights(1, lights2[1:])
        c.edit_materials(1, mats2[1:])
        _same(c, _with(s, lights[:1] + lights2[1:], mats[:1] + mats2[1:]), cam, f"{name} values from 1")
    finally:
        c.close()


@pytest.mark.parametrize("name", ["W4_Bunny", "Synthetic100k"])
def test_edit_as_the_first_call_after_upload(name):
    """The cull boxes and light records are pending then (Synthetic100k: exact cull on): the pending build must use
    the edited lights."""
    s, cam = gs.view(name)
    c = DeviceContext(DEV)
    try:
        c.upload(s)
        lights, mats = _value_edit(s)
        lights[0] = EC.moved(lights[0], EC.MOVE_IN)
        c.edit_lights(0, lights)
        c.edit_materials(0, mats)
        if name == "Synthetic100k":
            assert c.cull_info()[0]
        _same(c, _with(s, lights, mats), cam, f"{name} first call", oracle=name != "Synthetic100k")
    finally:
        c.close()


# ---- 2. moved lights --------------------------------------------------------------------------------------------

def _moved_light_round(c, checker, s_now, cam, l, origin, what):
    """On a context with current passes: move light l in place; the relight is refused, the refresh traces exactly
    light l, the plane is the checker's and the relight the frame.  Returns the edited scene."""
    lights = EC.lights_of(s_now)
    lights[l] = EC.moved(lights[l], origin)
    p = abi.make_params(W, H)
    c.edit_lights(l, [lights[l]])
    s2 = _with(s_now, lights)
    assert c.lib.rtx_relight_async(c.h, C.byref(p), 0) == abi.RTX_E_STATE, what   # (stale until the refresh)
    assert c.lib.rtx_relight_async(c.h, C.byref(abi.make_params(W, H, 3, 0)), 0) == abi.RTX_OK, what
    assert c.refresh_shadows_async() == 1 << l, what
    want, _ = relight_ref.plane(checker, s2, cam, W, H)
    assert np.array_equal(c.download_shadows(), want), f"{what}: plane"
    for mode, sh in CONFIGS:
        q = abi.make_params(W, H, mode, sh)
        relit = c.relight(q)
        _frame_eq(relit, c.render(cam, q), f"{what}: relight mode {mode} shadows {sh}")
    return s2


@pytest.mark.parametrize("which", ["room", "open", "W4_Bunny"])
def test_moved_lights(checker, tmp_path, which):
    """A move inside the room, out of it and back: the room-skip fact flips both ways (the two room scenes), and
    after every move the context is the fresh one."""
    if which == "W4_Bunny":
        s, cam = gs.view(which)
    else:
        hs = sus.file_scene(tmp_path, which, "base")
        s, cam = hs.view()
    room = which != "open"
    c = DeviceContext(DEV)
    try:
        p = abi.make_params(W, H)
        c.upload(s)
        c.render(cam, p)   # (a warm context)
        assert c.room_info()[0] == room
        home = tuple(s.lights[1].origin)
        now = s
        for k, (to, fact) in enumerate(((EC.MOVE_IN, room), (EC.MOVE_OUT, False), (home, room))):
            c.render_aov_async(cam, p, AOV_ALL)
            c.render_shadows_async()
            m0 = c.room_info()[1]
            now = _moved_light_round(c, checker, now, cam, 1, to, f"{which} move {k}")
            assert c.room_info()[0] == fact, f"{which} move {k}: room fact"
            if room:
                assert c.room_info()[1] != m0, f"{which} move {k}: room_M did not change"
            _same(c, now, cam, f"{which} move {k}")
    finally:
        c.close()


def _dump(ctx, anchor):
    ns = C.c_uint32()
    abi.check(ctx.lib.rtx_cull_dump(ctx.h, anchor, C.byref(ns), None, None, None, None, None, None), "dump", ctx.h)
    a = np.zeros(5, np.float32)
    rec = np.zeros(8 * ns.value, np.float32)
    abi.check(ctx.lib.rtx_cull_dump(ctx.h, anchor, C.byref(ns), None, a.ctypes.data, rec.ctypes.data, None, None, None),
              "dump", ctx.h)
    return a, rec


def test_moved_light_rebuilds_its_own_cull_anchor(checker):
    """Synthetic100k, exact cull on: after a move only the moved light's anchor records are rebuilt (equal to the
    fresh context's, like every other anchor's); the camera anchors are not (cull_updates stays)."""
    s, cam = gs.view("Synthetic100k")
    c, f = DeviceContext(DEV), DeviceContext(DEV)
    try:
        p = abi.make_params(W, H)
        c.upload(s)
        assert c.cull_info()[0]
        c.render(cam, p)
        c.render_aov_async(cam, p, AOV_ALL)
        c.render_shadows_async()
        updates = c.cull_info()[1]
        assert updates == 1   # the camera anchor, once
        old = [_dump(c, KMAXVIEWS + l) for l in range(s.n_lights)]
        l = s.n_lights - 1
        s2 = _moved_light_round(c, checker, s, cam, l, (1.0, 3.0, -2.0), "Synthetic100k move")
        assert c.cull_info() == (True, updates), "the camera anchors were rebuilt"
        f.upload(s2)
        f.render(cam, p)
        for k in range(s.n_lights):
            (ga, grec), (wa, wrec) = _dump(c, KMAXVIEWS + k), _dump(f, KMAXVIEWS + k)
            assert np.array_equal(_bits(ga), _bits(wa)) and np.array_equal(_bits(grec), _bits(wrec)), f"light anchor {k}"
            assert np.array_equal(_bits(grec), _bits(old[k][1])) == (k != l), f"light anchor {k} vs before the move"
        (ga, grec), (wa, wrec) = _dump(c, 0), _dump(f, 0)
        assert np.array_equal(_bits(ga), _bits(wa)) and np.array_equal(_bits(grec), _bits(wrec)), "camera anchor"
        _same(c, s2, cam, "Synthetic100k move", oracle=False)
    finally:
        c.close()
        f.close()


# ---- 3. device forms ----------------------------------------------------------------------------------------------

SENTINEL = 7.25e9


def _guarded(values: np.ndarray, shift: int = 0):
    """A device buffer holding `values` between sentinel floats, `shift` floats off the allocation's alignment;
    returns (tensor, device address of the values)."""
    flat = np.ascontiguousarray(values, np.float32).reshape(-1)
    host = np.full(64 + shift + flat.size + 64, SENTINEL, np.float32)
    host[64 + shift:64 + shift + flat.size] = flat
    t = torch.from_numpy(host).to(f"cuda:{DEV}")
    torch.cuda.synchronize(DEV)
    return t, t.data_ptr() + 4 * (64 + shift)


def test_device_material_values_equal_the_host_form():
    """16 rounds of 256 materials whose eight floats are random bit patterns (finite): the device form's Lambert
    term, product and division, gives the host form's image byte for byte.  A division by reciprocal or a contracted
    multiply-add would show here."""
    s, cam = gs.view("W4_Bunny")
    mats = EC.many_materials(s)
    s256 = _with(s, materials=list(mats))
    values = EC.random_material_values()
    mag = np.abs(values.astype(np.float64))
    assert ((mag > 0) & (mag < 2.0 ** -126)).any() and (mag > 2.0 ** 100).any()   # (the seed's condition)
    host, dev = DeviceContext(DEV), DeviceContext(DEV)
    try:
        host.upload(s256)
        dev.upload(s256)
        for r in range(values.shape[0]):
            host.edit_materials(0, EC.value_materials(mats, values[r]))
            t, ptr = _guarded(values[r], shift=r % 4)   # (no more than a float's alignment)
            dev.edit_material_values_device(0, EC.N_MANY, ptr)
            a, b = pack_cases.read_image(host), pack_cases.read_image(dev)
            assert np.array_equal(a, b), f"round {r}: {int((a != b).sum())} bytes differ"
            del t
    finally:
        host.close()
        dev.close()


def test_device_forms_from_first_above_zero_read_n_records():
    """first > 0 and n short of the last record, from a sentinel-guarded buffer: the records outside the range keep
    their values, so a read past n records would show; lights and materials; then the context is the fresh one."""
    s, cam = gs.view("W4_Bunny")
    lights, mats = _value_edit(s)
    nl, nm = len(lights), len(mats)
    assert nl >= 3 and nm >= 3
    c = DeviceContext(DEV)
    try:
        c.upload(s)
        c.render(cam, abi.make_params(W, H))
        lv = np.array([[*l.color, l.intensity] for l in lights[1:nl - 1]], np.float32)
        mv = np.array([[*m.color, m.kd, m.ks, m.exponent, m.metalness, m.roughness] for m in mats[1:nm - 1]], np.float32)
        tl, pl = _guarded(lv, 1)
        tm, pm = _guarded(mv, 3)
        c.edit_light_values_device(1, nl - 2, pl)
        c.edit_material_values_device(1, nm - 2, pm)
        c.synchronize()
        own_l, own_m = EC.lights_of(s), EC.materials_of(s)
        edited = _with(s, own_l[:1] + lights[1:nl - 1] + own_l[nl - 1:], own_m[:1] + mats[1:nm - 1] + own_m[nm - 1:])
        _same(c, edited, cam, "device forms")
        del tl, tm
    finally:
        c.close()


# ---- 4. ordering --------------------------------------------------------------------------------------------------

def test_edits_are_ordered_with_the_frames():
    """render, edit, render, edit back, render with no synchronisation between, on a scene that splits heavy tiles
    (W4_Optional at 256 x 144: the split chain of a frame reads the image on another stream): each frame gathered
    behind its render is the frame of its own scene."""
    w, h = 256, 144
    s, cam = gs.view("W4_Optional")
    lights, mats = _value_edit(s)
    lights[0] = EC.moved(lights[0], EC.MOVE_IN)
    sB = _with(s, lights, mats)
    p = abi.make_params(w, h)
    ref = DeviceContext(DEV)
    c = DeviceContext(DEV)
    out = [np.zeros(w * h, np.uint32) for _ in range(3)]
    try:
        ref.upload(s)
        wantA = ref.render(cam, p, False)[0]
        ref.upload(sB)
        wantB = ref.render(cam, p, False)[0]
        assert not np.array_equal(wantA, wantB)
        for o in out:
            assert c.lib.rtx_host_register(c.h, o.ctypes.data_as(C.c_void_p), o.nbytes) == abi.RTX_OK
        c.upload(s)
        for _ in range(3):   # the measured frame, then frames that split
            c.render(cam, p, False)
        assert c.split_info()[0] > 0, "no heavy tile is split: the case does not reach the split chain"
        own_l, own_m = EC.lights_of(s), EC.materials_of(s)
        c.render_async(cam, p)
        c.gather_async(out[0])
        c.edit_lights(0, lights)
        c.edit_materials(0, mats)
        c.render_async(cam, p)
        c.gather_async(out[1])
        c.edit_lights(0, own_l)
        c.edit_materials(0, own_m)
        c.render_async(cam, p)
        c.gather_async(out[2])
        c.synchronize()
        assert c.split_info()[0] > 0
        for k, want in enumerate((wantA, wantB, wantA)):
            assert np.array_equal(out[k], want), f"frame {k}: {int((out[k] != want).sum())} pixels"
        _same(c, s, cam, "edited back", oracle=False)
    finally:
        for o in out:
            c.lib.rtx_host_unregister(c.h, o.ctypes.data_as(C.c_void_p))
        c.close()
        ref.close()


def test_edits_beside_uploads():
    """An edit followed at once by the upload of a third scene, and an upload followed at once by an edit (the
    upload's copy out of the pinned image still pending): both are the fresh context."""
    s, cam = gs.view("W4_Optional")
    s3, cam3 = gs.view("W4_Bunny")
    lights, mats = _value_edit(s)
    lights[1] = EC.moved(lights[1], EC.MOVE_OUT)
    c = DeviceContext(DEV)
    try:
        c.upload(s)
        c.render_async(cam, abi.make_params(W, H))
        c.edit_lights(0, lights)
        c.upload(s3)
        _same(c, s3, cam3, "edit then upload", oracle=False)
        c.upload(s)
        c.edit_lights(0, lights)
        c.edit_materials(0, mats)
        _same(c, _with(s, lights, mats), cam, "upload then edit", oracle=False)
    finally:
        c.close()


# ---- 5. a payload of several launches -----------------------------------------------------------------------------

def test_all_256_materials():
    s, cam = gs.view("W4_Bunny")
    mats = EC.many_materials(s)
    c = DeviceContext(DEV)
    try:
        c.upload(_with(s, materials=list(mats)))
        c.render(cam, abi.make_params(W, H))
        new = [EC.revalue(m, i) for i, m in enumerate(mats)]
        c.edit_materials(0, new)
        _same(c, _with(s, materials=new), cam, "256 materials")
    finally:
        c.close()


# ---- 6. errors ----------------------------------------------------------------------------------------------------

def test_error_table():
    s, cam = gs.view("W4_Bunny")
    lib = abi.load_hip()
    lights, mats = _value_edit(s)
    nl, nm = len(lights), len(mats)
    L, M = (abi.Light * nl)(*lights), (abi.Material * nm)(*mats)
    p = abi.make_params(W, H)
    c = DeviceContext(DEV)
    try:
        # 1. RTX_E_INVALID: NULL ctx, NULL records with n > 0 (before a scene too)
        for fn, rec in ((lib.rtx_edit_lights, L), (lib.rtx_edit_materials, M)):
            assert fn(None, 0, 1, rec) == abi.RTX_E_INVALID
            assert fn(c.h, 0, 1, None) == abi.RTX_E_INVALID
        for fn in (lib.rtx_edit_light_values_device, lib.rtx_edit_material_values_device):
            assert fn(None, 0, 1, None) == abi.RTX_E_INVALID and fn(c.h, 0, 1, None) == abi.RTX_E_INVALID
        # 2. RTX_E_STATE: no scene
        assert lib.rtx_edit_lights(c.h, 0, 1, L) == abi.RTX_E_STATE
        assert lib.rtx_edit_materials(c.h, 0, 1, M) == abi.RTX_E_STATE
        assert b"no scene" in lib.rtx_last_error(c.h)
        c.upload(s)
        image, frame = pack_cases.read_image(c), c.render(cam, p)
        info = _info(c)
        t, ptr = _guarded(np.zeros(8 * nm, np.float32))

        def unchanged(what):
            assert np.array_equal(pack_cases.read_image(c), image), what
            _frame_eq(c.render(cam, p), frame, what)
            assert _info(c) == info, what

        # first + n above the count, also where the sum overflows 32 bits
        for first, n in ((0, nl + 1), (nl, 1), (1, nl), (2, 0xFFFFFFFF), (0xFFFFFFFF, 2), (0xFFFFFFFF, 0xFFFFFFFF)):
            assert lib.rtx_edit_lights(c.h, first, n, L) == abi.RTX_E_INVALID, (first, n)
            assert lib.rtx_edit_light_values_device(c.h, first, n, ptr) == abi.RTX_E_INVALID, (first, n)
        for first, n in ((0, nm + 1), (nm, 1), (1, nm), (2, 0xFFFFFFFF), (0xFFFFFFFF, 2)):
            assert lib.rtx_edit_materials(c.h, first, n, M) == abi.RTX_E_INVALID, (first, n)
            assert lib.rtx_edit_material_values_device(c.h, first, n, ptr) == abi.RTX_E_INVALID, (first, n)
        unchanged("a range beyond the count")
        # 3. RTX_E_UNSUPPORTED: the LAST record of a range changes its type / kind: nothing of the range is applied
        L[nl - 1].type = 1 - L[nl - 1].type
        assert lib.rtx_edit_lights(c.h, 0, nl, L) == abi.RTX_E_UNSUPPORTED
        assert f"light {nl - 1} ".encode() in lib.rtx_last_error(c.h)
        M[nm - 1].kind = (M[nm - 1].kind + 1) % 4
        assert lib.rtx_edit_materials(c.h, 0, nm, M) == abi.RTX_E_UNSUPPORTED
        assert f"material {nm - 1} ".encode() in lib.rtx_last_error(c.h)
        unchanged("a changed type or kind")
        # n == 0: RTX_OK, nothing launched (records may be NULL, first may be the count)
        assert lib.rtx_edit_lights(c.h, nl, 0, None) == abi.RTX_OK and lib.rtx_edit_materials(c.h, 0, 0, None) == abi.RTX_OK
        assert lib.rtx_edit_light_values_device(c.h, 0, 0, None) == abi.RTX_OK
        assert lib.rtx_edit_material_values_device(c.h, nm, 0, None) == abi.RTX_OK
        unchanged("n == 0")
        # the context keeps working: the legal part of the refused edit
        c.edit_lights(0, lights[:nl - 1])
        _same(c, _with(s, lights[:nl - 1] + EC.lights_of(s)[nl - 1:]), cam, "after the refusals")
        del t
    finally:
        c.close()


def test_a_registered_animation_is_not_edited():
    hs = HostScene("W4_Bunny")
    s, cam = hs.view()
    lights, mats = _value_edit(s)
    L, M = (abi.Light * len(lights))(*lights), (abi.Material * len(mats))(*mats)
    c = DeviceContext(DEV)
    anim = None
    try:
        anim = DeviceAnimation(hs, c)
        for _ in range(2):   # at registration, and after an Update
            image = pack_cases.read_image(c)
            assert c.lib.rtx_edit_lights(c.h, 0, 1, L) == abi.RTX_E_UNSUPPORTED
            assert b"registration" in c.lib.rtx_last_error(c.h)
            assert c.lib.rtx_edit_materials(c.h, 0, 1, M) == abi.RTX_E_UNSUPPORTED
            assert c.lib.rtx_edit_light_values_device(c.h, 0, 1, 4096) == abi.RTX_E_UNSUPPORTED
            assert c.lib.rtx_edit_material_values_device(c.h, 0, 1, 4096) == abi.RTX_E_UNSUPPORTED
            assert np.array_equal(pack_cases.read_image(c), image)
            anim.update(0.7, c)
        anim.close()
        anim = None
        c.upload(s)   # a host upload again: edited
        c.edit_lights(0, lights)
        _same(c, _with(s, lights), cam, "after an upload over the registration", oracle=False)
    finally:
        if anim is not None:
            anim.close()
        c.close()


# ---- 7. the layers above ------------------------------------------------------------------------------------------

def test_renderer_edits_keep_the_uploaded_scene_in_step():
    hs = HostScene("W4_Bunny")
    s, _ = hs.view()
    lights, mats = _value_edit(s)
    lights[2] = EC.moved(lights[2], EC.MOVE_IN)
    r, fresh = Renderer(W, H, device=DEV), Renderer(W, H, device=DEV)
    try:
        before = r.Render(hs).copy()
        r.EditLights(hs, 0, lights)
        r.EditMaterials(hs, 1, mats[1:])
        got = r.Render(hs, upload=False).copy()           # sees the edit without an upload ...
        assert not np.array_equal(got, before)
        assert np.array_equal(got, fresh.Render(hs))      # ... which is the host scene's state now
        assert np.array_equal(pack_cases.read_image(r.ctx), pack_cases.read_image(fresh.ctx))
        assert np.array_equal(r.Render(hs, upload=True), got)
        # the relighting loop through the Renderer: passes, an edit that moves a light, refresh, relight
        r.RenderAOV(hs, AOV_ALL, upload=False)
        r.RenderShadows()
        r.EditLights(hs, 0, [EC.moved(lights[0], EC.MOVE_OUT)])
        with pytest.raises(RuntimeError):
            r.Relight()
        r.RefreshShadows()
        assert np.array_equal(r.Relight(), fresh.Render(hs))
        # a scene that is not the uploaded one: the edit becomes its upload
        other = HostScene("W3")
        so, _ = other.view()
        r.EditLights(other, 0, [EC.recolour(so.lights[0], 0)])
        assert np.array_equal(r.Render(other, upload=False), fresh.Render(other))
        with pytest.raises(ValueError):
            r.EditLights(other, so.n_lights, [so.lights[0]])
    finally:
        r.ctx.close()
        fresh.ctx.close()


def test_cli_in_place_writes_the_same_file(tmp_path):
    assert EXE.exists(), "lib/rtx_render is not built"
    move = ["--move-light", "0,1.5,6,3", "--move-light", "2,8,5,-5"]

    def run(*args):
        return subprocess.run([str(EXE), "W4_Optional", "61", "45", *args], check=True, cwd=tmp_path, timeout=120,
                              capture_output=True, text=True).stdout

    run("--out", "plain.bmp", *move)
    up = run("--out", "upload.bmp", "--relight", *move)
    ed = run("--out", "edit.bmp", "--relight", "--in-place", *move)
    run("--out", "unmoved.bmp", "--relight")
    want = (tmp_path / "upload.bmp").read_bytes()
    assert len(want) == 54 + 4 * 61 * 45 and (tmp_path / "plain.bmp").read_bytes() == want
    assert (tmp_path / "edit.bmp").read_bytes() == want and (tmp_path / "unmoved.bmp").read_bytes() != want
    assert "moved 2 light(s) in place" in ed and "in place" not in up
    assert "light mask 0x5 re-traced" in ed and "light mask 0x5 re-traced" in up
    r = subprocess.run([str(EXE), "W4_Optional", "61", "45", "--in-place"], cwd=tmp_path, capture_output=True, timeout=120)
    assert r.returncode == 2


MIRROR = r"""
#include <cstdio>
#include <stdexcept>
#include "rtx_renderer.hpp"
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); return 1; } } while (0)
template <class F> static bool throws(F f) { try { f(); } catch (const std::runtime_error&) { return true; } return false; }
int main() {
    const int W = 64, H = 48;
    char err[256] = {0};
    rtx_host_scene* hs = nullptr;
    REQUIRE(rtx_host_scene_create("W4_Bunny", nullptr, &hs, err, sizeof err) == RTX_OK);
    rtx::Renderer r(W, H), fresh(W, H);
    rtx_scene s;
    rtx_camera cam;
    REQUIRE(rtx_host_scene_view(hs, &s, &cam) == RTX_OK);
    REQUIRE(throws([&] { r.EditLights(0, {s.lights[0]}); }));            // no scene uploaded
    r.Render(hs, true);
    const std::vector<uint32_t> before = r.Pixels();
    // a value edit of every light and of the materials from 1 on, mirrored into the host scene through its view
    std::vector<rtx_light> lights(s.lights, s.lights + s.n_lights);
    std::vector<rtx_material> mats(s.materials + 1, s.materials + s.n_materials);
    for (size_t i = 0; i < lights.size(); ++i) { lights[i].color[0] = 0.25f + 0.125f * i; lights[i].intensity = 33.f + 7.f * i; }
    for (size_t i = 0; i < mats.size(); ++i) { mats[i].color[1] = 0.5f - 0.0625f * i; mats[i].kd = 0.75f; }
    r.EditLights(0, lights);
    r.EditMaterials(1, mats);
    for (size_t i = 0; i < lights.size(); ++i) const_cast<rtx_light*>(s.lights)[i] = lights[i];
    for (size_t i = 0; i < mats.size(); ++i) const_cast<rtx_material*>(s.materials)[1 + i] = mats[i];
    r.Render(hs, false);
    fresh.Render(hs, true);
    REQUIRE(r.Pixels() == fresh.Pixels() && r.Pixels() != before);
    // the loop for a moved light: edit, refresh, relight
    r.RenderAov(hs, RTX_AOV_ALL, false);
    r.RenderShadows();
    const float to[3] = {4.f, 1.f, 3.f};
    REQUIRE(rtx_host_light_set_origin(hs, 1, to) == RTX_OK);
    r.EditLights(1, {s.lights[1]});
    REQUIRE(throws([&] { r.Relight(); }));                               // shadows on, light 1 moved
    uint32_t traced = 0;
    r.RefreshShadows(&traced);
    REQUIRE(traced == 2u);
    r.Relight();
    fresh.Render(hs, true);
    REQUIRE(r.Pixels() == fresh.Pixels());
    // refusals throw and change nothing
    std::vector<rtx_light> bad(1, s.lights[0]);
    bad[0].type = 1 - bad[0].type;
    REQUIRE(throws([&] { r.EditLights(0, bad); }));
    REQUIRE(throws([&] { r.EditLights(s.n_lights, lights); }));
    std::vector<rtx_material> badm(1, s.materials[0]);
    badm[0].kind = (badm[0].kind + 1) % 4;
    REQUIRE(throws([&] { r.EditMaterials(0, badm); }));
    r.Render(hs, false);
    REQUIRE(r.Pixels() == fresh.Pixels());
    rtx_host_scene_destroy(hs);
    std::puts("mirror ok");
    return 0;
}
"""


def test_cpp_mirror(tmp_path):
    """rtx::Renderer::EditLights / EditMaterials as a compiled program: value edits, the moved-light loop and the
    refusals, against a second renderer that uploads."""
    (tmp_path / "mirror.cpp").write_text(MIRROR)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'include'}", str(tmp_path / "mirror.cpp"),
                    "-o", str(tmp_path / "mirror"), f"-L{LIB}", "-lrtx_hip", "-lrtx_host", f"-Wl,-rpath,{LIB}",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([str(tmp_path / "mirror")], capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert r.returncode == 0 and "mirror ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
