"""Python mirror of dae::Renderer (source/Renderer.h:17-61) over the HIP C-ABI.

    r = Renderer(1920, 1080)            # Renderer(SDL_Window*): width/height of the surface
    r.Render(scene)                     # Renderer::Render(Scene*) -> fills r.buffer (uint32 XRGB)
    r.CycleLightingMode(); r.ToggleShadows(); r.SaveBufferToImage("out.bmp")

Multi-GPU: `Renderer(..., device=rank, stripe=(16, rank, world))` renders only the
16-row stripes this rank owns (rows of stripe s with s % world == rank); stitching the
ranks' buffers gives the single-GPU image bit for bit.

There is no CPU fallback: if librtx_hip.so or the GPU is missing this raises.
"""
from __future__ import annotations

import ctypes as C
import struct
import weakref

import numpy as np

from . import abi
from .scene import HostScene


AOV_DEPTH, AOV_NORMAL, AOV_MATERIAL, AOV_PRIMITIVE, AOV_ALL = (abi.RTX_AOV_DEPTH, abi.RTX_AOV_NORMAL,
                                                                 abi.RTX_AOV_MATERIAL, abi.RTX_AOV_PRIMITIVE,
                                                                 abi.RTX_AOV_ALL)
# plane name -> (mask bit, dtype, elements per pixel), in rtx_aov_planes' order
AOV_PLANES = {"depth": (AOV_DEPTH, np.float32, 1), "normal": (AOV_NORMAL, np.float32, 3),
              "material": (AOV_MATERIAL, np.uint32, 1), "primitive": (AOV_PRIMITIVE, np.uint32, 1)}


def aov_host_planes(width: int, height: int, mask: int, n_views: int = 1) -> dict:
    """Zeroed host planes (flat numpy arrays) for the planes of `mask`."""
    n = int(width) * int(height) * int(n_views)
    return {k: np.zeros(e * n, dt) for k, (bit, dt, e) in AOV_PLANES.items() if mask & bit}


def aov_struct(planes: dict) -> abi.AovPlanes:
    """rtx_aov_planes over a dict of host planes (a missing name = NULL: skipped)."""
    out = abi.AovPlanes()
    for k, (_, dt, _) in AOV_PLANES.items():
        a = planes.get(k)
        if a is not None:
            assert a.dtype == dt and a.flags.c_contiguous, k
            setattr(out, k, a.ctypes.data_as(C.POINTER(C.c_float if dt == np.float32 else C.c_uint32)))
    return out


def _u32p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


class LightingMode:
    ObservedArea, Radiance, BRDF, Combined, Count = 0, 1, 2, 3, 4


class DeviceContext:
    """Owns one rtx_ctx (one GPU) and its uploaded scene."""

    def __init__(self, device: int = 0):
        self.lib = abi.load_hip()
        h = C.c_void_p()
        rc = self.lib.rtx_create(C.byref(h), int(device))
        if rc != abi.RTX_OK:
            why = (self.lib.rtx_last_error(None) or b"").decode(errors="replace")
            raise RuntimeError(f"rtx_create(device={device}) failed with code {rc}: {why or 'no usable HIP device?'}")
        self.h = h
        self.device = device
        self._uploaded = None
        self._aov_shape = None   # (width, height, views) of the last hit pass queued through this object

    def close(self):
        if getattr(self, "h", None):
            self.lib.rtx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, name: str, *args) -> None:
        """Entry point `name` on this context; anything but RTX_OK raises with the context's last error."""
        abi.check(getattr(self.lib, name)(self.h, *args), name, self.h)

    def _timed(self, name: str, iters: int, *args) -> float:
        """An rtx_time_* entry point, whose last two arguments are `iters` and the mean's address: the mean in ms."""
        ms = C.c_float()
        self._call(name, *args, int(iters), C.byref(ms))
        return ms.value

    @staticmethod
    def _pixels(n: int, want_rgb: bool, px: np.ndarray | None = None):
        """The outputs of a frame of n pixels, (px, rgb, their pointers): `px` or a zeroed uint32[n], and a zeroed
        float32[3n] or, without want_rgb, None and NULL."""
        if px is None:
            px = np.zeros(n, np.uint32)
        rgb = np.zeros(3 * n, np.float32) if want_rgb else None
        return px, rgb, _u32p(px), rgb.ctypes.data_as(C.POINTER(C.c_float)) if want_rgb else None

    def _frame(self, name: str, n: int, want_rgb: bool, *args, px: np.ndarray | None = None):
        """A blocking frame of n pixels by entry point `name`, whose last two arguments are the outputs: (px, rgb)."""
        px, rgb, pxp, rgbp = self._pixels(n, want_rgb, px)
        self._call(name, *args, pxp, rgbp)
        return px, rgb

    def upload(self, scene: abi.Scene) -> None:
        self._call("rtx_upload_scene", C.byref(scene))

    def set_supersample(self, k: int) -> None:
        """k x k samples per pixel (1, 2, 4 or 8) for every later frame (rtx_set_supersample)."""
        self._call("rtx_set_supersample", int(k))

    def render(self, cam: abi.Camera, params: abi.RenderParams, want_rgb: bool = True):
        return self._frame("rtx_render", params.width * params.height, want_rgb, C.byref(cam), C.byref(params))

    def render_adaptive(self, cam: abi.Camera, params: abi.RenderParams, k: int, threshold: int,
                        want_rgb: bool = True):
        """Adaptive supersampling (rtx_render_adaptive), blocking: the plain frame with k x k samples
        (k = 2, 4, 8) for the pixels that differ from a 4-neighbour by more than `threshold` (0..255) in a
        channel; (pixels, rgb) like render()."""
        return self._frame("rtx_render_adaptive", params.width * params.height, want_rgb, C.byref(cam),
                           C.byref(params), int(k), int(threshold))

    def render_adaptive_async(self, cam, params, k: int, threshold: int, want_rgb: bool = False) -> None:
        self._call("rtx_render_adaptive_async", C.byref(cam), C.byref(params), int(want_rgb), int(k), int(threshold))

    def adaptive_refined(self) -> int:
        """The pixels the last adaptive frame refined (rtx_adaptive_refined; waits for the stream)."""
        n = C.c_uint32()
        self._call("rtx_adaptive_refined", C.byref(n))
        return n.value

    def time_adaptive_frames(self, cam, params, k: int, threshold: int, iters: int) -> float:
        return self._timed("rtx_time_adaptive_frames", iters, C.byref(cam), C.byref(params), int(k), int(threshold))

    def render_async(self, cam, params, want_rgb=False):
        self._call("rtx_render_async", C.byref(cam), C.byref(params), int(want_rgb))

    def synchronize(self):
        self._call("rtx_synchronize")

    def gather_async(self, out_px: np.ndarray, out_rgb: np.ndarray | None = None) -> None:
        """Queue the D2H copy of the rows the last render owns into full-frame host arrays
        (rtx_gather_async); complete after synchronize()."""
        assert out_px.dtype == np.uint32 and out_px.flags.c_contiguous
        rgbp = None
        if out_rgb is not None:
            assert out_rgb.dtype == np.float32 and out_rgb.flags.c_contiguous
            rgbp = out_rgb.ctypes.data_as(C.POINTER(C.c_float))
        self._call("rtx_gather_async", _u32p(out_px), rgbp)

    def render_aov(self, cam: abi.Camera, params: abi.RenderParams, mask: int = AOV_ALL) -> dict:
        """The hit pass (rtx_render_aov), blocking: {"depth", "normal", "material", "primitive"} ->
        flat numpy planes, those of `mask` (include/rtx.h gives their values)."""
        planes = aov_host_planes(params.width, params.height, mask)
        out = aov_struct(planes)
        self._call("rtx_render_aov", C.byref(cam), C.byref(params), int(mask), C.byref(out))
        self._aov_shape = (params.width, params.height, 1)
        return planes

    def render_aov_async(self, cams, params: abi.RenderParams, mask: int = AOV_ALL) -> None:
        """Queue the hit pass of one camera or a sequence of up to 8 (rtx_render_aov_async)."""
        if isinstance(cams, abi.Camera):
            cams = [cams]
        arr = (abi.Camera * len(cams))(*cams)
        self._call("rtx_render_aov_async", arr, len(cams), C.byref(params), int(mask))
        self._aov_shape = (params.width, params.height, len(cams))

    def gather_aov_async(self, planes: dict) -> None:
        """Queue the D2H copy of the rows the last hit pass owns into full-frame host planes
        (rtx_gather_aov_async); complete after synchronize()."""
        out = aov_struct(planes)
        self._call("rtx_gather_aov_async", C.byref(out))

    def download_aov(self, planes: dict) -> dict:
        """Copy the last hit pass's owned rows into `planes` and wait (rtx_download_aov)."""
        out = aov_struct(planes)
        self._call("rtx_download_aov", C.byref(out))
        return planes

    def device_aov_buffers(self) -> dict:
        """Device addresses of the HBM planes (0 for a plane no mask has named yet)."""
        out = abi.AovPlanes()
        self._call("rtx_device_aov_buffers", C.byref(out))
        return {k: C.cast(getattr(out, k), C.c_void_p).value or 0 for k in AOV_PLANES}

    def device_buffers(self) -> tuple[int, int]:
        """Device addresses (d_px, d_rgb) of the colour frame buffer (rtx_device_buffers; 0 for a plane
        no frame has asked for yet).  A larger frame reallocates them: fetch them afresh."""
        px, rgb = C.c_void_p(), C.c_void_p()
        self._call("rtx_device_buffers", C.byref(px), C.byref(rgb))
        return px.value or 0, rgb.value or 0

    @staticmethod
    def _rays(rays) -> np.ndarray:
        """(n, 8) float32 rows {origin, direction, tmin, tmax} (rtx_ray), C-contiguous."""
        a = np.ascontiguousarray(rays, np.float32)
        if a.ndim != 2 or a.shape[1] != 8:
            raise ValueError(f"rays must be (n, 8) float32 rows of origin, direction, tmin, tmax; got {a.shape}")
        return a

    def trace_rays(self, rays, mask: int = AOV_ALL) -> dict:
        """Scene::GetClosestHit on caller-supplied rays (rtx_trace_rays), blocking: the planes of `mask`,
        keyed as render_aov's, element i = ray i's record.  Nothing about a ray is interpreted: the
        direction is not normalised and nothing is validated (include/rtx.h)."""
        a = self._rays(rays)
        n = a.shape[0]
        planes = {k: np.zeros(e * n, dt) for k, (bit, dt, e) in AOV_PLANES.items() if mask & bit}
        out = aov_struct(planes)
        self._call("rtx_trace_rays", a.ctypes.data_as(C.POINTER(abi.Ray)), n, int(mask), C.byref(out))
        return planes

    def occluded(self, rays) -> np.ndarray:
        """Scene::DoesHit on caller-supplied rays (rtx_occluded), blocking: uint8[n], 1 = something lies
        in the ray's [tmin, tmax]."""
        a = self._rays(rays)
        n = a.shape[0]
        out = np.zeros(n, np.uint8)
        self._call("rtx_occluded", a.ctypes.data_as(C.POINTER(abi.Ray)), n, out.ctypes.data_as(C.POINTER(C.c_uint8)))
        return out

    def trace_rays_device(self, d_rays: int, n: int, mask: int, d_planes: dict) -> None:
        """rtx_trace_rays_device: `d_rays` and the values of `d_planes` (plane name -> address, a missing
        name or 0 = not asked for) are device addresses; queued, complete after synchronize()."""
        out = abi.AovPlanes()
        for k, (_, dt, _) in AOV_PLANES.items():
            if d_planes.get(k):
                setattr(out, k, C.cast(C.c_void_p(int(d_planes[k])),
                                       C.POINTER(C.c_float if dt == np.float32 else C.c_uint32)))
        self._call("rtx_trace_rays_device", C.c_void_p(int(d_rays)), int(n), int(mask), C.byref(out))

    def occluded_device(self, d_rays: int, n: int, d_out: int) -> None:
        """rtx_occluded_device: device addresses; queued, complete after synchronize()."""
        self._call("rtx_occluded_device", C.c_void_p(int(d_rays)), int(n), C.c_void_p(int(d_out)))

    def shade_rays(self, rays, params: abi.RenderParams):
        """Renderer::RenderPixel from GetClosestHit on for caller-supplied rays (rtx_shade_rays), blocking:
        (pixels uint32[n], rgb float32[3n]), element i = ray i's.  `params` supplies the lighting mode,
        shadows and pixel format; its frame size is ignored.  Nothing about a ray is interpreted and Shade
        receives -direction as given (include/rtx.h)."""
        a = self._rays(rays)
        n = a.shape[0]
        return self._frame("rtx_shade_rays", n, True, a.ctypes.data_as(C.POINTER(abi.Ray)), n, C.byref(params))

    def shade_rays_device(self, d_rays: int, n: int, params: abi.RenderParams, d_pixels: int = 0, d_rgb: int = 0) -> None:
        """rtx_shade_rays_device: device addresses (0 = that output is not asked for); queued, complete
        after synchronize()."""
        self._call("rtx_shade_rays_device", C.c_void_p(int(d_rays)), int(n), C.byref(params),
                   C.c_void_p(int(d_pixels) or None), C.c_void_p(int(d_rgb) or None))

    def time_shade_rays(self, d_rays: int, n: int, params: abi.RenderParams, d_pixels: int, d_rgb: int,
                        iters: int) -> float:
        return self._timed("rtx_time_shade_rays", iters, C.c_void_p(int(d_rays)), int(n), C.byref(params),
                           C.c_void_p(int(d_pixels) or None), C.c_void_p(int(d_rgb) or None))

    def time_aov_frames(self, cam, params, mask: int, iters: int) -> float:
        ms = self._timed("rtx_time_aov_frames", iters, C.byref(cam), C.byref(params), int(mask))
        self._aov_shape = (params.width, params.height, 1)
        return ms

    def shade_aov_async(self, params: abi.RenderParams, want_rgb: bool = False) -> None:
        """Queue deferred shading of the last hit pass into the colour frame buffer (rtx_shade_aov_async):
        `params` supplies the lighting mode, shadows and pixel format, the pass everything else."""
        self._call("rtx_shade_aov_async", C.byref(params), int(want_rgb))

    def shade_aov(self, params: abi.RenderParams, want_rgb: bool = True):
        """Deferred shading of the last hit pass (rtx_shade_aov), blocking: (pixels, rgb) like render(), of
        the pass's size (every view of a multi-view pass, one after the other; rows a striped pass does
        not own stay zero)."""
        if self._aov_shape is None:   # no pass through this object: the library says why
            self.shade_aov_async(params, want_rgb)
        return self._frame("rtx_shade_aov", self._pass_pixels("shade_aov"), want_rgb, C.byref(params))

    def time_shade_aov(self, params: abi.RenderParams, want_rgb: bool, iters: int) -> float:
        return self._timed("rtx_time_shade_aov", iters, C.byref(params), int(want_rgb))

    def _pass_pixels(self, what: str) -> int:
        if self._aov_shape is None:
            raise RuntimeError(f"{what}: the last hit pass was not queued through this object, its size is unknown")
        return self._aov_shape[0] * self._aov_shape[1] * self._aov_shape[2]

    def render_shadows_async(self) -> None:
        """Queue the shadow pass of the last hit pass (rtx_render_shadows_async): per pixel one word whose bit
        l says that light l of the uploaded scene is occluded, kept in HBM for relight()."""
        self._call("rtx_render_shadows_async")

    def update_shadows_async(self, lights: int) -> None:
        """Queue the shadow pass for the lights named in `lights` only (bit l = light l) and merge their bits
        into the plane (rtx_update_shadows_async); every other light must be where the plane recorded it."""
        self._call("rtx_update_shadows_async", int(lights) & 0xFFFFFFFF)

    def refresh_shadows_async(self) -> int:
        """Make the plane valid for the uploaded lights at the least cost (rtx_refresh_shadows_async): the
        full pass without a current plane, else one launch over the lights that changed.  Returns the mask
        of the lights traced (0: nothing was launched, or only removed lights' bits were cleared)."""
        traced = C.c_uint32()
        self._call("rtx_refresh_shadows_async", C.byref(traced))
        return traced.value

    def download_shadows(self, out: np.ndarray | None = None) -> np.ndarray:
        """Copy the shadow plane's owned rows into a full-frame uint32 array and wait (rtx_download_shadows);
        rows the pass does not own keep what `out` held (zero in a new array)."""
        if out is None:
            out = np.zeros(self._pass_pixels("download_shadows"), np.uint32)
        self._call("rtx_download_shadows", _u32p(out))
        return out

    def gather_shadows_async(self, out: np.ndarray) -> None:
        self._call("rtx_gather_shadows_async", _u32p(out))

    def device_shadow_buffer(self) -> int:
        """Device address of the shadow plane (0 before the first shadow pass)."""
        d = C.POINTER(C.c_uint32)()
        self._call("rtx_device_shadow_buffer", C.byref(d))
        return C.cast(d, C.c_void_p).value or 0

    # ---- scene edits (rtx_edit_*): light and material records of the current image replaced in place
    @staticmethod
    def _records(records, kind):
        """`records` as a ctypes array of `kind` (a ctypes array of it passes through; else a sequence of them)."""
        if isinstance(records, C.Array) and records._type_ is kind:
            return records
        recs = list(records)
        return (kind * len(recs))(*recs)

    def edit_lights(self, first: int, lights) -> None:
        """Lights first .. first+len-1 of the uploaded scene take the given origin, color and intensity, in
        place and queued (rtx_edit_lights); the types must be the uploaded ones.  After a light moved, relight()
        with shadows needs update_shadows_async or refresh_shadows_async first, as after an upload."""
        arr = self._records(lights, abi.Light)
        self._call("rtx_edit_lights", int(first), len(arr), arr)

    def edit_materials(self, first: int, materials) -> None:
        """Materials first .. first+len-1 take the given values in place (rtx_edit_materials); kinds as uploaded."""
        arr = self._records(materials, abi.Material)
        self._call("rtx_edit_materials", int(first), len(arr), arr)

    def edit_light_values_device(self, first: int, n: int, d_ptr: int) -> None:
        """The colour and intensity of lights first .. first+n-1 from device memory: 4 floats a light, {color[3],
        intensity}, at device address `d_ptr` (rtx_edit_light_values_device).  Queued: the memory stays valid
        until the context's stream has passed the edit."""
        self._call("rtx_edit_light_values_device", int(first), int(n), int(d_ptr) or None)

    def edit_material_values_device(self, first: int, n: int, d_ptr: int) -> None:
        """The values of materials first .. first+n-1 from device memory: 8 floats a material, {color[3], kd, ks,
        exponent, metalness, roughness} (rtx_edit_material_values_device); the Lambert term is computed on the
        device, bit for bit the host form's."""
        self._call("rtx_edit_material_values_device", int(first), int(n), int(d_ptr) or None)

    def relight_async(self, params: abi.RenderParams, want_rgb: bool = False) -> None:
        """Queue the relight of the last hit pass into the colour frame buffer (rtx_relight_async): `params`
        supplies the lighting mode, shadows and pixel format; with shadows the shadow plane answers DoesHit."""
        self._call("rtx_relight_async", C.byref(params), int(want_rgb))

    def relight(self, params: abi.RenderParams, want_rgb: bool = True):
        """The relight (rtx_relight), blocking: (pixels, rgb) like shade_aov()."""
        if self._aov_shape is None:   # no pass through this object: the library says why
            self.relight_async(params, want_rgb)
        return self._frame("rtx_relight", self._pass_pixels("relight"), want_rgb, C.byref(params))

    def relight_resolve_async(self, params: abi.RenderParams, k: int, want_rgb: bool = False) -> None:
        """Queue the resolved relight (rtx_relight_resolve_async): the last hit pass of k*W x k*H is read as the
        sample frame of a W x H frame, every sample is relit and each pixel's k x k samples are box-filtered as
        rtx_set_supersample(k) defines; the frame buffer then holds the W x H frame."""
        self._call("rtx_relight_resolve_async", C.byref(params), int(k), int(want_rgb))

    def relight_resolve(self, params: abi.RenderParams, k: int, want_rgb: bool = True):
        """The resolved relight (rtx_relight_resolve), blocking: (pixels, rgb) of W*H*views pixels."""
        if self._aov_shape is None or k not in (2, 4, 8):   # no array can be sized: the library says why
            self.relight_resolve_async(params, k, want_rgb)
            # (accepted: a pass queued behind this object's back; the frame is in the frame buffer, unsized here)
            raise RuntimeError("relight_resolve: the last hit pass was not queued through this object, its size is "
                               "unknown")
        n = (self._aov_shape[0] // k) * (self._aov_shape[1] // k) * self._aov_shape[2]
        return self._frame("rtx_relight_resolve", n, want_rgb, C.byref(params), int(k))

    def time_relight_resolve(self, params: abi.RenderParams, k: int, want_rgb: bool, iters: int) -> float:
        return self._timed("rtx_time_relight_resolve", iters, C.byref(params), int(k), int(want_rgb))

    def time_shadows(self, iters: int) -> float:
        return self._timed("rtx_time_shadows", iters)

    def time_shadows_update(self, lights: int, iters: int) -> float:
        return self._timed("rtx_time_shadows_update", iters, int(lights) & 0xFFFFFFFF)

    def time_relight(self, params: abi.RenderParams, want_rgb: bool, iters: int) -> float:
        return self._timed("rtx_time_relight", iters, C.byref(params), int(want_rgb))

    def time_frames(self, cam, params, iters: int) -> float:
        return self._timed("rtx_time_frames", iters, C.byref(cam), C.byref(params))

    def split_info(self) -> tuple[int, int]:
        """(heavy tiles the next frame splits, BVH frontier parts of the scene)."""
        h, p = C.c_uint32(), C.c_uint32()
        self._call("rtx_split_info", C.byref(h), C.byref(p))
        return h.value, p.value

    def schedule_state(self, n: int):
        """(order, cost) of the first n tiles after a measured frame (rtx_schedule_state): the dispatch
        permutation and the one-piece tile costs it was sorted by."""
        order, cost, tiles = np.zeros(n, np.uint32), np.zeros(n, np.uint32), C.c_uint32()
        self._call("rtx_schedule_state", _u32p(order), _u32p(cost), int(n), C.byref(tiles))
        if tiles.value < n:
            raise RuntimeError(f"rtx_schedule_state: the schedule holds {tiles.value} tiles, {n} asked for")
        return order, cost

    def schedule_heavy(self, n: int) -> dict:
        """What the last measured frame selected (rtx_schedule_heavy): the heavy flags of the first n tiles,
        the heavy list, the four counter words, the threshold and the scalars the update ran with."""
        flag, lst = np.zeros(n, np.uint32), np.zeros(abi.MAX_HEAVY_TILES, np.uint32)
        hn, thr, par = (C.c_uint32 * 4)(), C.c_uint64(), (C.c_uint32 * 4)()
        self._call("rtx_schedule_heavy", _u32p(flag), int(n), _u32p(lst), hn, C.byref(thr), par)
        return {"heavy_flag": flag, "heavy_list": lst, "heavy_n": [int(v) for v in hn], "threshold": thr.value,
                "split_slots": par[0], "permille": par[1], "split_min": par[2], "wave_slots": par[3]}

    def schedule_run(self, cost, saved, was_heavy=None, *, tiles_x: int, tiles_y: int, parts: int = 0,
                     split_slots: int, permille: int, split_min: int, wave_slots: int, xcd: bool = False) -> dict:
        """The schedule kernels on given costs (rtx_schedule_run): uint32 arrays of n tiles in, the order, the
        XCD order when asked for, costs and saved costs afterwards, heavy flags, list, counter words and
        threshold out.  Nothing of the context's own schedule is touched."""
        cost, saved = np.ascontiguousarray(cost, np.uint32), np.ascontiguousarray(saved, np.uint32)
        n = cost.size
        if was_heavy is not None:
            was_heavy = np.ascontiguousarray(was_heavy, np.uint32)
        if saved.size != n or (was_heavy is not None and was_heavy.size != n):
            raise ValueError("cost, saved and was_heavy must have one word per tile")
        case = abi.ScheduleCase(_u32p(cost), _u32p(was_heavy) if was_heavy is not None else None, _u32p(saved), n,
                                int(tiles_x), int(tiles_y), int(parts), int(split_slots), int(permille),
                                int(split_min), int(wave_slots), int(bool(xcd)))
        out = {k: np.zeros(n, np.uint32) for k in ("order", "cost_after", "saved_after", "heavy_flag")}
        out["order_xcd"] = np.zeros(n, np.uint32) if xcd else None
        out["heavy_list"] = np.zeros(abi.MAX_HEAVY_TILES, np.uint32)
        res = abi.ScheduleResult(_u32p(out["order"]), _u32p(out["order_xcd"]) if xcd else None,
                                 _u32p(out["cost_after"]), _u32p(out["saved_after"]), _u32p(out["heavy_flag"]),
                                 _u32p(out["heavy_list"]))
        self._call("rtx_schedule_run", C.byref(case), C.byref(res))
        out["heavy_n"] = [int(v) for v in res.heavy_n]
        out["threshold"] = int(res.threshold)
        return out

    def split_tune_info(self) -> dict:
        """The split threshold's tuner: factor, last timed main kernel / split chain (ms), state."""
        f, m, ch, d = C.c_float(), C.c_float(), C.c_float(), C.c_uint32()
        self._call("rtx_split_tune_info", C.byref(f), C.byref(m), C.byref(ch), C.byref(d))
        return {"factor": round(f.value, 4), "main_ms": round(m.value, 5), "chain_ms": round(ch.value, 5),
                "state": ["tuning", "converged", "off"][d.value]}

    def inflight_info(self) -> dict:
        """Frames in flight: the last frame saw another context's frame in flight / rendered one piece
        for it; the heaviest tile's serialized time over the split frame's serialized span, the
        threshold, and the split frames' interval in flight on this context's stream (ms)."""
        a, b, r, t, w = C.c_uint32(), C.c_uint32(), C.c_float(), C.c_float(), C.c_float()
        self._call("rtx_inflight_info", C.byref(a), C.byref(b), C.byref(r), C.byref(t), C.byref(w))
        return {"concurrent": bool(a.value), "onepiece": bool(b.value), "crit": round(r.value, 3),
                "threshold": round(t.value, 3), "split_interval_ms": round(w.value, 5)}

    def light_major_info(self) -> tuple[bool, int]:
        """(the last prepared frame was light-major, the largest light-major launch in wave tiles)."""
        a, b = C.c_uint32(), C.c_uint32()
        self._call("rtx_light_major_info", C.byref(a), C.byref(b))
        return bool(a.value), int(b.value)

    def cull_info(self) -> tuple[bool, int]:
        """(the uploaded scene renders with the exact cull, camera-record rebuilds so far)."""
        on, n = C.c_uint32(), C.c_uint64()
        self._call("rtx_cull_info", C.byref(on), C.byref(n))
        return bool(on.value), n.value

    def spec_info(self) -> tuple[int, int]:
        """(kSpec* facts of the last frame launched, the kSpecVariants index it took: -1 = generic)."""
        f, v = C.c_uint32(), C.c_int32()
        self._call("rtx_spec_info", C.byref(f), C.byref(v))
        return f.value, v.value

    def room_info(self) -> tuple[bool, float]:
        """(the uploaded scene's room-skip fact, room_M: the bound on a shadow origin's plane distances)."""
        f, m = C.c_uint32(), C.c_float()
        self._call("rtx_room_info", C.byref(f), C.byref(m))
        return bool(f.value), float(m.value)

    def count_work(self, cam, params) -> np.ndarray:
        out = (C.c_uint64 * 12)()
        self._call("rtx_count_work", C.byref(cam), C.byref(params), out)
        return np.array(list(out), dtype=np.uint64)

    def count_work_culled(self, cam, params) -> np.ndarray:
        """The 15 counters of the walk the product executes (rtx_count_work_culled): the 12 model
        counters, per-wave node-pair and triangle steps, exact-cull box tests."""
        out = (C.c_uint64 * 15)()
        self._call("rtx_count_work_culled", C.byref(cam), C.byref(params), out, 15)
        return np.array(list(out), dtype=np.uint64)


class DeviceGroup:
    """Owns one rtx_group: one frame tiled over several contexts (GPUs) by this process,
    each member with its own host thread and stream gathering its 16-row stripes into
    one host frame (include/rtx.h)."""

    def __init__(self, devices):
        self.lib = abi.load_hip()
        ids = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        rc = self.lib.rtx_group_create(C.byref(h), ids, len(devices))
        if rc != abi.RTX_OK:
            why = (self.lib.rtx_group_last_error(None) or b"").decode(errors="replace")
            raise RuntimeError(f"rtx_group_create({list(devices)}) failed with code {rc}: {why}")
        self.h = h
        self.devices = list(devices)

    def _check(self, rc, what):
        if rc != abi.RTX_OK:
            why = (self.lib.rtx_group_last_error(self.h) or b"").decode(errors="replace")
            raise RuntimeError(f"{what} failed with code {rc}: {why}")

    def close(self):
        if getattr(self, "h", None):
            self.lib.rtx_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, scene: abi.Scene) -> None:
        self._check(self.lib.rtx_group_upload_scene(self.h, C.byref(scene)), "rtx_group_upload_scene")

    def set_supersample(self, k: int) -> None:
        """k x k samples per pixel (1, 2, 4 or 8) on every member (rtx_group_set_supersample)."""
        self._check(self.lib.rtx_group_set_supersample(self.h, int(k)), "rtx_group_set_supersample")

    def render(self, cam: abi.Camera, params: abi.RenderParams, want_rgb: bool = True, out_px=None):
        n = params.width * params.height
        px = np.zeros(n, np.uint32) if out_px is None else out_px
        rgb = np.zeros(3 * n, np.float32) if want_rgb else None
        rc = self.lib.rtx_group_render(self.h, C.byref(cam), C.byref(params),
                                       px.ctypes.data_as(C.POINTER(C.c_uint32)),
                                       rgb.ctypes.data_as(C.POINTER(C.c_float)) if want_rgb else None)
        self._check(rc, "rtx_group_render")
        return px, rgb

    def render_aov(self, cam: abi.Camera, params: abi.RenderParams, mask: int = AOV_ALL) -> dict:
        """The hit pass over the members' stripes (rtx_group_render_aov): the planes of `mask`."""
        planes = aov_host_planes(params.width, params.height, mask)
        out = aov_struct(planes)
        self._check(self.lib.rtx_group_render_aov(self.h, C.byref(cam), C.byref(params), int(mask), C.byref(out)),
                    "rtx_group_render_aov")
        return planes


class DeviceAnimation:
    """Owns one rtx_anim: Scene::Update of a host scene's turning meshes done on the device
    (transform, the reference's binned-SAH rebuild, scene image) — SURVEY §8(f)1.
    `DeviceAnimation(scene, ctx)` registers the scene's current state and uploads it to
    `ctx`; `update(t, ctx)` queues Update(t) into `ctx`'s scene image."""

    def __init__(self, scene, ctx: DeviceContext):
        self.lib = abi.load_hip()
        self.scene = scene
        ids = scene.spinning()
        if not ids:
            raise ValueError(f"scene {scene.name!r} has no turning mesh")
        s, _ = scene.view()
        srcs = (abi.MeshSource * len(ids))(*[scene.mesh_source(i) for i in ids])
        cids = (C.c_int32 * len(ids))(*ids)
        h = C.c_void_p()
        rc = self.lib.rtx_anim_create(C.byref(h), ctx.h, C.byref(s), cids, srcs, len(ids))
        if rc != abi.RTX_OK:
            why = (self.lib.rtx_anim_last_error(None) or b"").decode(errors="replace")
            raise RuntimeError(f"rtx_anim_create failed with code {rc}: {why}")
        self.h = h
        self.mesh_ids = list(ids)
        self.n_tris = [s.meshes[i].n_indices // 3 for i in ids]
        self.n_positions = [s.meshes[i].n_positions for i in ids]

    def _check(self, rc, what):
        if rc != abi.RTX_OK:
            why = (self.lib.rtx_anim_last_error(self.h) or b"").decode(errors="replace")
            raise RuntimeError(f"{what} failed with code {rc}: {why}")

    def close(self):
        if getattr(self, "h", None):
            self.lib.rtx_anim_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def update(self, total_time: float, ctx: DeviceContext) -> None:
        m = self.scene.transforms(total_time)
        self._check(self.lib.rtx_anim_update(self.h, ctx.h, m.ctypes.data_as(C.POINTER(C.c_float))),
                    "rtx_anim_update")

    def status(self, i: int = 0) -> np.ndarray:
        st = (C.c_uint32 * 4)()
        self._check(self.lib.rtx_anim_status(self.h, i, st), "rtx_anim_status")
        return np.array(list(st), np.uint32)

    def stamps(self, i: int = 0) -> np.ndarray:
        """The last update's 128 status words of registered mesh i (rtx_anim.h: errors, counts,
        phase stamps, completeness word 28); no error check."""
        out = (C.c_uint32 * 128)()
        self._check(self.lib.rtx_anim_stamps(self.h, i, out), "rtx_anim_stamps")
        return np.array(list(out), np.uint32)

    def download(self, i: int = 0) -> dict:
        """Registered mesh i in the reference's form (TriangleMesh after UpdateTransforms)."""
        T, V = self.n_tris[i], self.n_positions[i]
        pos = np.zeros(3 * V, np.float32)
        idx = np.zeros(3 * T, np.int32)
        nrm = np.zeros(3 * T, np.float32)
        tn = np.zeros(3 * T, np.float32)
        nodes = (abi.BVHNode * (3 * T))()
        f = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
        self._check(self.lib.rtx_anim_download(self.h, i, f(pos), idx.ctypes.data_as(C.POINTER(C.c_int32)), f(nrm),
                                               f(tn), nodes), "rtx_anim_download")
        raw = np.ctypeslib.as_array(C.cast(nodes, C.POINTER(C.c_uint32)), shape=(3 * T * 9,)).copy().reshape(-1, 9)
        return {"tpositions": pos, "indices": idx, "normals": nrm, "tnormals": tn, "nodes": raw}


class Renderer:
    def __init__(self, width: int, height: int, device: int = 0, stripe: tuple[int, int, int] | None = None,
                 pixel_format=abi.XRGB8888, supersample: int = 1, adaptive: tuple[int, int] | None = None):
        self.m_Width, self.m_Height = int(width), int(height)
        self.m_AspectRatio = self.m_Width / float(self.m_Height)
        self.m_CurrentLightingMode = LightingMode.Combined
        self.m_ShadowsEnabled = True
        self.stripe = stripe
        self.format = pixel_format
        self.ctx = DeviceContext(device)
        if supersample != 1:
            self.ctx.set_supersample(supersample)
        self.supersample = int(supersample)
        # (k, threshold): Render takes k x k samples for the pixels that alias only (RenderAdaptive)
        self.adaptive = (int(adaptive[0]), int(adaptive[1])) if adaptive is not None else None
        self._scene_ref = None   # weakref to the uploaded HostScene
        self._scene_gen = -1      # its generation at upload
        self.buffer = np.zeros(self.m_Width * self.m_Height, np.uint32)
        self.rgb = None

    def params(self) -> abi.RenderParams:
        sr, first, step = self.stripe if self.stripe else (0, 0, 1)
        return abi.make_params(self.m_Width, self.m_Height, self.m_CurrentLightingMode, self.m_ShadowsEnabled,
                               self.format, sr, first, step)

    def _view(self, scene: HostScene, upload: bool):
        """The scene's flattened view and camera, uploaded when asked to or when it is not the
        uploaded scene's current state."""
        s, cam = scene.view()
        same = self._scene_ref is not None and self._scene_ref() is scene and self._scene_gen == scene.generation
        if upload or not same:
            self.ctx.upload(s)
            self._scene_ref = weakref.ref(scene)
            self._scene_gen = scene.generation
        return s, cam

    def _edit(self, scene: HostScene, first: int, records, which: str) -> None:
        """Write `records` over the host scene's own from `first` on (type and kind stay the scene's), and
        bring the device in step: in place when `scene` in this state is the uploaded one, else by an upload."""
        s, _ = scene.view()
        own, count = (s.lights, s.n_lights) if which == "lights" else (s.materials, s.n_materials)
        records = list(records)
        if first < 0 or first + len(records) > count:
            raise ValueError(f"Edit: {which} {first} .. {first + len(records) - 1} of {count}")
        same = self._scene_ref is not None and self._scene_ref() is scene and self._scene_gen == scene.generation
        for i, r in enumerate(records):
            if which == "lights":
                own[first + i].origin[:] = list(r.origin)
                own[first + i].color[:] = list(r.color)
                own[first + i].intensity = r.intensity
            else:
                kind = own[first + i].kind
                C.memmove(C.byref(own[first + i]), C.byref(r), C.sizeof(abi.Material))
                own[first + i].kind = kind
        if not same:
            self._view(scene, True)
        elif which == "lights":
            self.ctx.edit_lights(first, [own[first + i] for i in range(len(records))])
        else:
            self.ctx.edit_materials(first, [own[first + i] for i in range(len(records))])

    def EditLights(self, scene: HostScene, first: int, lights) -> None:
        """Lights first .. of `scene` take the origin, color and intensity of `lights` (abi.Light records), in
        the host scene and, without an upload, in the uploaded one (rtx_edit_lights; not in the reference's
        Renderer): a later call with upload=False sees the edit, one with upload=True uploads the same scene.
        After a moved light, RefreshShadows before Relight, as after an upload."""
        self._edit(scene, int(first), lights, "lights")

    def EditMaterials(self, scene: HostScene, first: int, materials) -> None:
        """Materials first .. of `scene` take the values of `materials` (abi.Material records; kinds stay), as
        EditLights does for lights (rtx_edit_materials)."""
        self._edit(scene, int(first), materials, "materials")

    def _fill(self, name: str, want_rgb: bool, *args) -> np.ndarray:
        """The blocking frame of entry point `name` into self.buffer (and self.rgb): self.buffer."""
        _, self.rgb = self.ctx._frame(name, self.m_Width * self.m_Height, want_rgb, *args, px=self.buffer)
        return self.buffer

    def RenderAOV(self, scene: HostScene, mask: int = AOV_ALL, upload: bool = True) -> dict:
        """The hit pass of the frame Render would render (same size, stripes and upload bookkeeping):
        the planes of `mask` as flat numpy arrays; rows this renderer's stripes do not own stay 0."""
        _, cam = self._view(scene, upload)
        return self.ctx.render_aov(cam, self.params(), mask)

    def ShadeAOV(self, want_rgb: bool = False) -> np.ndarray:
        """Deferred shading (rtx_shade_aov; not in the reference's Renderer): the frame Render would
        render, shaded from the last RenderAOV's planes (all four) with the renderer's CURRENT lighting
        mode, shadows and pixel format, without tracing a primary ray.  Explicit: nothing is cached or
        reused automatically, and the scene is whatever was uploaded last.  Blocking; fills self.buffer."""
        self._own_pass("ShadeAOV", lambda: self.ctx.shade_aov_async(self.params(), want_rgb))
        return self._fill("rtx_shade_aov", want_rgb, C.byref(self.params()))

    def _own_pass(self, what: str, probe) -> None:
        if self.ctx._aov_shape != (self.m_Width, self.m_Height, 1):
            if self.ctx._aov_shape is None:
                probe()   # no pass yet: the library says why
            raise RuntimeError(f"{what}: the context's last hit pass is {self.ctx._aov_shape}, not this renderer's")

    def RenderShadows(self) -> np.ndarray:
        """The shadow pass of the last RenderAOV (rtx_render_shadows_async; not in the reference's Renderer):
        per pixel a word whose bit l says light l of the scene uploaded last is occluded, kept on the device
        for Relight and returned.  Blocking."""
        self._own_pass("RenderShadows", self.ctx.render_shadows_async)
        self.ctx.render_shadows_async()
        return self.ctx.download_shadows()

    def UpdateShadows(self, lights: int) -> np.ndarray:
        """RenderShadows for the lights named in `lights` only (bit l = light l), merged into the plane
        (rtx_update_shadows_async): the step after an upload that moved those lights and no other.  Returns
        the plane.  Blocking."""
        self._own_pass("UpdateShadows", lambda: self.ctx.update_shadows_async(lights))
        self.ctx.update_shadows_async(lights)
        return self.ctx.download_shadows()

    def RefreshShadows(self) -> np.ndarray:
        """The plane made valid for the scene uploaded last at the least cost (rtx_refresh_shadows_async):
        only the lights that moved, appeared or went are traced or cleared; the full pass when there is no
        plane of the last RenderAOV.  Returns the plane.  Blocking."""
        self._own_pass("RefreshShadows", self.ctx.refresh_shadows_async)
        self.ctx.refresh_shadows_async()
        return self.ctx.download_shadows()

    def Relight(self, want_rgb: bool = False) -> np.ndarray:
        """The frame Render would render, shaded from the last RenderAOV's planes and the last
        RenderShadows' bits without casting a ray (rtx_relight), with the renderer's CURRENT lighting mode,
        shadows and pixel format; light colours, intensities and material values are the scene's uploaded
        last.  Explicit, like ShadeAOV.  Blocking; fills self.buffer."""
        self._own_pass("Relight", lambda: self.ctx.relight_async(self.params(), want_rgb))
        return self._fill("rtx_relight", want_rgb, C.byref(self.params()))

    def RenderSamplePasses(self, scene: HostScene, k: int, upload: bool = True) -> None:
        """The passes an anti-aliased relighting loop starts from (not in the reference's Renderer): the hit pass
        of the k*m_Width x k*m_Height sample frame of the frame Render would render (all four planes; stripes
        k times as tall), then its shadow pass.  Both stay on the device for RelightResolved.  k in 2, 4, 8, on
        a renderer whose own supersample factor is 1."""
        if k not in (2, 4, 8):
            raise ValueError(f"RenderSamplePasses: k must be 2, 4 or 8, not {k}")
        _, cam = self._view(scene, upload)
        sr, first, step = self.stripe if self.stripe else (0, 0, 1)
        sp = abi.make_params(k * self.m_Width, k * self.m_Height, self.m_CurrentLightingMode, self.m_ShadowsEnabled,
                             self.format, k * sr, first, step)
        self.ctx.render_aov_async(cam, sp, AOV_ALL)
        self.ctx.render_shadows_async()
        self._sample_k = int(k)

    def RelightResolved(self, want_rgb: bool = False) -> np.ndarray:
        """The frame a renderer made with supersample=k would render, from the last RenderSamplePasses without
        casting a ray (rtx_relight_resolve): every stored sample relit with the renderer's CURRENT lighting mode,
        shadows and pixel format and the scene uploaded last, each pixel's k x k samples box-filtered.  After an
        upload that moved a light, RefreshShadows' device call (ctx.refresh_shadows_async) comes first.
        Explicit, like Relight.  Blocking; fills self.buffer."""
        k = getattr(self, "_sample_k", 0)
        if not k or self.ctx._aov_shape != (k * self.m_Width, k * self.m_Height, 1):
            if self.ctx._aov_shape is None:
                self.ctx.relight_resolve_async(self.params(), k or 2, want_rgb)   # no pass yet: the library says why
            raise RuntimeError(f"RelightResolved: the context's last hit pass is {self.ctx._aov_shape}, not this "
                               "renderer's sample pass (RenderSamplePasses)")
        return self._fill("rtx_relight_resolve", want_rgb, C.byref(self.params()), k)

    def TraceRays(self, scene: HostScene, rays, mask: int = AOV_ALL, upload: bool = True) -> dict:
        """Scene::GetClosestHit on the caller's (n, 8) rays against `scene` (same upload bookkeeping as
        Render): the planes of `mask`, element i = ray i's record."""
        self._view(scene, upload)
        return self.ctx.trace_rays(rays, mask)

    def Occluded(self, scene: HostScene, rays, upload: bool = True) -> np.ndarray:
        """Scene::DoesHit on the caller's (n, 8) rays against `scene`: uint8[n]."""
        self._view(scene, upload)
        return self.ctx.occluded(rays)

    def ShadeRays(self, scene: HostScene, rays, upload: bool = True):
        """RenderPixel from GetClosestHit on for the caller's (n, 8) rays against `scene`, with the
        renderer's current lighting mode, shadows and pixel format: (pixels uint32[n], rgb float32[3n])."""
        self._view(scene, upload)
        return self.ctx.shade_rays(rays, self.params())

    def Render(self, scene: HostScene, upload: bool = True, want_rgb: bool = False) -> np.ndarray:
        """Renderer::Render (Renderer.cpp:34-98): blocking; fills self.buffer.  A renderer made with
        `adaptive=(k, threshold)` renders the adaptive frame (RenderAdaptive)."""
        if self.adaptive is not None:
            return self.RenderAdaptive(scene, *self.adaptive, upload=upload, want_rgb=want_rgb)
        s, cam = self._view(scene, upload)
        return self._fill("rtx_render", want_rgb, C.byref(cam), C.byref(self.params()))

    def RenderAdaptive(self, scene: HostScene, k: int, threshold: int, upload: bool = True,
                       want_rgb: bool = False) -> np.ndarray:
        """Render with adaptive supersampling (rtx_render_adaptive; not in the reference's Renderer):
        k x k samples for the pixels whose 8-bit colour differs from a 4-neighbour's by more than
        `threshold` in a channel, the plain pixel elsewhere.  Blocking; fills self.buffer."""
        _, cam = self._view(scene, upload)
        return self._fill("rtx_render_adaptive", want_rgb, C.byref(cam), C.byref(self.params()), int(k), int(threshold))

    def CycleLightingMode(self) -> None:   # Renderer.cpp:189-193
        self.m_CurrentLightingMode = (self.m_CurrentLightingMode + 1) % LightingMode.Count

    def ToggleShadows(self) -> None:       # Renderer.h:34-36
        self.m_ShadowsEnabled = not self.m_ShadowsEnabled

    def SaveBufferToImage(self, path: str = "RayTracing_Buffer.bmp") -> bool:
        """SDL_SaveBMP of the XRGB8888 surface (Renderer.cpp:184-187): 32-bit BI_RGB BMP."""
        return save_bmp(path, self.buffer, self.m_Width, self.m_Height)


def save_bmp(path: str, pixels: np.ndarray, width: int, height: int) -> bool:
    img = np.asarray(pixels, dtype=np.uint32).reshape(height, width)[::-1]   # bottom-up rows
    data = img.astype("<u4").tobytes()
    header = struct.pack("<2sIHHI", b"BM", 14 + 40 + len(data), 0, 0, 54)
    info = struct.pack("<IiiHHIIiiII", 40, width, height, 1, 32, 0, len(data), 2835, 2835, 0, 0)
    with open(path, "wb") as f:
        f.write(header + info + data)
    return True
