"""Shaded rays beside the colour frame of the same camera: serialized launches on one stream through
rtx_time_shade_rays / rtx_time_frames, interleaved in one process; one JSON line per figure and one
summary line (medians and ratios) per scene.

    python tools/shade_time.py SCENE[,SCENE...] WxH REPEATS ITERS

The rays are the frame's primary rays (made in numpy as tools/rayq_time.py makes them: timing needs no
bit parity), once in the frame's order (64 consecutive rays = one 8 x 8 tile) and once row-major, each
with the colour plane alone and with both outputs.  Beside them: the frame (rtx_time_frames, same
scene, camera, mode and shadows), the frame on a context without the room skip (RTX_ROOM_SKIP=0) and,
where the scene has the exact cull, on one without it (RTX_NO_CULL=1) -- a caller's ray has neither --
the frame through the generic kernel (RTX_NO_SPEC=1 with both off: the body the shade kernel restates),
and the device-to-device copy of the 32 bytes per ray a shade call reads and the frame does not.
W and H multiples of 8.

profiles/shade/shade_vs_frame.txt: W4_Bunny,W3,Synthetic100k 1920x1080 9 100."""
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rayq_time import Hip, primary_rays, wave_tiles  # noqa: E402
from gp1_raytracer_2223_amd import abi  # noqa: E402
from gp1_raytracer_2223_amd.renderer import AOV_ALL, DeviceContext  # noqa: E402
from gp1_raytracer_2223_amd.scene import HostScene  # noqa: E402


def context_with(env, scene):
    os.environ.update(env)
    try:
        c = DeviceContext(0)
    finally:
        for k in env:
            del os.environ[k]
    c.upload(scene)
    return c


def main():
    scenes = sys.argv[1].split(",")
    W, H = (int(x) for x in sys.argv[2].split("x"))
    reps, iters = int(sys.argv[3]), int(sys.argv[4])
    for name in scenes:
        hs = HostScene(name)
        s, cam = hs.view()
        ctx = DeviceContext(0)
        hip = Hip()
        ctx.upload(s)
        p = abi.make_params(W, H)
        n = W * H
        rm = primary_rays(cam, W, H)
        tiled = rm[wave_tiles(W, H)]
        d_tiled, d_rm = hip.upload(tiled), hip.upload(rm)
        d_px, d_rgb = hip.alloc(4 * n), hip.alloc(12 * n)
        culled = bool(ctx.cull_info()[0])
        noskip = context_with({"RTX_ROOM_SKIP": "0"}, s)
        nocull = context_with({"RTX_NO_CULL": "1"}, s) if culled else None
        # the frame through the generic kernel (SPEC 0), the body rtx_shade_kernel restates
        nospec = context_with({"RTX_NO_SPEC": "1", "RTX_ROOM_SKIP": "0", "RTX_NO_CULL": "1"}, s)

        def copy():
            ms = C.c_float()
            abi.check(ctx.lib.rtx_time_ray_queries(ctx.h, d_tiled, n, 2, AOV_ALL, None, None, iters, C.byref(ms)),
                      "rtx_time_ray_queries", ctx.h)
            return ms.value

        series = {"frame": lambda: ctx.time_frames(cam, p, iters),
                  "frame_noskip": lambda: noskip.time_frames(cam, p, iters),
                  "frame_generic": lambda: nospec.time_frames(cam, p, iters),
                  "shade_tiled_rgb": lambda: ctx.time_shade_rays(d_tiled, n, p, 0, d_rgb, iters),
                  "shade_tiled_both": lambda: ctx.time_shade_rays(d_tiled, n, p, d_px, d_rgb, iters),
                  "shade_rowmajor_rgb": lambda: ctx.time_shade_rays(d_rm, n, p, 0, d_rgb, iters),
                  "shade_rowmajor_both": lambda: ctx.time_shade_rays(d_rm, n, p, d_px, d_rgb, iters),
                  "copy_rays": copy}
        if nocull is not None:
            series["frame_nocull"] = lambda: nocull.time_frames(cam, p, iters)
        for f in series.values():   # (allocations and first launches outside the figures)
            f()
        figs = {k: [] for k in series}
        for r in range(reps):   # interleaved, so a drift of the machine touches all alike
            for k, f in series.items():
                ms = f()
                figs[k].append(ms)
                print(json.dumps({"scene": name, "width": W, "height": H, "what": k, "rep": r, "iters": iters,
                                  "ms": round(ms, 5)}), flush=True)
        med = {k: statistics.median(v) for k, v in figs.items()}
        summ = {"scene": name, "width": W, "height": H, "rays": n,
                "summary": "median of %d figures of %d launches" % (reps, iters),
                **{k + "_ms": round(v, 5) for k, v in med.items()},
                **{k + "_range_ms": [round(min(figs[k]), 5), round(max(figs[k]), 5)] for k in figs},
                "shade_over_frame": round(med["shade_tiled_both"] / med["frame"], 4),
                "shade_over_frame_plus_copy": round(med["shade_tiled_both"] / (med["frame"] + med["copy_rays"]), 4),
                "shade_over_frame_noskip_plus_copy": round(med["shade_tiled_both"] / (med["frame_noskip"] + med["copy_rays"]), 4),
                "shade_over_frame_generic_plus_copy": round(med["shade_tiled_both"] / (med["frame_generic"] + med["copy_rays"]), 4),
                "rowmajor_over_tiled": round(med["shade_rowmajor_both"] / med["shade_tiled_both"], 4),
                "rgb_only_over_both": round(med["shade_tiled_rgb"] / med["shade_tiled_both"], 4), "frame_cull": culled}
        if nocull is not None:
            summ["shade_over_frame_nocull_plus_copy"] = round(
                med["shade_tiled_both"] / (med["frame_nocull"] + med["copy_rays"]), 4)
        print(json.dumps(summ), flush=True)
        ctx.synchronize()
        for d in (d_tiled, d_rm, d_px, d_rgb):
            hip.free(d)
        for c in (noskip, nocull, nospec, ctx):
            if c is not None:
                c.close()


if __name__ == "__main__":
    main()
