"""Relighting beside the colour frame and deferred shading of the same build: serialized launches on one stream
through rtx_time_frames / rtx_time_shade_aov / rtx_time_shadows / rtx_time_relight, interleaved in one process; one
JSON line per figure and one summary line (medians, ranges, the ratios) per scene.

    python tools/relight_time.py SCENE[,SCENE...] WxH REPEATS ITERS

Combined lighting, shadows on.  The series: the frame, the shade of a stored hit pass (rtx_shade_aov, which traces
every shadow ray again), the shadow pass (a moved light pays less: tools/shadow_update_time.py), the relight with pixels only and with
both planes, and a device-to-device copy of 32 bytes per pixel: the relight reads 28 (depth 4, normal 12, material
4, primitive 4, shadow word 4) and writes 4.  The copy reads and writes its 32, so it moves twice the relight's
bytes; half of it is the floor.

Comparison points: relight / frame and relight / shade (what a light, material, mode or shadow change costs
against tracing again), and relight against the lightest existing shade of a tile-dispatched pass (ObservedArea
without shadows), measured here as shade_oa_ms.

profiles/relight/relight_vs_frame.txt: W4_Bunny,W3,W4_Optional,Bunny8Lights,Synthetic100k 1920x1080 9 100."""
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rayq_time import Hip  # noqa: E402
from gp1_raytracer_2223_amd import abi  # noqa: E402
from gp1_raytracer_2223_amd.renderer import AOV_ALL, DeviceContext  # noqa: E402
from gp1_raytracer_2223_amd.scene import HostScene  # noqa: E402


def main():
    scenes = sys.argv[1].split(",")
    W, H = (int(x) for x in sys.argv[2].split("x"))
    reps, iters = int(sys.argv[3]), int(sys.argv[4])
    n = W * H
    hip = Hip()
    for name in scenes:
        hs = HostScene(name)
        s, cam = hs.view()
        ctx = DeviceContext(0)
        ctx.upload(s)
        p = abi.make_params(W, H)
        p_oa = abi.make_params(W, H, abi.RTX_MODE_OBSERVED_AREA, 0)
        d_rec = hip.alloc(32 * n)
        for _ in range(3):   # the shape's measured frames, cost order, split tuner
            ctx.time_frames(cam, p, iters)
        ctx.time_aov_frames(cam, p, AOV_ALL, 1)   # the hit pass every series below reads

        def copy():   # n rays of 32 bytes
            ms = C.c_float()
            abi.check(ctx.lib.rtx_time_ray_queries(ctx.h, d_rec, n, 2, AOV_ALL, None, None, iters, C.byref(ms)),
                      "rtx_time_ray_queries", ctx.h)
            return ms.value

        # (the shadow pass comes before the relights in every round: they read the plane it leaves)
        series = {"frame": lambda: ctx.time_frames(cam, p, iters),
                  "shade": lambda: ctx.time_shade_aov(p, False, iters),
                  "shade_oa": lambda: ctx.time_shade_aov(p_oa, False, iters),
                  "shadows": lambda: ctx.time_shadows(iters),
                  "relight_px": lambda: ctx.time_relight(p, False, iters),
                  "relight_both": lambda: ctx.time_relight(p, True, iters),
                  "copy_32B": copy}
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
        print(json.dumps({"scene": name, "width": W, "height": H, "lights": int(s.n_lights),
                          "summary": "median of %d figures of %d launches" % (reps, iters),
                          **{k + "_ms": round(v, 5) for k, v in med.items()},
                          **{k + "_range_ms": [round(min(figs[k]), 5), round(max(figs[k]), 5)] for k in figs},
                          "relight_over_frame": round(med["relight_px"] / med["frame"], 4),
                          "relight_over_shade": round(med["relight_px"] / med["shade"], 4),
                          "relight_over_lightest_shade": round(med["relight_px"] / med["shade_oa"], 4),
                          "relight_over_half_copy": round(med["relight_px"] / (med["copy_32B"] / 2), 4),
                          "shadows_over_shade": round(med["shadows"] / med["shade"], 4),
                          "both_over_px": round(med["relight_both"] / med["relight_px"], 4),
                          "relight_GBps": round(32 * n / med["relight_px"] / 1e6, 1),
                          "variant": ctx.spec_info()[1], "cull": ctx.cull_info()[0], "room_skip": ctx.room_info()[0],
                          "heavy_tiles": ctx.split_info()[0]}), flush=True)
        hip.free(d_rec)
        ctx.close()


if __name__ == "__main__":
    main()
