"""Deferred shading beside the colour frame and the hit pass of the same build: serialized launches on one
stream through rtx_time_frames / rtx_time_aov_frames / rtx_time_shade_aov, interleaved in one process; one
JSON line per figure and one summary line (medians, ranges, the ratios) per scene.

    python tools/deferred_time.py SCENE[,SCENE...] WxH REPEATS ITERS

Combined lighting, shadows on.  The series: the frame, the hit pass with all four planes, the shade of that
pass with pixels only and with both planes, and the device-to-device copy of 24 bytes per pixel (the record
the shade reads and the frame does not; the copy reads and writes them, so half of it is the read).

The ratios: shade / frame, and (pass + shade) / (pass + frame), what a caller who wants the planes and the
colour pays against two full traversals.  The expectation is frame - pass + copy / 2: the frame without the
work the pass does, plus reading the record.

profiles/deferred/shade_aov_vs_frame.txt: W4_Bunny,W3,W4_Optional,Bunny8Lights,Synthetic100k 1920x1080 9 100."""
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
    assert n % 4 == 0, "the copy's 24 B per pixel are counted in 32-byte rays"
    hip = Hip()
    for name in scenes:
        hs = HostScene(name)
        s, cam = hs.view()
        ctx = DeviceContext(0)
        ctx.upload(s)
        p = abi.make_params(W, H)
        d_rec = hip.alloc(24 * n)
        for _ in range(3):   # the shape's measured frames, cost order, split tuner
            ctx.time_frames(cam, p, iters)

        def copy():   # 3n/4 rays of 32 bytes = 24 bytes per pixel
            ms = C.c_float()
            abi.check(ctx.lib.rtx_time_ray_queries(ctx.h, d_rec, 3 * n // 4, 2, AOV_ALL, None, None, iters, C.byref(ms)),
                      "rtx_time_ray_queries", ctx.h)
            return ms.value

        # (the pass comes before the shades in every round: they shade the planes it leaves)
        series = {"frame": lambda: ctx.time_frames(cam, p, iters),
                  "pass_all": lambda: ctx.time_aov_frames(cam, p, AOV_ALL, iters),
                  "shade_px": lambda: ctx.time_shade_aov(p, False, iters),
                  "shade_both": lambda: ctx.time_shade_aov(p, True, iters),
                  "copy_24B": copy}
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
        expect = med["frame"] - med["pass_all"] + med["copy_24B"] / 2
        print(json.dumps({"scene": name, "width": W, "height": H,
                          "summary": "median of %d figures of %d launches" % (reps, iters),
                          **{k + "_ms": round(v, 5) for k, v in med.items()},
                          **{k + "_range_ms": [round(min(figs[k]), 5), round(max(figs[k]), 5)] for k in figs},
                          "shade_over_frame": round(med["shade_px"] / med["frame"], 4),
                          "pass_plus_shade_over_pass_plus_frame":
                              round((med["pass_all"] + med["shade_px"]) / (med["pass_all"] + med["frame"]), 4),
                          "expected_ms": round(expect, 5),
                          "shade_over_expected": round(med["shade_px"] / expect, 4),
                          "expected_pair_ratio": round((med["pass_all"] + expect) / (med["pass_all"] + med["frame"]), 4),
                          "both_over_px": round(med["shade_both"] / med["shade_px"], 4),
                          "variant": ctx.spec_info()[1], "cull": ctx.cull_info()[0], "room_skip": ctx.room_info()[0],
                          "heavy_tiles": ctx.split_info()[0]}), flush=True)
        hip.free(d_rec)
        ctx.close()


if __name__ == "__main__":
    main()
