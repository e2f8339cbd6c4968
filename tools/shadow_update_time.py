"""The incremental shadow pass beside the full pass, the relight and the colour frame of the same build: serialized
launches on one stream through rtx_time_shadows / rtx_time_shadows_update / rtx_time_relight / rtx_time_frames,
interleaved in one process; one JSON line per figure and one summary line (medians, ranges, the ratios) per scene.

    python tools/shadow_update_time.py SCENE[,SCENE...] WxH REPEATS ITERS [--full-only]

Combined lighting, shadows on.  The series: the full shadow pass (every light, keep mask 0: the plane is not read);
the update of one light (light 0), of half the lights (the lower half) and of all lights (the full pass's rays plus
the merge's load: its own cost over the full pass); the relight (pixels only); the frame.

Comparison points: update(1) / full pass (what moving one light costs against tracing them all), (update(1) +
relight) / frame (the relighting loop's step against rendering from scratch) and update(all) / full pass.

--full-only times the full pass alone: with RTX_HIP_LIB naming another build's library, the A/B of
profiles/shadow_update/ab_full_pass.txt (a fresh process per library, alternating).

profiles/shadow_update/update_vs_pass.txt: W4_Bunny,W3,W4_Optional,Bunny8Lights,Synthetic100k 1920x1080 9 100."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gp1_raytracer_2223_amd import abi  # noqa: E402
from gp1_raytracer_2223_amd.renderer import AOV_ALL, DeviceContext  # noqa: E402
from gp1_raytracer_2223_amd.scene import HostScene  # noqa: E402


def main():
    full_only = "--full-only" in sys.argv
    args = [a for a in sys.argv[1:] if a != "--full-only"]
    scenes = args[0].split(",")
    W, H = (int(x) for x in args[1].split("x"))
    reps, iters = int(args[2]), int(args[3])
    for name in scenes:
        hs = HostScene(name)
        s, cam = hs.view()
        L = int(s.n_lights)
        ctx = DeviceContext(0)
        ctx.upload(s)
        p = abi.make_params(W, H)
        for _ in range(3):   # the shape's measured frames, cost order, split tuner
            ctx.time_frames(cam, p, iters)
        ctx.time_aov_frames(cam, p, AOV_ALL, 1)   # the hit pass every series below reads
        half = (1 << max(L // 2, 1)) - 1
        # (the full pass comes first in every round: the updates and the relight need the plane it leaves)
        series = {"shadows": lambda: ctx.time_shadows(iters)}
        if not full_only:
            series.update({"update_1": lambda: ctx.time_shadows_update(1, iters),
                           "update_half": lambda: ctx.time_shadows_update(half, iters),
                           "update_all": lambda: ctx.time_shadows_update((1 << L) - 1, iters),
                           "relight_px": lambda: ctx.time_relight(p, False, iters),
                           "frame": lambda: ctx.time_frames(cam, p, iters)})
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
        out = {"scene": name, "width": W, "height": H, "lights": L,
               "summary": "median of %d figures of %d launches" % (reps, iters),
               **{k + "_ms": round(v, 5) for k, v in med.items()},
               **{k + "_range_ms": [round(min(figs[k]), 5), round(max(figs[k]), 5)] for k in figs}}
        if not full_only:
            out.update({"half_mask": half,
                        "update1_over_full": round(med["update_1"] / med["shadows"], 4),
                        "update_half_over_full": round(med["update_half"] / med["shadows"], 4),
                        "update_all_over_full": round(med["update_all"] / med["shadows"], 4),
                        "update1_plus_relight_over_frame": round((med["update_1"] + med["relight_px"]) / med["frame"], 4),
                        "full_plus_relight_over_frame": round((med["shadows"] + med["relight_px"]) / med["frame"], 4)})
        out.update({"variant": ctx.spec_info()[1], "cull": ctx.cull_info()[0], "room_skip": ctx.room_info()[0],
                    "heavy_tiles": ctx.split_info()[0]})
        print(json.dumps(out), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
