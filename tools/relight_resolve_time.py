"""The resolved relight beside the supersampled frame of the same build: serialized launches on one stream through
rtx_time_frames (under rtx_set_supersample), rtx_time_aov_frames, rtx_time_shadows, rtx_time_relight,
rtx_time_relight_resolve and rtx_time_shadows_update, interleaved in one process; one JSON line per figure and one
summary line (medians, ranges, the ratios) per scene and factor.

    python tools/relight_resolve_time.py SCENE[,SCENE...] WxH REPEATS ITERS [K[,K...]]

Combined lighting, shadows on, factors 2 and 4 unless given (8 x 8 at 1080p needs 4.2 GB of planes).  W x H is the
OUTPUT frame; the passes run at kW x kH.  The series, per round in this order (the hit pass makes the shadow plane
stale, so the shadow pass follows it and everything that reads the plane follows that):
    ss_frame      the supersampled frame: what an edit costs without stored passes
    hit, shadows  the two passes at sample size: what the loop pays once
    relight_px    the plain relight of the sample pass, pixels only: the same bytes and arithmetic per sample
    resolve_px    the resolved relight, pixels only; resolve_both with the colour plane
    update_one    the incremental shadow pass for light 0 at sample size: what a moved light adds

Comparison points: resolve / ss_frame and (update_one + resolve) / ss_frame (what an edit of an anti-aliased
frame costs against rendering it again), resolve / relight_px against the plain relight's own spread over the
rounds (max / median): the resolved relight must not lose to it by more than that, and the achieved GB/s over 32
bytes per sample.

profiles/relight_resolve/resolve_vs_ss_frame.txt: W4_Bunny,W3,W4_Optional,Bunny8Lights,Synthetic100k 1920x1080 9 100."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gp1_raytracer_2223_amd import abi  # noqa: E402
from gp1_raytracer_2223_amd.renderer import AOV_ALL, DeviceContext  # noqa: E402
from gp1_raytracer_2223_amd.scene import HostScene  # noqa: E402


def main():
    scenes = sys.argv[1].split(",")
    W, H = (int(x) for x in sys.argv[2].split("x"))
    reps, iters = int(sys.argv[3]), int(sys.argv[4])
    factors = [int(x) for x in sys.argv[5].split(",")] if len(sys.argv) > 5 else [2, 4]
    for name in scenes:
        hs = HostScene(name)
        s, cam = hs.view()
        for k in factors:
            ctx = DeviceContext(0)
            ctx.upload(s)
            p = abi.make_params(W, H)
            sp = abi.make_params(k * W, k * H)
            n_samples = k * W * k * H

            def ss_frame():
                ctx.set_supersample(k)
                try:
                    return ctx.time_frames(cam, p, iters)
                finally:
                    ctx.set_supersample(1)

            for _ in range(3):   # the shape's measured frames, cost order, split tuner
                ss_frame()
            series = {"ss_frame": ss_frame,
                      "hit": lambda: ctx.time_aov_frames(cam, sp, AOV_ALL, iters),
                      "shadows": lambda: ctx.time_shadows(iters),
                      "relight_px": lambda: ctx.time_relight(sp, False, iters),
                      "resolve_px": lambda: ctx.time_relight_resolve(p, k, False, iters),
                      "resolve_both": lambda: ctx.time_relight_resolve(p, k, True, iters),
                      "update_one": lambda: ctx.time_shadows_update(1, iters)}
            for f in series.values():   # (allocations and first launches outside the figures)
                f()
            figs = {key: [] for key in series}
            for r in range(reps):   # interleaved, so a drift of the machine touches all alike
                for key, f in series.items():
                    ms = f()
                    figs[key].append(ms)
                    print(json.dumps({"scene": name, "width": W, "height": H, "k": k, "what": key, "rep": r,
                                      "iters": iters, "ms": round(ms, 5)}), flush=True)
            med = {key: statistics.median(v) for key, v in figs.items()}
            spread = max(figs["relight_px"]) / med["relight_px"]
            over_plain = med["resolve_px"] / med["relight_px"]
            print(json.dumps({"scene": name, "width": W, "height": H, "k": k, "lights": int(s.n_lights),
                              "summary": "median of %d figures of %d launches" % (reps, iters),
                              **{key + "_ms": round(v, 5) for key, v in med.items()},
                              **{key + "_range_ms": [round(min(figs[key]), 5), round(max(figs[key]), 5)] for key in figs},
                              "resolve_over_ss_frame": round(med["resolve_px"] / med["ss_frame"], 4),
                              "update_plus_resolve_over_ss_frame":
                                  round((med["update_one"] + med["resolve_px"]) / med["ss_frame"], 4),
                              "passes_over_ss_frame": round((med["hit"] + med["shadows"]) / med["ss_frame"], 4),
                              "both_over_px": round(med["resolve_both"] / med["resolve_px"], 4),
                              "resolve_GBps": round(32 * n_samples / med["resolve_px"] / 1e6, 1),
                              "relight_GBps": round(32 * n_samples / med["relight_px"] / 1e6, 1),
                              "resolve_over_plain_relight": round(over_plain, 4),
                              "plain_relight_max_over_median": round(spread, 4),
                              "within_plain_relights_spread": bool(over_plain <= spread),
                              "variant": ctx.spec_info()[1], "cull": ctx.cull_info()[0]}), flush=True)
            ctx.close()


if __name__ == "__main__":
    main()
