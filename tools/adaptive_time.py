"""Adaptive supersampling beside the plain and the fully supersampled frame of the same camera: serialized
frames on one stream through rtx_time_frames / rtx_time_adaptive_frames, the series interleaved in one
process; one JSON line per figure and one summary line (medians, spreads, ratios, model) per scene.

    python tools/adaptive_time.py SCENE[,SCENE...] WxH REPEATS ITERS [K]

Series (each on a context of its own, so that none changes another's launch shape or schedule):
  plain          the frame, factor 1
  full           the frame with rtx_set_supersample(K): the comparator
  adaptive_t8    rtx_render_adaptive_async(K, 8)
  adaptive_t32   rtx_render_adaptive_async(K, 32)
  adaptive_t255  ... with the empty mask: the plain frame + the counter reset, the classifier and a
                 refinement launch that finds nothing (the mode's fixed cost)
  shade          rtx_shade_rays_device over the frame's W * H primary rays in 8 x 8 tiles, pixels and colours:
                 the per-ray cost of the body the refinement restates
Beside them the refined share |E| / (W * H) of each threshold, and the model
  plain + (adaptive_t255 - plain) + share * K^2 * shade / (W * H).
W and H multiples of 8.

profiles/adaptive/adaptive_vs_full.txt: W4_Bunny,W3,Synthetic100k 1920x1080 9 100."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rayq_time import Hip, primary_rays, wave_tiles  # noqa: E402
from gp1_raytracer_2223_amd import abi  # noqa: E402
from gp1_raytracer_2223_amd.renderer import DeviceContext  # noqa: E402
from gp1_raytracer_2223_amd.scene import HostScene  # noqa: E402

TAUS = (8, 32, 255)


def main():
    scenes = sys.argv[1].split(",")
    W, H = (int(x) for x in sys.argv[2].split("x"))
    reps, iters = int(sys.argv[3]), int(sys.argv[4])
    K = int(sys.argv[5]) if len(sys.argv) > 5 else 4
    n = W * H
    for name in scenes:
        hs = HostScene(name)
        s, cam = hs.view()
        p = abi.make_params(W, H)
        ctxs = {k: DeviceContext(0) for k in ("plain", "full", "shade") + tuple(f"adaptive_t{t}" for t in TAUS)}
        for c in ctxs.values():
            c.upload(s)
        ctxs["full"].set_supersample(K)
        hip = Hip()
        d_rays = hip.upload(primary_rays(cam, W, H)[wave_tiles(W, H)])
        d_px, d_rgb = hip.alloc(4 * n), hip.alloc(12 * n)
        series = {"plain": lambda: ctxs["plain"].time_frames(cam, p, iters),
                  "full": lambda: ctxs["full"].time_frames(cam, p, iters),
                  "shade": lambda: ctxs["shade"].time_shade_rays(d_rays, n, p, d_px, d_rgb, iters)}
        for t in TAUS:
            series[f"adaptive_t{t}"] = (lambda t=t: ctxs[f"adaptive_t{t}"].time_adaptive_frames(cam, p, K, t, iters))
        for f in series.values():   # the shapes' measured frames, cost order and tuner; allocations
            f()
            f()
        share = {t: ctxs[f"adaptive_t{t}"].adaptive_refined() / n for t in TAUS}
        figs = {k: [] for k in series}
        for r in range(reps):   # interleaved, so a drift of the machine touches all alike
            for k, f in series.items():
                ms = f()
                figs[k].append(ms)
                print(json.dumps({"scene": name, "width": W, "height": H, "k": K, "what": k, "rep": r, "iters": iters,
                                  "ms": round(ms, 5)}), flush=True)
        med = {k: statistics.median(v) for k, v in figs.items()}
        spread = {k: max(v) - min(v) for k, v in figs.items()}
        fixed = med["adaptive_t255"] - med["plain"]
        per_ray = med["shade"] / n
        summ = {"scene": name, "width": W, "height": H, "k": K,
                "summary": "median of %d figures of %d serialized frames" % (reps, iters),
                **{k + "_ms": round(v, 5) for k, v in med.items()},
                **{k + "_range_ms": [round(min(figs[k]), 5), round(max(figs[k]), 5)] for k in figs},
                "classify_and_empty_refine_ms": round(fixed, 5), "shade_ns_per_ray": round(per_ray * 1e6, 4)}
        for t in (8, 32):
            a = med[f"adaptive_t{t}"]
            model = med["plain"] + fixed + share[t] * K * K * med["shade"]
            summ[f"t{t}"] = {"refined_share": round(share[t], 5), "adaptive_over_plain": round(a / med["plain"], 3),
                             "model_over_plain": round(model / med["plain"], 3), "model_ms": round(model, 5),
                             "full_over_adaptive": round(med["full"] / a, 3),
                             "full_minus_adaptive_ms": round(med["full"] - a, 5),
                             "adaptive_spread_ms": round(spread[f"adaptive_t{t}"], 5),
                             "faster_beyond_spread": bool(med["full"] - a > spread[f"adaptive_t{t}"])}
        summ["full_over_plain"] = round(med["full"] / med["plain"], 3)
        print(json.dumps(summ), flush=True)
        for c in ctxs.values():
            c.synchronize()
        for d in (d_rays, d_px, d_rgb):
            hip.free(d)
        for c in ctxs.values():
            c.close()


if __name__ == "__main__":
    main()
