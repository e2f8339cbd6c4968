"""The hit pass beside the colour frame of the same build: serialized frames on one stream through
rtx_time_frames / rtx_time_aov_frames, one JSON line per figure and one summary line (medians, the
pass / colour ratio) per (scene, size).

    python tools/aov_time.py SCENE[,SCENE...] WxH REPEATS ITERS

profiles/aov/pass_vs_colour.txt: W4_Bunny,Synthetic100k 1920x1080 9 100."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gp1_raytracer_2223_amd import abi  # noqa: E402
from gp1_raytracer_2223_amd.renderer import AOV_ALL, AOV_DEPTH, DeviceContext  # noqa: E402
from gp1_raytracer_2223_amd.scene import HostScene  # noqa: E402

scenes = sys.argv[1].split(",")
W, H = (int(x) for x in sys.argv[2].split("x"))
reps, iters = int(sys.argv[3]), int(sys.argv[4])
for name in scenes:
    hs = HostScene(name)
    s, cam = hs.view()
    ctx = DeviceContext(0)
    ctx.upload(s)
    p = abi.make_params(W, H)
    for _ in range(3):   # the shape's measured frames, cost order, split tuner
        ctx.time_frames(cam, p, iters)
    series = {"colour": lambda: ctx.time_frames(cam, p, iters),
              "aov_depth": lambda: ctx.time_aov_frames(cam, p, AOV_DEPTH, iters),
              "aov_all": lambda: ctx.time_aov_frames(cam, p, AOV_ALL, iters)}
    for f in series.values():   # (the planes' allocation and the first launches outside the figures)
        f()
    figs = {k: [] for k in series}
    for r in range(reps):   # the three series interleaved, so a drift of the machine touches all alike
        for k, f in series.items():
            ms = f()
            figs[k].append(ms)
            print(json.dumps({"scene": name, "width": W, "height": H, "what": k, "rep": r, "iters": iters,
                              "ms_per_frame": round(ms, 5)}), flush=True)
    med = {k: statistics.median(v) for k, v in figs.items()}
    print(json.dumps({"scene": name, "width": W, "height": H, "summary": "median of %d figures of %d frames" % (reps, iters),
                      **{k + "_ms": round(v, 5) for k, v in med.items()},
                      **{k + "_range_ms": [round(min(figs[k]), 5), round(max(figs[k]), 5)] for k in figs},
                      "depth_over_colour": round(med["aov_depth"] / med["colour"], 4),
                      "all_over_colour": round(med["aov_all"] / med["colour"], 4),
                      "cull": ctx.cull_info()[0], "heavy_tiles": ctx.split_info()[0]}), flush=True)
    ctx.close()
