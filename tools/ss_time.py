"""rtx_time_frames on W4_Bunny, plain and supersampled: one JSON line per (label, W, H, k, repeat).

    [RTX_HIP_LIB=<experiment build>] python tools/ss_time.py LABEL WxHxk[,WxHxk...] REPEATS ITERS

The library is the one RTX_HIP_LIB names (a fresh process per library; one without
rtx_set_supersample can time k = 1 only).  profiles/ss/fused_resolve.txt alternates
`parent 3840x2160x1,7680x4320x1` with `this 1920x1080x2,1920x1080x4,...`."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gp1_raytracer_2223_amd import abi
from gp1_raytracer_2223_amd.renderer import DeviceContext
from gp1_raytracer_2223_amd.scene import HostScene

label = sys.argv[1]
cases = [tuple(int(x) for x in c.split("x")) for c in sys.argv[2].split(",")]   # WxHxk
reps, iters = int(sys.argv[3]), int(sys.argv[4])
hs = HostScene("W4_Bunny")
s, cam = hs.view()
ctx = DeviceContext(0)
ctx.upload(s)
for W, H, k in cases:
    if k != 1:
        ctx.set_supersample(k)
    p = abi.make_params(W, H)
    ctx.time_frames(cam, p, 100)   # the shape's measured frames, cost order, tuner
    ctx.time_frames(cam, p, 100)
    for r in range(reps):
        ms = ctx.time_frames(cam, p, iters)
        print(json.dumps({"lib": label, "width": W, "height": H, "k": k, "samples": W * k * H * k, "rep": r,
                          "iters": iters, "ms_per_frame": round(ms, 5), "px_plane_bytes": W * H * 4}), flush=True)
    if k != 1:
        ctx.set_supersample(1)
ctx.close()
