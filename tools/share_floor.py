"""What bounds one stripe share of a frame (strong scaling): rank 0's share of a
frame cut into 16-row stripes over s ranks, on one GPU.

Per s it records
  serial_ms     rtx_time_views: the mean of serialized launches of one context (the predictor's method)
  inflight2_ms  two contexts alternating frames of the same share (the bench's --inflight 2), wall time
  noshadow_ms   serialized, shadows off (the primary pass alone)
  tiles         the share's wave tiles; the measured one-piece tile costs (rtx_schedule_state, 16 shader
                cycles per unit, reported in us at RTX_CLOCK_GHZ, default 2.4): max, p99, p90, mean, and
                `crit` = max tile / (sum / wave slots), the share's critical-path bound in units of its
                ideal time

Usage (GPU box): python tools/share_floor.py <scene> <W> <H> [s ...]
"""
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from gp1_raytracer_2223_amd import abi  # noqa: E402

abi.load_hip()
from gp1_raytracer_2223_amd.renderer import DeviceContext  # noqa: E402
from gp1_raytracer_2223_amd.scene import HostScene  # noqa: E402

GHZ = float(os.environ.get("RTX_CLOCK_GHZ", "2.4"))
SLOTS = int(os.environ.get("RTX_WAVE_SLOTS", str(256 * 4 * 8)))


def serial(ctx, cam, p, n=40):
    ms = C.c_float()
    abi.check(ctx.lib.rtx_time_views(ctx.h, cam, 1, C.byref(p), 8, C.byref(ms)), "t", ctx.h)
    best = 1e9
    for _ in range(3):
        abi.check(ctx.lib.rtx_time_views(ctx.h, cam, 1, C.byref(p), n, C.byref(ms)), "t", ctx.h)
        best = min(best, ms.value)
    return best


def inflight(ctxs, cam, p, frames=200):
    for i in range(20):
        ctxs[i % len(ctxs)].render_async(cam, p)
    for c in ctxs:
        c.synchronize()
    best = 1e9
    for _ in range(3):
        t0 = time.perf_counter()
        for i in range(frames):
            ctxs[i % len(ctxs)].render_async(cam, p)
        for c in ctxs:
            c.synchronize()
        best = min(best, (time.perf_counter() - t0) / frames * 1e3)
    return best


def share_tiles(W, H, st):
    """wave tiles of rank 0's share (rtx_frame.hip frame_shape(): the grid of the largest owner)"""
    tx, groups = (W + 7) // 8, (H + 7) // 8
    if st == 1:
        return tx * groups
    nstripes = (groups + 1) // 2
    return tx * ((nstripes + st - 1) // st) * 2


def costs(ctx, ntiles):
    n = C.c_uint32()
    abi.check(ctx.lib.rtx_schedule_state(ctx.h, None, None, 0, C.byref(n)), "sched", ctx.h)
    if n.value == 0:
        return None
    order = np.zeros(ntiles, np.uint32)
    cost = np.zeros(ntiles, np.uint32)
    abi.check(ctx.lib.rtx_schedule_state(ctx.h, order.ctypes.data_as(C.POINTER(C.c_uint32)),
                                         cost.ctypes.data_as(C.POINTER(C.c_uint32)), ntiles, C.byref(n)),
              "sched", ctx.h)
    n.value = ntiles
    us = cost.astype(np.float64) * 16 / (GHZ * 1e3)
    tot = us.sum()
    return {"tiles": int(n.value), "max_us": round(float(us.max()), 2), "p99_us": round(float(np.percentile(us, 99)), 2),
            "p90_us": round(float(np.percentile(us, 90)), 2), "mean_us": round(float(us.mean()), 3),
            "ideal_us": round(float(tot / min(SLOTS, n.value)), 2),
            "crit": round(float(us.max() / (tot / min(SLOTS, n.value))), 3)}


def main():
    scene, W, H = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    steps = [int(x) for x in sys.argv[4:]] or [1, 2, 4, 8]
    hs = HostScene(scene)
    s, cam = hs.view()
    ctxs = [DeviceContext(0), DeviceContext(0)]
    for c in ctxs:
        c.upload(s)
    for st in steps:
        p = abi.make_params(W, H, stripe_rows=16 if st > 1 else 0, stripe_first=0, stripe_step=st)
        ps = abi.make_params(W, H, shadows=False, stripe_rows=16 if st > 1 else 0, stripe_first=0, stripe_step=st)
        row = {"scene": scene, "W": W, "H": H, "s": st}
        row["serial_ms"] = round(serial(ctxs[0], cam, p), 5)
        row["costs"] = costs(ctxs[0], share_tiles(W, H, st))
        row["heavy"] = ctxs[0].split_info()[0]
        row["inflight2_ms"] = round(inflight(ctxs, cam, p), 5)
        row["noshadow_ms"] = round(serial(ctxs[0], cam, ps), 5)
        row["costs_noshadow"] = costs(ctxs[0], share_tiles(W, H, st))
        print(json.dumps(row), flush=True)
    for c in ctxs:
        c.close()


if __name__ == "__main__":
    main()
