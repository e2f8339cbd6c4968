"""One step of the relighting loop, timed two ways in the same build: the scene change through rtx_upload_scene
and through rtx_edit_lights.  WALL time on the host, from the call to the end of rtx_synchronize: an upload's cost
is mostly host work (the pack, the emit, the copy's submission), which stream time alone would hide.

    python tools/edit_loop.py SCENE[,SCENE...] WxH STEPS ROUNDS

Combined lighting, shadows on, after the hit pass and the shadow pass of the frame.  Per scene, ROUNDS rounds of
every series, interleaved (a drift of the machine touches all alike), each round STEPS steps after STEPS / 10 of
warm-up; a series' figure is the median over all its steps, its spread the range of its rounds' medians:
  relight          rtx_relight_async alone (the floor of every step)
  value_upload     light 0's colour alternates between two values: rtx_upload_scene, relight
  value_edit       ... rtx_edit_lights, relight
  move_upload      light 0's origin alternates between two places: rtx_upload_scene, rtx_refresh_shadows_async, relight
  move_edit        ... rtx_edit_lights, refresh, relight
Then the frame time of the launch shape (rtx_time_frames, 1 frame a figure) in steady state, in the first frames
after an edit and in the first frames after an upload: an edit leaves the tile schedule warm.
One JSON line per (scene, series, round) and one summary line per scene.

profiles/scene_edit/edit_loop.txt: W4_Bunny,W3,W4_Optional,Bunny8Lights,Synthetic100k 1920x1080 200 5."""
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gp1_raytracer_2223_amd import abi  # noqa: E402
from gp1_raytracer_2223_amd.renderer import AOV_ALL, DeviceContext  # noqa: E402
from gp1_raytracer_2223_amd.scene import HostScene  # noqa: E402


def variant(s, light: abi.Light):
    """(scene with light 0 replaced, the one-record array an edit takes); the scene keeps its arrays."""
    arr = (abi.Light * s.n_lights)()
    for l in range(s.n_lights):
        C.memmove(C.byref(arr[l]), C.byref(s.lights[l]), C.sizeof(abi.Light))
    arr[0] = light
    s2 = abi.Scene()
    C.memmove(C.byref(s2), C.byref(s), C.sizeof(abi.Scene))
    s2.lights = arr
    s2._keep = (arr, s)
    return s2, (abi.Light * 1)(light)


def copy_light(l):
    out = abi.Light()
    C.memmove(C.byref(out), C.byref(l), C.sizeof(abi.Light))
    return out


def main():
    scenes = sys.argv[1].split(",")
    W, H = (int(x) for x in sys.argv[2].split("x"))
    steps, rounds = int(sys.argv[3]), int(sys.argv[4])
    for name in scenes:
        hs = HostScene(name)
        s, cam = hs.view()
        ctx = DeviceContext(0)
        lib, h = ctx.lib, ctx.h
        p = abi.make_params(W, H)
        ctx.upload(s)
        for _ in range(3):   # the shape's measured frames, cost order, split tuner
            ctx.time_frames(cam, p, 20)
        ctx.render_aov_async(cam, p, AOV_ALL)
        ctx.render_shadows_async()
        ctx.synchronize()
        base = copy_light(s.lights[0])
        tint, away = copy_light(base), copy_light(base)
        tint.color[:] = [0.25, 0.75, 0.5]
        away.origin[:] = [base.origin[0] + 0.5, base.origin[1] - 0.25, base.origin[2] + 0.5]
        values = [variant(s, base), variant(s, tint)]
        moves = [variant(s, base), variant(s, away)]
        traced = C.c_uint32()

        def ok(rc):
            if rc != abi.RTX_OK:
                raise RuntimeError(f"code {rc}: {lib.rtx_last_error(h).decode()}")

        def relight(k):
            ok(lib.rtx_relight_async(h, C.byref(p), 0))

        def value_upload(k):
            ok(lib.rtx_upload_scene(h, C.byref(values[k & 1][0])))
            ok(lib.rtx_relight_async(h, C.byref(p), 0))

        def value_edit(k):
            ok(lib.rtx_edit_lights(h, 0, 1, values[k & 1][1]))
            ok(lib.rtx_relight_async(h, C.byref(p), 0))

        def move_upload(k):
            ok(lib.rtx_upload_scene(h, C.byref(moves[k & 1][0])))
            ok(lib.rtx_refresh_shadows_async(h, C.byref(traced)))
            ok(lib.rtx_relight_async(h, C.byref(p), 0))

        def move_edit(k):
            ok(lib.rtx_edit_lights(h, 0, 1, moves[k & 1][1]))
            ok(lib.rtx_refresh_shadows_async(h, C.byref(traced)))
            ok(lib.rtx_relight_async(h, C.byref(p), 0))

        series = {"relight": relight, "value_upload": value_upload, "value_edit": value_edit,
                  "move_upload": move_upload, "move_edit": move_edit}
        every = {k: [] for k in series}
        medians = {k: [] for k in series}
        for r in range(rounds):
            for what, step in series.items():
                times = []
                for k in range(1, steps // 10 + steps + 1):   # (k = 1 first: every step changes the scene)
                    t0 = time.perf_counter()
                    step(k)
                    ok(lib.rtx_synchronize(h))
                    times.append((time.perf_counter() - t0) * 1e3)
                times = times[steps // 10:]
                if what.startswith("move") and traced.value != 1:
                    raise RuntimeError(f"{what}: the refresh traced mask {traced.value:#x}, not light 0 alone")
                every[what] += times
                medians[what].append(statistics.median(times))
                print(json.dumps({"scene": name, "width": W, "height": H, "what": what, "round": r, "steps": steps,
                                  "median_ms": round(medians[what][-1], 5), "min_ms": round(min(times), 5),
                                  "p90_ms": round(sorted(times)[int(0.9 * len(times))], 5)}), flush=True)
                ok(lib.rtx_upload_scene(h, C.byref(values[0][0])))   # every series starts from the base scene
                ok(lib.rtx_refresh_shadows_async(h, C.byref(traced)))
        med = {k: statistics.median(v) for k, v in every.items()}
        # the frame: steady state, then the first frames after an edit and after an upload (1 frame a figure)
        for _ in range(3):
            ctx.time_frames(cam, p, 20)
        steady = [ctx.time_frames(cam, p, 1) for _ in range(9)]
        ok(lib.rtx_edit_lights(h, 0, 1, values[1][1]))
        after_edit = [ctx.time_frames(cam, p, 1) for _ in range(5)]
        ok(lib.rtx_upload_scene(h, C.byref(values[0][0])))
        after_upload = [ctx.time_frames(cam, p, 1) for _ in range(5)]
        nb = C.c_uint64(0)
        lib.rtx_scene_bytes(h, C.byref(nb))
        out = {"scene": name, "width": W, "height": H, "lights": int(s.n_lights), "scene_bytes": int(nb.value),
               "summary": "median of %d rounds x %d steps, wall ms; range of the rounds' medians" % (rounds, steps),
               **{k + "_ms": round(v, 5) for k, v in med.items()},
               **{k + "_range_ms": [round(min(medians[k]), 5), round(max(medians[k]), 5)] for k in medians},
               "value_upload_over_edit": round(med["value_upload"] / med["value_edit"], 2),
               "move_upload_over_edit": round(med["move_upload"] / med["move_edit"], 2),
               "value_edit_over_relight": round(med["value_edit"] / med["relight"], 3),
               "frame_steady_ms": round(statistics.median(steady), 5),
               "frames_after_edit_ms": [round(x, 5) for x in after_edit],
               "frames_after_upload_ms": [round(x, 5) for x in after_upload],
               "cull": ctx.cull_info()[0], "room_skip": ctx.room_info()[0], "heavy_tiles": ctx.split_info()[0]}
        print(json.dumps(out), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
