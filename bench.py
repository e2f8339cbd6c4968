#!/usr/bin/env python3
"""Headline benchmark of the HIP render path (BASELINE.json metric):
Mpixels/s (primary + shadow rays) at 1920x1080 on Scene_W4_BunnyScene (Initialize
state, Combined lighting, shadows on).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--scene S --width W --height H]
                    [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A plain run does what the headline needs and no more: it uploads the scene, warms up (1000
serialized launches per context, then W steps), times the K steps and prints the JSON line with part 1
below (`value`, `ms_per_step`, `config`).  `--dump-outputs DIR` also writes the frames the last timed
step left in HBM, fetched as a caller would fetch them, to DIR/frame.npy (DIR/frame_rank<r>.npy under
torchrun): float32 R, G, B per pixel, shape (views, H, W, 3), or a fixed seeded sample of pixels where
that would pass 48 MB.  The scene and cameras are built from constants, so two runs with the same
arguments render the same inputs.  Everything else — `roofline` (kernel time, FLOP count, PMC
traffic), `host_gather`, `parity`, `end_to_end_mpix_s` and parts 2-4 — takes runs of its own and is
measured only with `--full`.

With `--full` the JSON line has four parts:

1. The headline (`value`), `--mode views` by default.  A step renders N views of the scene:
   view f is the reference camera moved 0.05 f along x.  Every view's rows are cut into 16-row
   stripes dealt round robin over the N ranks (rank r owns view f's stripe s iff
   s % N == (r - f) mod N).  So every image is tiled across all the GPUs and
   every rank renders one frame's worth of pixels per step: weak scaling.  At N = 1 a step is
   exactly one reference Renderer::Render frame.  `--mode frame` tiles ONE frame per step over
   the N ranks (strong scaling).
2. `multi_gpu_configs`, at every N (N = 1 anchors the curve): the headline scene and the north
   star's multi-GPU workloads, W4_Bunny and Synthetic100k 1920x1080 and Bunny + 8 lights 3840x2160
   (+ W4_Optional), each as ONE image per step tiled in 16-row stripes over the N ranks (the reference's one-frame parallel_for,
   Renderer.cpp:79-85) — Mpix/s device-resident and gathered into the page-locked host frame,
   each rank's HBM traffic from the PMC record of this build, and the gathered frame's parity.
3. `parity_configs` (N = 1): every BASELINE config, plus W4_Reference and W4_Optional, rendered
   at full size on a fresh context (4 frames, so the cost-ordered and split state is live)
   against the reference's own frame (tests/golden/config_*.npz).
4. `cpu_baseline`: the reference's CPU Renderer timed on this host (rank 0, N = 1).

Timed regions are bracketed by barrier + stream sync and max-reduced over ranks:
  `value`: K steps with inputs resident in HBM and the frames left in HBM;
  `host_gather`: K steps whose frames are ALSO gathered into page-locked host frames shared by
     all ranks (/dev/shm mapping, hipHostRegister; every rank hipMemcpy2DAsync's only its own
     stripes over its own PCIe link) — the north star's "independent tiles gathered on host".
     PCIe-inclusive, so never `value`.
No data moves between ranks.  The control plane (barrier, max / sum of a few numbers) is a
shared-memory block on the node (ShmCtl), so the bench process loads only the ROCm runtime
librtx_hip links against, never torch's bundled copy.

Frames in flight (--inflight, default 2): consecutive steps go round robin to that many render
contexts on the rank's GPU (each its own stream, frame buffer and tile schedule), so frame k+1
starts while frame k's last waves drain.  `roofline.kernel_ms` is the serialized launch time of
ONE context (HIP events on its stream, mean of 1000 launches), the figure a rocprofv3 kernel
trace of `--inflight 1` shows.  It is measured first, before the W warm-up steps: those 1000
launches (~60 ms) also take the GPU from its idle clock to its steady rendering clock, which a
short run's few warm-up steps do not.

`roofline.traffic` is the HBM bytes per launch from the PMC record (tools/pmc_configs.sh ->
profiles/r*/pmc_configs.json) of THIS build: records carry the SHA-256 of the librtx_hip.so
they were measured with, and a record of another build is never used (traffic null).
"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import json
import mmap
import os
import struct
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

# Load the HIP library before anything else can pull in another copy of the runtime.
from gp1_raytracer_2223_amd import abi  # noqa: E402

abi.load_hip()
from gp1_raytracer_2223_amd.hostframe import SharedFrame  # noqa: E402
from gp1_raytracer_2223_amd.renderer import DeviceContext  # noqa: E402
from gp1_raytracer_2223_amd.scene import HostScene  # noqa: E402

FP32_PEAK_TFLOPS = 157.3   # MI355X FP32 vector peak (MI355X_MICROARCH.md, spec)
HBM_PEAK_GBS = 8000.0      # MI355X HBM3E peak (spec)
GOLDEN = ROOT / "tests" / "golden"
LIB_HIP = ROOT / "gp1_raytracer_2223_amd" / "lib" / "librtx_hip.so"
# ref_harness's FNV-1a (oracle/ref/ref_harness.cpp `bench`) starts from the decimal basis
# 1469598103934665603; SURVEY §8(c)'s recorded hashes use the same one.
FNV_BASIS = 1469598103934665603
COST = [41, 19, 14, 12, 63, 9, 15, 1, 26, 6, 31, 103]   # SURVEY §8(d) FLOP per counted unit
# the exact cull's box test per lane (cull_nf + cull_pass, rtx_hip.hip): (c - o) * inv 6, three fma
# 6, n / f 6 add + 4 min/max, n - dt 1 — the executed-work model of the culled lines (roofline frac)
COST_CULL_TEST = 23
K_KERNEL_LAUNCHES = 1000   # launches averaged for the headline's roofline.kernel_ms

# BASELINE.json's multi-GPU workloads: one image per step, tiled over the ranks (steps per run)
# (+ W4_Optional: with Synthetic100k a scene the exact cull runs on; on those two lines the roofline
# counts the work the culled walk executes, the reference-equivalent rate beside it)
# W4_Bunny 1080p first: the headline scene as ONE frame per step over the N ranks (strong scaling), the
# curve beside `value`'s weak-scaling one in the driver's N = 1, 2, 4, 8 runs
MULTI_GPU_CONFIGS = [("W4_Bunny", 1920, 1080, 300), ("Synthetic100k", 1920, 1080, 100), ("Bunny8Lights", 3840, 2160, 300),
                     ("W4_Optional", 1920, 1080, 300)]
# parity_configs: (scene, W, H, bit-exact required).  Cook-Torrance / Phong use powf, where the
# device libm may differ from glibc by an ulp: those are held to the north star's tolerance.
PARITY_CONFIGS = [("W1", 640, 480, True), ("W3", 1280, 720, False), ("W4_Bunny", 1920, 1080, True),
                  ("Synthetic100k", 1920, 1080, True), ("Bunny8Lights", 3840, 2160, True),
                  ("W4_Reference", 1920, 1080, False), ("W4_Optional", 1920, 1080, False)]
PARITY_FRAMES = 4


def make_views(cam: abi.Camera, n: int) -> "C.Array":
    arr = (abi.Camera * n)()
    for f in range(n):
        C.memmove(C.byref(arr[f]), C.byref(cam), C.sizeof(abi.Camera))
        arr[f].origin[0] = cam.origin[0] + 0.05 * f
    return arr


def fnv1a(px: np.ndarray) -> str:
    h = FNV_BASIS
    m = (1 << 64) - 1
    for b in np.ascontiguousarray(px, dtype="<u4").view(np.uint8).tobytes():
        h = ((h ^ b) * 0x100000001B3) & m
    return f"{h:016x}"


def sha256(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def lib_sha256() -> str:
    return hashlib.sha256(LIB_HIP.read_bytes()).hexdigest()


# ---------------------------------------------------------------------------- control plane
class ShmCtl:
    """Barrier and small reductions over the ranks of ONE node through a /dev/shm block.

    Rank r owns one sequence word and two 16-value slots; it writes only those (aligned 8-byte
    stores, which x86 never tears or reorders against each other).  barrier(): bump the own
    sequence word to k and wait until every rank's is >= k.  Reductions write the values into
    slot k % 2 before the barrier and read every rank's slot after it; a rank cannot come back
    to that slot before every rank has passed the next barrier, i.e. finished reading.  The
    block is created by rank 0 under a temporary name and renamed into place (atomic), and
    unlinked once every rank has mapped it."""

    SLOT = 16

    def __init__(self, world: int, rank: int, tag: str):
        self.world, self.rank = world, rank
        self.k = 0
        words = world * (1 + 2 * self.SLOT)
        nbytes = 8 * words
        path = os.path.join(SharedFrame._dirs()[0] if os.path.isdir("/dev/shm") else tempfile.gettempdir(),
                            f"rtx_ctl_{tag}")
        if rank == 0:
            tmp = f"{path}.{os.getpid()}"
            fd = os.open(tmp, os.O_RDWR | os.O_CREAT | os.O_EXCL, 0o600)
            os.ftruncate(fd, nbytes)
            os.rename(tmp, path)
        else:
            t0 = time.monotonic()
            while True:
                try:
                    fd = os.open(path, os.O_RDWR)
                    if os.fstat(fd).st_size >= nbytes:
                        break
                    os.close(fd)
                except FileNotFoundError:
                    pass
                if time.monotonic() - t0 > 300:
                    raise TimeoutError(f"rank {rank}: control block {path} never appeared")
                time.sleep(0.005)
        try:
            self.mm = mmap.mmap(fd, nbytes, mmap.MAP_SHARED, mmap.PROT_READ | mmap.PROT_WRITE)
        finally:
            os.close(fd)
        a = np.frombuffer(self.mm, dtype=np.int64)
        self.seq = a[:world]
        self.vals = np.frombuffer(self.mm, dtype=np.float64, offset=8 * world).reshape(2, world, self.SLOT)
        self.path = path
        self.barrier()
        if rank == 0:
            try:
                os.unlink(path)   # every rank has it mapped
            except FileNotFoundError:
                pass

    def barrier(self) -> None:
        self.k += 1
        self.seq[self.rank] = self.k
        t0 = time.monotonic()
        while int(self.seq.min()) < self.k:
            if time.monotonic() - t0 > 600:
                raise TimeoutError(f"rank {self.rank}: barrier {self.k} timed out ({self.seq.tolist()})")
            time.sleep(0)

    def allreduce(self, xs: list[float]) -> np.ndarray:
        assert len(xs) <= self.SLOT
        slot = self.vals[(self.k + 1) % 2]
        slot[self.rank, :len(xs)] = xs
        self.barrier()
        return slot[:, :len(xs)].copy()

    def close(self) -> None:
        self.seq = self.vals = None
        try:
            self.mm.close()
        except BufferError:
            pass


class Dist:
    """Rank / world from the torch.distributed.run environment; the control plane is ShmCtl
    (one node, no torch in this process)."""

    def __init__(self):
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        self.local = int(os.environ.get("LOCAL_RANK", "0"))
        self.ctl = None
        if self.world > 1:
            # every rank of one torchrun launch has the same parent (the elastic agent)
            tag = f"{os.environ.get('MASTER_PORT', 'solo')}_{os.getuid()}_{os.getppid()}"
            self.ctl = ShmCtl(self.world, self.rank, tag)

    def barrier(self):
        if self.ctl:
            self.ctl.barrier()

    def max(self, x: float) -> float:
        return x if not self.ctl else float(self.ctl.allreduce([x]).max())

    def sum_i64(self, xs: list[int]) -> list[int]:
        if not self.ctl:
            return xs
        # exact: float64 holds integers below 2^53 (FLOP per frame ~1e10)
        return [int(v) for v in self.ctl.allreduce([float(x) for x in xs]).sum(axis=0)]

    def gather(self, xs: list[float]) -> np.ndarray:
        return np.array([xs], np.float64) if not self.ctl else self.ctl.allreduce(xs)

    def close(self):
        if self.ctl:
            self.ctl.close()


# ---------------------------------------------------------------------------- CPU reference
def write_obj_from_asset(asset: Path, out_obj: Path) -> None:
    """Re-emit an .rtxmesh as OBJ text (exact float round trip, 1-based faces) so the
    reference harness can load it where /root/reference does not exist."""
    b = asset.read_bytes()
    nv, ni = struct.unpack_from("<II", b, 4)
    pos = np.frombuffer(b, np.float32, 3 * nv, 12).reshape(-1, 3)
    idx = np.frombuffer(b, np.int32, ni, 12 + 12 * nv).reshape(-1, 3)
    lines = [f"v {x:.9g} {y:.9g} {z:.9g}" for x, y, z in pos.tolist()]
    lines += [f"f {a + 1} {b_ + 1} {c + 1}" for a, b_, c in idx.tolist()]
    out_obj.write_text("\n".join(lines) + "\n")


def cpu_model() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return ""


def cgroup_cpu_quota() -> float | None:
    """CPUs this process may use per the cgroup-v2 quota (cpu.max), None if unlimited."""
    try:
        q, period = open("/sys/fs/cgroup/cpu.max").read().split()
        return None if q == "max" else int(q) / int(period)
    except (OSError, ValueError):
        return None


class CpuReference:
    """The reference CPU Renderer timed on this host: the reference's own sources built in
    place by oracle/ref (kind "reference"), or the C restatement in oracle/ when that build
    is absent (kind "port").  Test infrastructure, run only outside the timed regions."""

    def __init__(self):
        self.harness = ROOT / "oracle" / "_ref" / "ref_harness"
        self.kind = "reference" if self.harness.exists() else "port"
        self.td = None
        if self.kind == "reference":
            self.td = tempfile.TemporaryDirectory()
            res = Path(self.td.name) / "Resources"
            res.mkdir()
            for stem in ("lowpoly_bunny2", "Assignment3D1"):
                write_obj_from_asset(abi.ASSET_DIR / f"{stem}.rtxmesh", res / f"{stem}.obj")
            self.how = "reference sources built in place with g++ -O2 -ffp-contract=off (oracle/ref), 1024-pixel dynamic chunks"
        else:
            self.how = "C restatement oracle/rtx_oracle.c"

    def run(self, scene: str, width: int, height: int, threads: int, frames: int) -> dict:
        if self.kind == "reference":
            out = subprocess.run([str(self.harness), "bench", scene, "-1", str(width), str(height), str(threads),
                                  str(frames)], cwd=self.td.name, check=True, capture_output=True, text=True,
                                 timeout=900)
            return json.loads(out.stdout.strip().splitlines()[-1])
        sys.path.insert(0, str(ROOT / "tests"))
        import oracle_bind   # test infrastructure: the checker, timed here as the CPU baseline
        hs = HostScene(scene)
        s, cam = hs.view()
        p = abi.make_params(width, height)
        oracle_bind.render(s, cam, p, threads=threads, want_rgb=False)
        ts = []
        for _ in range(frames):
            t0 = time.perf_counter()
            oracle_bind.render(s, cam, p, threads=threads, want_rgb=False)
            ts.append(time.perf_counter() - t0)
        med = float(np.median(ts))
        return {"median_s": med, "mpix_s": width * height / med / 1e6, "fnv": None}

    def close(self):
        if self.td:
            self.td.cleanup()


def cpu_baseline(ref: CpuReference, scene: str, width: int, height: int, frames: int) -> dict:
    """Threads = every CPU this process may run on (len(sched_getaffinity)), which is what the
    reference's PPL parallel_for uses (std::thread::hardware_concurrency, Renderer.cpp:79-85).
    Where a cgroup CPU quota caps the process below that (the GPU box: 16 CPUs of 256), the
    quota-sized run and a single-thread run are recorded too, and `full_host_upper_bound` =
    single-thread rate x hardware threads (perfect linear scaling over every hardware thread,
    SMT included) bounds what the whole host could do."""
    nthreads = len(os.sched_getaffinity(0))
    quota = cgroup_cpu_quota()
    runs = {"all": ref.run(scene, width, height, nthreads, frames)}
    if quota is not None and int(quota) < nthreads:
        runs["quota"] = ref.run(scene, width, height, max(1, int(quota)), frames)
    runs["one"] = ref.run(scene, width, height, 1, 1)
    # `value` = the best CPU configuration measured here (the quota-sized run can beat the
    # oversubscribed hardware_concurrency one), so speedup_vs_cpu is never inflated by a slow run
    best = "quota" if "quota" in runs and runs["quota"]["mpix_s"] > runs["all"]["mpix_s"] else "all"
    r = runs[best]
    used = max(1, int(quota)) if best == "quota" else nthreads
    one = runs["one"]["mpix_s"]
    out = {"value": round(r["mpix_s"], 4), "unit": "Mpixels/s", "cores": used, "kind": ref.kind,
           "sample": f"{frames} frames of {scene} {width}x{height}, median of Renderer::Render, {used} threads "
                     f"(the faster of sched_getaffinity = {nthreads}, the reference's hardware_concurrency, and the "
                     f"cgroup quota), {ref.how}",
           "median_s": r["median_s"], "fnv": r.get("fnv"),
           "all_threads_mpix_s": round(runs["all"]["mpix_s"], 4),
           "single_thread_mpix_s": round(one, 4),
           "full_host_upper_bound_mpix_s": round(one * nthreads, 2),
           "cpu_model": cpu_model(), "nproc": os.cpu_count(), "cgroup_cpu_quota": quota}
    if "quota" in runs:
        out["quota_threads_mpix_s"] = round(runs["quota"]["mpix_s"], 4)
        out["note"] = (f"this process is capped by a cgroup quota of {quota:g} CPUs, so the {nthreads}-thread run "
                       f"gets at most {quota:g} CPUs of time; full_host_upper_bound_mpix_s assumes perfect scaling "
                       f"of the single-thread rate to all {nthreads} hardware threads")
    return out


# ---------------------------------------------------------------------------- records
def pmc_traffic(scene: str, width: int, height: int, views: int, stripe_step: int,
                lib_hash: str) -> tuple[dict | None, str | None]:
    """The PMC record of this configuration measured with THIS librtx_hip.so (its SHA-256),
    from the newest profiles/r*/pmc_configs.json: HBM bytes per launch of the main render
    kernel and per frame (every render launch of the frame), 2 x FETCH_SIZE + WRITE_SIZE per
    the gfx950 correction of MI355X_MICROARCH.md.  A benchmark process cannot read its own
    counters; a record of any other build is ignored (traffic null)."""
    want = {"scene": scene, "width": width, "height": height, "views": views, "stripe_step": stripe_step}
    for f in sorted(ROOT.glob("profiles/r*/pmc_configs.json"), reverse=True):
        try:
            recs = json.loads(f.read_text())
        except (OSError, ValueError):
            continue
        for r in recs.get("records", []):
            if r.get("config") == want and r.get("lib_sha256") == lib_hash:
                return r, str(f.relative_to(ROOT))
    return None, None


def golden_for(scene: str, width: int, height: int):
    f = GOLDEN / f"config_{scene}_{width}x{height}.npz"
    return (np.load(f), f) if f.exists() else (None, None)


def _channels(p):
    return np.stack([(p >> 16) & 255, (p >> 8) & 255, p & 255], -1).astype(np.int32)


def parity_report(px: np.ndarray, rgb: np.ndarray, scene: str, width: int, height: int, cpu_fnv: str | None = None,
                  exact: bool = True, with_fnv: bool = True) -> dict:
    """Self-check of a rendered frame against the reference's own frame (golden)."""
    g, f = golden_for(scene, width, height)
    out = {}
    if with_fnv:
        out["gpu_fnv"] = fnv1a(px)
        if cpu_fnv:
            out["cpu_fnv"] = cpu_fnv
            out["fnv_match"] = out["gpu_fnv"] == cpu_fnv
    if g is None:
        out["reference"] = None
        return out
    rgb3 = rgb.reshape(-1, 3)
    idx = g["idx"]
    px_ok = sha256(px) == str(g["sha_pixels"][0])
    rgb_ok = sha256(rgb3) == str(g["sha_rgb"][0])
    out.update({"reference": str(f.relative_to(ROOT)), "pixels_sha256_match": px_ok, "rgb_sha256_match": rgb_ok,
                "bit_exact": bool(px_ok and rgb_ok),
                "max_abs": float(np.abs(rgb3[idx] - g["rgb"]).max()),
                "max_lsb": int(np.abs(_channels(px[idx]) - _channels(g["pixels"])).max()),
                "samples": int(idx.size), "tolerance": "max_abs <= 1e-4, <= 1 LSB (north star)"})
    out["within_tolerance"] = bool(out["max_abs"] <= 1e-4 and out["max_lsb"] <= 1 and not np.isnan(rgb3).any())
    out["required"] = "bit_exact" if exact else "within_tolerance (powf in the BRDF)"
    out["ok"] = bool(out["bit_exact"] if exact else out["within_tolerance"])
    return out


DUMP_BUDGET = 48 << 20   # bytes of --dump-outputs over all ranks (under the 64 MB a dump may hold)
DUMP_SEED = 0


def dump_outputs(out_dir: Path, px: np.ndarray, nviews: int, W: int, H: int, rank: int, world: int) -> Path:
    """--dump-outputs: the timed path's last frames as float32 R, G, B (0..255, exact) per pixel,
    `frame.npy` (N = 1) or `frame_rank<r>.npy`, shape (views, H, W, 3).  Frames beyond this
    rank's share of DUMP_BUDGET are cut to a fixed sample of pixels (the same seeded indices
    in every run, sorted), shape (samples, 3)."""
    out_dir.mkdir(parents=True, exist_ok=True)
    rgb = _channels(px).astype(np.float32)
    keep = DUMP_BUDGET // world // 12
    if rgb.shape[0] > keep:
        idx = np.sort(np.random.default_rng(DUMP_SEED).choice(rgb.shape[0], keep, replace=False))
        rgb = rgb[idx]
    else:
        rgb = rgb.reshape(nviews, H, W, 3)
    f = out_dir / ("frame.npy" if world == 1 else f"frame_rank{rank}.npy")
    np.save(f, rgb)
    return f


# ---------------------------------------------------------------------------- one workload
class Workload:
    """One scene x size x mode on this rank's contexts: the timed regions, the algorithmic
    FLOP count, and the gathered frame for the parity check."""

    def __init__(self, ctxs, d: Dist, scene: str, W: int, H: int, mode: str):
        self.ctxs, self.d = ctxs, d
        self.scene, self.W, self.H, self.mode = scene, W, H, mode
        N = d.world
        self.striped = N > 1
        self.hs = HostScene(scene)
        s, cam = self.hs.view()
        for c in ctxs:
            c.upload(s)
        self.cam = cam
        self.nviews = 1 if mode == "frame" else N
        self.views = make_views(cam, self.nviews)
        self.params = abi.make_params(W, H, stripe_rows=16 if self.striped else 0, stripe_first=d.rank,
                                      stripe_step=N)
        self.frame_pixels = self.nviews * W * H   # per step, all ranks together
        self.lib = ctxs[0].lib

    def step(self, i, gather_to=None):
        c = self.ctxs[i % len(self.ctxs)]
        rc = self.lib.rtx_render_views_async(c.h, self.views, self.nviews, C.byref(self.params), 0)
        if rc != abi.RTX_OK:
            abi.check(rc, "rtx_render_views_async", c.h)
        if gather_to is not None:
            c.gather_async(gather_to)

    def sync_all(self):
        for c in self.ctxs:
            c.synchronize()

    def timed(self, fn, k):
        self.d.barrier()
        self.sync_all()
        t0 = time.perf_counter()
        for i in range(k):
            fn(i)
        self.sync_all()
        self.d.barrier()
        return self.d.max(time.perf_counter() - t0)

    def kernel_ms(self, launches: int, ctx=None) -> float:
        """Mean launch time of ONE context's serialized launches (HIP events on its stream)."""
        ms = C.c_float()
        ctx = ctx or self.ctxs[0]
        abi.check(self.lib.rtx_time_views(ctx.h, self.views, self.nviews, C.byref(self.params), launches,
                                          C.byref(ms)), "rtx_time_views", ctx.h)
        return ms.value

    def flop(self) -> tuple[int, int, int, int]:
        """Algorithmic work (SURVEY §8(d) FLOP model, instrumented kernel) of this rank's
        launch and of the whole step over all ranks: (flop, pixels, step flop, step pixels)."""
        N, r = self.d.world, self.d.rank
        counts = np.zeros(12, np.uint64)
        for f in range(self.nviews):
            pv = abi.make_params(self.W, self.H, stripe_rows=16 if self.striped else 0,
                                 stripe_first=(r - f) % N if self.mode == "views" else r, stripe_step=N)
            counts += self.ctxs[0].count_work(self.views[f], pv)
        flop = int(sum(int(c) * w for c, w in zip(counts, COST)))
        pixels = int(counts[0])
        step_flop, step_pixels = self.d.sum_i64([flop, pixels])
        return flop, pixels, step_flop, step_pixels

    def flop_executed(self) -> tuple[int, list]:
        """The same model over the walk the product executes (rtx_count_work_culled: the exact
        cull's pruned, ordered walk, one-piece frame) plus its cull box tests: (flop of this
        rank's launch, the 15 counters)."""
        N, r = self.d.world, self.d.rank
        counts = np.zeros(15, np.uint64)
        for f in range(self.nviews):
            pv = abi.make_params(self.W, self.H, stripe_rows=16 if self.striped else 0,
                                 stripe_first=(r - f) % N if self.mode == "views" else r, stripe_step=N)
            counts += self.ctxs[0].count_work_culled(self.views[f], pv)
        flop = int(sum(int(c) * w for c, w in zip(counts[:12], COST))) + int(counts[14]) * COST_CULL_TEST
        return flop, [int(x) for x in counts]

    def last_frames(self, steps: int) -> np.ndarray:
        """What the last of `steps` timed steps left in HBM, fetched as a caller would
        (rtx_gather_async of the context that rendered it): the packed XRGB pixels of this
        rank's rows of every view, the other ranks' rows zero."""
        c = self.ctxs[(steps - 1) % len(self.ctxs)]
        px = np.zeros(self.nviews * self.W * self.H, np.uint32)
        c.gather_async(px)
        c.synchronize()
        return px

    def run(self, steps: int, warmup: int, launches: int, gather: bool, tag: str, full: bool = True,
            dump_to: Path | None = None) -> dict:
        d, W, H = self.d, self.W, self.H
        # untimed: serialized launches on EVERY context (each context's tile schedule measured and its
        # split threshold tuned before its frames go in flight), which also bring the GPU clock up
        for c in self.ctxs:
            self.kernel_ms(launches, c)
        for i in range(warmup):
            self.step(i)
        self.sync_all()
        elapsed = self.timed(self.step, steps)          # device-resident frames (`value`)
        if dump_to is not None:
            dump_outputs(dump_to, self.last_frames(steps), self.nviews, W, H, d.rank, d.world)
        if not full:
            return {"elapsed": elapsed, "value": self.frame_pixels * steps / elapsed / 1e6,
                    "ms_per_step": elapsed / steps * 1e3}
        # timed after the steps: a fresh process starts the GPU at its idle clock, whose ramp a mean
        # taken first would include ("Short runs and the GPU clock")
        kernel_ms = self.kernel_ms(launches)

        # the same frames gathered into host frames shared by the ranks
        nbytes = self.nviews * W * H * 16   # uint32 pixels + float RGB plane per view (parity)
        shared = None
        if d.rank == 0:
            shared = SharedFrame.create(tag, nbytes)
        d.barrier()
        if d.rank != 0:
            shared = SharedFrame.attach(tag, nbytes)
        d.barrier()
        if d.rank == 0:
            shared.unlink()   # every rank has it mapped: nothing stays behind in /dev/shm
        pinned = shared.pin(self.ctxs[0])
        host_px = shared.view(np.uint32, self.nviews * W * H)
        host_rgb = shared.view(np.float32, 3 * self.nviews * W * H, offset=4 * self.nviews * W * H)
        gathered = None
        if gather:
            for i in range(min(warmup, 10)):
                self.step(i, host_px)
            self.sync_all()
            g_elapsed = self.timed(lambda i: self.step(i, host_px), steps)
            gathered = {"mpix_s": round(self.frame_pixels * steps / g_elapsed / 1e6, 3),
                        "ms_per_step": round(g_elapsed / steps * 1e3, 5), "pinned": bool(pinned),
                        "target": "page-locked host frames (one per view) shared by all ranks (/dev/shm mapping)",
                        "copy": "hipMemcpy2DAsync of the rank's own 16-row stripes (rtx_gather_async)"}
        flop, pixels, step_flop, step_pixels = self.flop()
        # Parity: every rank renders its stripes once more on the timed context (same schedule
        # state), with colours, gathered into the shared host frame; rank 0 checks view 0.
        ctx = self.ctxs[0]
        abi.check(self.lib.rtx_render_views_async(ctx.h, self.views, self.nviews, C.byref(self.params), 1),
                  "rtx_render_views_async", ctx.h)
        ctx.gather_async(host_px, host_rgb)
        ctx.synchronize()
        d.barrier()
        px0 = np.array(host_px[:W * H]) if d.rank == 0 else None
        rgb0 = np.array(host_rgb[:3 * W * H]) if d.rank == 0 else None
        d.barrier()   # nobody unmaps before rank 0 has copied the frame
        del host_px, host_rgb
        shared.close()
        return {"kernel_ms": kernel_ms, "elapsed": elapsed, "gathered": gathered, "flop": flop, "pixels": pixels,
                "step_flop": step_flop, "step_pixels": step_pixels, "px0": px0, "rgb0": rgb0,
                "value": self.frame_pixels * steps / elapsed / 1e6, "ms_per_step": elapsed / steps * 1e3}


def wl_ref_counts(wl: "Workload") -> list:
    """The reference traversal's counters of the workload's rank-0 view (rtx_count_work)."""
    N, r = wl.d.world, wl.d.rank
    pv = abi.make_params(wl.W, wl.H, stripe_rows=16 if wl.striped else 0, stripe_first=r, stripe_step=N)
    return [int(x) for x in wl.ctxs[0].count_work(wl.views[0], pv)]


def stripe_predictor(ctxs, wl: "Workload", lib_hash: str, steps=(2, 4, 8), launches: int = 30) -> dict:
    """One-GPU predictor of strong scaling (N = 1 only): the frame cut into 16-row stripes dealt
    over s ranks, each rank's share timed alone on this GPU (serialized launches, HIP events,
    after a warm-up that builds the share's cost order).  The step time at s GPUs is the slowest
    share's, so efficiency(s) = t_full / (s * max_r t_share(r)); `rank0` uses rank 0's share only.
    `inflight`: the same with the rank's frames in flight as the N-GPU bench runs them (--inflight:
    the rank's contexts alternating frames, wall time per frame over 200 frames after each context's
    serialized warm-up and 200 alternating frames), the full
    frame likewise.  What it leaves out: the host gather and the ranks' clocks (one GPU times every
    share)."""
    ctx = ctxs[0]
    lib = ctx.lib
    cam = wl.views

    def t(p):
        ms = C.c_float()
        # 100 warm-up launches: the share's schedule, split tuner and frontier refinement settle
        abi.check(lib.rtx_time_views(ctx.h, cam, 1, C.byref(p), 100, C.byref(ms)), "rtx_time_views", ctx.h)
        best = None
        for _ in range(2):
            abi.check(lib.rtx_time_views(ctx.h, cam, 1, C.byref(p), launches, C.byref(ms)), "rtx_time_views", ctx.h)
            best = ms.value if best is None else min(best, ms.value)
        return best

    def t_inflight(p, frames=200, warm=200):
        for c in ctxs:   # every context's schedule measured and tuned first, as Workload.run does
            ms = C.c_float()
            abi.check(lib.rtx_time_views(c.h, cam, 1, C.byref(p), 100, C.byref(ms)), "rtx_time_views", c.h)
        for i in range(warm):
            abi.check(lib.rtx_render_views_async(ctxs[i % len(ctxs)].h, cam, 1, C.byref(p), 0), "render", ctx.h)
        for c in ctxs:
            c.synchronize()
        t0 = time.perf_counter()
        for i in range(frames):
            abi.check(lib.rtx_render_views_async(ctxs[i % len(ctxs)].h, cam, 1, C.byref(p), 0), "render", ctx.h)
        for c in ctxs:
            c.synchronize()
        return (time.perf_counter() - t0) / frames * 1e3

    t_full = t(abi.make_params(wl.W, wl.H))
    t_full_if = t_inflight(abi.make_params(wl.W, wl.H))
    out = {"method": f"each share timed alone (rtx_time_views, best of 2 x {launches} launches after 100 warm-up "
                     "launches); efficiency = t_full / (s * slowest share)", "t_full_ms": round(t_full, 5),
           "inflight": {"method": f"each share with {len(ctxs)} frames in flight (the rank's contexts alternating, "
                                  "wall time per frame of 200 frames after 100 serialized launches per context "
                                  "and 200 in flight), the full frame likewise: the "
                                  "N-GPU bench's own mode", "frames_in_flight": len(ctxs),
                        "t_full_ms": round(t_full_if, 5)}}
    for s_ in steps:
        ps = [abi.make_params(wl.W, wl.H, stripe_rows=16, stripe_first=r, stripe_step=s_) for r in range(s_)]
        shares = [t(p) for p in ps]
        shares_if = [t_inflight(p) for p in ps]
        rec, src = pmc_traffic(wl.scene, wl.W, wl.H, 1, s_, lib_hash)
        out[f"s{s_}"] = {"share_ms": [round(x, 5) for x in shares],
                         "efficiency": round(t_full / (s_ * max(shares)), 4),
                         "efficiency_rank0": round(t_full / (s_ * shares[0]), 4),
                         "hbm_bytes_per_frame_rank0": rec.get("hbm_bytes_per_frame") if rec else None,
                         "hbm_source": src}
        out["inflight"][f"s{s_}"] = {"share_ms": [round(x, 5) for x in shares_if],
                                     "efficiency": round(t_full_if / (s_ * max(shares_if)), 4)}
    return out


def roofline(flop: int, kernel_ms: float, rec: dict | None, src: str | None) -> dict:
    achieved = flop / (kernel_ms * 1e-3) / 1e12 if kernel_ms > 0 else 0.0
    out = {"bound": "valu", "achieved": round(achieved, 4), "peak": FP32_PEAK_TFLOPS, "unit": "TFLOP/s",
           "frac": round(achieved / FP32_PEAK_TFLOPS, 5)}
    traffic = rec["hbm_bytes_per_launch"] if rec else None
    frame_traffic = rec.get("hbm_bytes_per_frame") if rec else None
    out.update({"traffic": traffic, "traffic_unit": "bytes/launch (HBM, PMC, main render kernel)",
                "traffic_source": src,
                "traffic_note": None if rec else "no PMC record of this librtx_hip.so build for this configuration",
                "hbm_bytes_per_frame": frame_traffic,
                "hbm_gbs": round(traffic / (kernel_ms * 1e-3) / 1e9, 2) if traffic and kernel_ms > 0 else None,
                # north star: the HBM roofline fraction, reported beside the VALU one
                "hbm_frac": round(traffic / (kernel_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5)
                if traffic and kernel_ms > 0 else None,
                "kernel_ms": round(kernel_ms, 5)})
    return out


def parity_configs(dev: int) -> list[dict]:
    """Every BASELINE config (+ W4_Reference, W4_Optional) at full size on a fresh context:
    PARITY_FRAMES frames (frame 1 measures tile costs, later ones run cost-ordered and split),
    the last one checked against the reference's frame."""
    out = []
    for scene, W, H, exact in PARITY_CONFIGS:
        ctx = DeviceContext(dev)
        try:
            hs = HostScene(scene)
            s, cam = hs.view()
            ctx.upload(s)
            p = abi.make_params(W, H)
            for _ in range(PARITY_FRAMES - 1):
                ctx.render_async(cam, p)
            px, rgb = ctx.render(cam, p)
            heavy = ctx.split_info()[0]
            rep = parity_report(px, rgb, scene, W, H, exact=exact, with_fnv=False)
            out.append({"config": f"{scene} {W}x{H}", "frames": PARITY_FRAMES, "heavy_tiles_split": heavy, **rep})
        finally:
            ctx.close()
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--scene", default="W4_Bunny")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--mode", choices=["frame", "views"], default="views",
                    help="frame: one frame per step tiled over the ranks (strong); views: N views per step (weak)")
    ap.add_argument("--cpu-frames", type=int, default=8)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-gather", action="store_true", help="skip the host-gather timed region")
    ap.add_argument("--no-extra", action="store_true", help="headline only: no multi_gpu_configs / parity_configs")
    ap.add_argument("--inflight", type=int, default=2, help="frames in flight (render contexts per GPU)")
    ap.add_argument("--inflight-frame", type=int, default=3,
                    help="frames in flight for the one-frame-per-step workloads (multi_gpu_configs)")
    ap.add_argument("--full", action="store_true",
                    help="everything beside the headline: roofline (kernel time, FLOP count, PMC traffic), host "
                         "gather, parity, end-to-end frame, multi_gpu_configs, parity_configs, cpu_baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", type=Path, default=None,
                    help="write the frames of the last timed step to DIR/frame.npy (float32 R, G, B per pixel)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    # RTX_BENCH_DEVICE pins every rank to one device: rehearsing the N-rank path on a one-GPU
    # machine (the driver's multi-GPU runs leave it unset: rank r -> device LOCAL_RANK)
    dev = int(os.environ.get("RTX_BENCH_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    ctxs = [DeviceContext(dev) for _ in range(max(1, args.inflight))]
    d = Dist()
    N = d.world
    if args.gpus != N and d.rank == 0:
        print(f"warning: --gpus {args.gpus} but WORLD_SIZE={N}; using {N}", file=sys.stderr)
    lib_hash = lib_sha256()
    tag = f"{os.environ.get('MASTER_PORT', 'solo')}_{os.getuid()}_{os.getppid() if N > 1 else os.getpid()}"
    W, H = args.width, args.height

    # ---- 1. headline
    hw = Workload(ctxs, d, args.scene, W, H, args.mode)
    hr = hw.run(args.steps, args.warmup, K_KERNEL_LAUNCHES, not args.no_gather, tag + "_h", full=args.full,
                dump_to=args.dump_outputs)
    strong = args.mode == "frame"
    out = {
        "metric": "Mpixels/s (primary+shadow rays) at 1920x1080; per-channel max-abs vs CPU ref",
        "value": round(hr["value"], 3),
        "unit": "Mpixels/s",
        "n_gpus": N,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(hr["ms_per_step"], 5),
        "higher_is_better": True,
        "scaling": "strong" if strong else "weak",
        "vs_baseline": None,
        "dtype": "f32",
        "data": f"synthetic: the reference's {args.scene} scene (Initialize state) built by the host scene layer; "
                "no datasets",
        "config": {"workload": (f"{args.scene} {W}x{H}, Combined lighting, shadows on, one frame per step"
                                if N == 1 else
                                f"{args.scene} {W}x{H}, Combined lighting, shadows on, one frame per step tiled "
                                f"over {N} ranks in 16-row stripes" if strong else
                                f"{args.scene} {W}x{H}, Combined lighting, shadows on, {N} views per step, each "
                                f"tiled over the {N} ranks in 16-row stripes"),
                   "scene": args.scene, "width": W, "height": H, "views_per_step": hw.nviews,
                   "stripe_rows": 16 if N > 1 else 0,
                   "parallelism": f"image stripes x{N} (no collective)", "frames_in_flight": len(ctxs)},
        "full": args.full,
    }
    if not args.full:
        # the plain run: the headline and nothing that takes a run of its own
        if d.rank == 0:
            print(json.dumps(out), flush=True)
        for c in ctxs:
            c.close()
        d.close()
        return 0

    # End-to-end single frame through the blocking C-ABI entry into pageable memory (N = 1).
    e2e = None
    if N == 1:
        host = np.zeros(W * H, np.uint32)
        p1 = abi.make_params(W, H)
        ts = []
        for _ in range(10):
            t1 = time.perf_counter()
            abi.check(hw.lib.rtx_render(ctxs[0].h, C.byref(hw.cam), C.byref(p1),
                                        host.ctypes.data_as(C.POINTER(C.c_uint32)), None), "rtx_render", ctxs[0].h)
            ts.append(time.perf_counter() - t1)
        e2e = W * H / float(np.median(ts)) / 1e6

    # ---- 2. the north star's multi-GPU workloads, one image per step tiled over the N ranks
    multi = []
    # the one-frame-per-step workloads keep --inflight-frame frames in flight (3: a frame's slowest
    # tile overlaps two other frames; profiles/r06/bench_inflight3.json: W4_Optional 14.9k -> 17.3k,
    # Synthetic100k 3.4k -> 4.0k Mpix/s; 4 contexts share hardware queues and lose)
    fctxs = ctxs + [DeviceContext(dev) for _ in range(max(0, args.inflight_frame - len(ctxs)))]
    fctxs = fctxs[:max(1, args.inflight_frame)]
    if not args.no_extra:
        for scene, mw, mh, msteps in MULTI_GPU_CONFIGS:
            wl = Workload(fctxs, d, scene, mw, mh, "frame")
            # (150 warm-up steps: the contexts' in-flight probe, rtx_inflight_info, settles in ~130)
            r = wl.run(msteps, 150, 100, not args.no_gather, f"{tag}_{scene}")
            rec, src = pmc_traffic(scene, mw, mh, 1, N, lib_hash)
            # every rank's HBM rate over its own launches (the PMC record is rank 0's stripes)
            per_rank = d.gather([r["kernel_ms"], r["flop"]])
            entry = {"config": f"{scene} {mw}x{mh}, one frame per step tiled over {N} rank(s) in 16-row stripes",
                     "scene": scene, "width": mw, "height": mh, "n_gpus": N, "steps": msteps,
                     "frames_in_flight": len(fctxs),
                     "mpix_s": round(r["value"], 3), "ms_per_step": round(r["ms_per_step"], 5),
                     "gathered_mpix_s": r["gathered"]["mpix_s"] if r["gathered"] else None,
                     "roofline_rank0": roofline(r["flop"], r["kernel_ms"], rec, src),
                     "per_rank_kernel_ms": [round(float(x), 5) for x in per_rank[:, 0]],
                     "per_rank_tflops": [round(float(f) / (float(k) * 1e-3) / 1e12, 3) if k > 0 else None
                                         for k, f in per_rank],
                     "hbm_per_rank": None, "frame_flop_all_ranks": r["step_flop"],
                     "frame_pixels_counted": r["step_pixels"]}
            if rec:
                entry["hbm_per_rank"] = [
                    {"gbs": round(rec["hbm_bytes_per_launch"] / (float(k) * 1e-3) / 1e9, 2),
                     "frac": round(rec["hbm_bytes_per_launch"] / (float(k) * 1e-3) / 1e9 / HBM_PEAK_GBS, 5)}
                    for k in per_rank[:, 0]]
                entry["hbm_note"] = ("rank 0's PMC bytes per launch over each rank's own launch time (ranks render "
                                     "equal shares of 16-row stripes)")
            if ctxs[0].cull_info()[0]:
                # The exact cull proves most of the reference traversal's slab and
                # triangle tests unnecessary and skips them, so `achieved` / `frac` count the work the
                # culled walk EXECUTES (rtx_count_work_culled); the model's FLOP of the reference's own
                # traversal over the same time is kept beside it as *_reference_equivalent.
                rr = entry["roofline_rank0"]
                fx, cx = wl.flop_executed()
                ach = fx / (r["kernel_ms"] * 1e-3) / 1e12 if r["kernel_ms"] > 0 else 0.0
                ref_counts = wl_ref_counts(wl)
                rr.update({
                    "achieved_reference_equivalent": rr["achieved"], "frac_reference_equivalent": rr["frac"],
                    "achieved": round(ach, 4), "frac": round(ach / FP32_PEAK_TFLOPS, 5),
                    "flop_per_launch": fx, "flop_reference_per_launch": r["flop"],
                    "flop_basis": ("executed: SURVEY §8(d) costs over the slab / triangle / cull-box tests the culled "
                                   "ordered walk performs (rtx_count_work_culled, one-piece frame: the split "
                                   "launches' repeated path tests are not counted) + 23 FLOP per cull box test; "
                                   "*_reference_equivalent: the model's FLOP of the reference's full traversal over "
                                   "the same time, an effective rate"),
                    "executed_vs_reference": {"slab_tests": round(cx[3] / max(1, ref_counts[3]), 4),
                                              "triangle_tests": round(cx[4] / max(1, ref_counts[4]), 4),
                                              "cull_box_tests": cx[14]}})
            if d.rank == 0:
                exact = next((x for sc, w_, h_, x in PARITY_CONFIGS if (sc, w_, h_) == (scene, mw, mh)), True)
                entry["parity"] = parity_report(r["px0"], r["rgb0"], scene, mw, mh, exact=exact, with_fnv=False)
            if N == 1:
                entry["strong_scaling_predictor"] = stripe_predictor(fctxs, wl, lib_hash)
            multi.append(entry)

    # ---- 3. parity of every config at full size (N = 1; one rank per GPU renders stripes at N > 1)
    pconf = parity_configs(dev) if (N == 1 and not args.no_extra) else None

    # ---- 4. CPU reference on this host, same run (rank 0, N = 1)
    cpu = None
    if d.rank == 0 and N == 1 and not args.no_cpu_baseline:
        ref = CpuReference()
        try:
            cpu = cpu_baseline(ref, args.scene, W, H, args.cpu_frames)
            nthreads = len(os.sched_getaffinity(0))
            for entry in multi:   # one frame of each multi-GPU workload, all threads
                try:
                    cr = ref.run(entry["scene"], entry["width"], entry["height"], nthreads, 1)
                    entry["cpu_reference_mpix_s"] = round(cr["mpix_s"], 4)
                    entry["speedup_vs_cpu"] = round(entry["mpix_s"] / cr["mpix_s"], 1)
                except Exception as e:   # noqa: BLE001
                    entry["cpu_reference_mpix_s"] = f"failed: {e}"
        except Exception as e:   # the baseline must not take the headline down
            cpu = {"value": None, "unit": "Mpixels/s", "cores": 0, "kind": ref.kind, "sample": f"failed: {e}"}
        finally:
            ref.close()

    parity = None
    if d.rank == 0:
        # view 0 is the reference camera: the frame the goldens were made from
        parity = {"frame": "the host-gathered frame of the timed contexts (cost-ordered / split state)",
                  **parity_report(hr["px0"], hr["rgb0"], args.scene, W, H, cpu.get("fnv") if cpu else None)}

    rec, src = pmc_traffic(args.scene, W, H, hw.nviews, N, lib_hash)
    roof = roofline(hr["flop"], hr["kernel_ms"], rec, src)
    roof.update({"kernel": "rtx_render_kernel<false, 0, false, SPEC> (the specialised variant the scene's facts "
                           "select; + split phases 1-3 when tiles are heavy)",
                 "kernel_launches": K_KERNEL_LAUNCHES, "flop_per_launch": hr["flop"],
                 "pixels_per_launch": hr["pixels"], "flop_per_pixel": round(hr["flop"] / max(hr["pixels"], 1), 2),
                 "frame_flop_all_ranks": hr["step_flop"], "frame_pixels_counted": hr["step_pixels"],
                 "lib_sha256": lib_hash,
                 "note": "FP32 VALU-bound path (no dense contraction, 4 B/pixel of HBM output); "
                         "FLOP = SURVEY §8(d) algorithmic model counted by the instrumented kernel; "
                         "kernel_ms/achieved are rank 0's launches (mean of kernel_launches serialized launches, "
                         "timed after the timed steps, the clock up)"})
    out.update({
        "roofline": roof,
        "cpu_baseline": cpu,
        "parity": parity,
        "host_gather": hr["gathered"],
        "end_to_end_mpix_s": round(e2e, 3) if e2e else None,
        "multi_gpu_configs": multi,
        "parity_configs": pconf,
    })
    if pconf is not None:
        out["parity_configs_all_ok"] = all(p.get("ok", False) for p in pconf)
    if cpu and cpu.get("value"):
        out["speedup_vs_cpu"] = round(hr["value"] / cpu["value"], 1)
        if cpu.get("full_host_upper_bound_mpix_s"):
            out["speedup_vs_cpu_full_host_upper_bound"] = round(hr["value"] / cpu["full_host_upper_bound_mpix_s"], 1)
    if d.rank == 0:
        print(json.dumps(out), flush=True)
    for c in {id(c): c for c in ctxs + fctxs}.values():
        c.close()
    d.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
