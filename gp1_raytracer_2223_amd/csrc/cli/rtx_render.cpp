// rtx_render — headless C++ host program (the reference's main.cpp frame loop without
// the SDL window): builds a catalogue scene with librtx_host.so, renders it through the
// C-ABI of librtx_hip.so and writes RayTracing_Buffer.bmp like the reference's X key.
//
//   rtx_render <scene> [width height] [--time T] [--mode 0..3] [--no-shadows]
//              [--frames N] [--out file.bmp] [--assets dir] [--benchmark [windows]] [--inflight F]
//              [--device-update] [--ss K] [--aov PREFIX] [--rays FILE] [--adaptive K,T] [--deferred] [--relight]
//              [--resolve K] [--move-light L,X,Y,Z]... [--in-place]
//
// --benchmark runs the reference's frame loop (main.cpp:86-100: Scene::Update with the
// timer's total time, Render into the host pixel buffer, Timer::Update) under its F6
// benchmark (Timer.cpp:44-131): `windows` one-second dFPS windows (default 10), then
// ">> HIGH/LOW/AVG" on stdout and benchmark.txt in the reference's format.  Animated
// scenes are re-uploaded after every Update; the per-stage means are printed as well.
// --inflight F (default 2) overlaps F frames (run_benchmark); 1 = the serial loop.
// --ss K (1, 2, 4 or 8; default 1) renders K x K samples per pixel (rtx_set_supersample).
// --aov PREFIX (single frames only, not --benchmark / --sequence, and not with --ss above 1) also runs
// the hit pass of the frame it rendered (rtx_render_aov) and writes its planes as raw little-endian
// files: PREFIX_depth.f32, PREFIX_normal.f32 (3 floats per pixel), PREFIX_material.u32 and
// PREFIX_primitive.u32 (kind << 30 | index), row-major width x height.
// --rays FILE (single frames only: not with --benchmark, --sequence, --aov or --ss above 1) shades the
// image from the caller's rays instead of the camera's (rtx_shade_rays): FILE is raw little-endian
// float32, width x height rays of eight floats {origin, direction, tmin, tmax}, row-major.
// --adaptive K,T (single frames only: not with --benchmark, --sequence, --aov, --rays or --ss above 1) renders
// the frame with adaptive supersampling (rtx_render_adaptive): K x K samples (K = 2, 4 or 8) for the pixels
// that differ from a 4-neighbour by more than T (0..255) in an 8-bit channel, and prints how many that was.
// --deferred (single frames only: not with --benchmark, --sequence, --rays, --adaptive or --ss above 1) makes the
// image from one hit pass plus deferred shading (rtx_render_aov, rtx_shade_aov) instead of a frame: the same
// BMP, and with --aov the same planes, from one primary traversal.
// --relight (single frames only, and not with --deferred: the combinations --deferred refuses) makes the image from
// one hit pass, its shadow pass and a relight (rtx_render_aov, rtx_render_shadows_async, rtx_relight): the same BMP;
// with --aov also PREFIX_shadow.u32, one word per pixel whose bit l says light l is occluded.
// --resolve K (K = 2, 4 or 8; only with --relight, and not with --aov) makes the W x H image anti-aliased from stored
// passes: the hit pass and the shadow pass run at K*W x K*H and the resolved relight (rtx_relight_resolve) shades
// every stored sample and box-filters each pixel's K x K: the same BMP as the plain run with --ss K.  --move-light
// works as with plain --relight, the refresh running at sample size.
// --move-light L,X,Y,Z (repeatable) sets light L's origin to (X, Y, Z) before anything is uploaded, for any run.
// With --relight the hit pass and the full shadow pass run with the scene's ORIGINAL lights; then the moved scene is
// uploaded, rtx_refresh_shadows_async re-traces only the moved lights, and the relight makes the image: the same
// BMP as the plain run with the same moves, and with --aov the refreshed PREFIX_shadow.u32.
// --in-place (only with --relight and --move-light) makes the move an edit of the uploaded scene (rtx_edit_lights)
// instead of a second upload; the refresh and the image are the same.
#include <algorithm>
#include <array>
#include <cfloat>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <memory>
#include <numeric>
#include <string>
#include <utility>
#include <vector>

#include <sys/resource.h>

#include "benchmark.h"
#include "rtx_renderer.hpp"

namespace {

using Clock = std::chrono::steady_clock;
double secs(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }
double cpu_secs() {   // the process's CPU time, every thread (user + system)
    rusage u{};
    getrusage(RUSAGE_SELF, &u);
    return double(u.ru_utime.tv_sec + u.ru_stime.tv_sec) + 1e-6 * double(u.ru_utime.tv_usec + u.ru_stime.tv_usec);
}

// The pipelined host side of run_benchmark.  The reference's BuildBVH permutes the triangles in
// place (DataTypes.h:335-363), so the state Update k leaves depends on every earlier Update: ONE
// chain scene is updated serially, on a worker thread, and after Update k its state is copied into
// snapshot k % D (rtx_host_scene_copy_state), which the main thread uploads.  The worker runs up to D
// frames ahead of the uploads: Update k + 1 overlaps frame k's upload and the GPU's frames, and only
// the snapshot copy waits for its slot.  time_of(k) gives frame k's Update time (taken when that
// Update starts); `limit` (>= 0) stops the worker after that many frames.
class ChainUpdater {
public:
    ChainUpdater(rtx_host_scene* chain, std::vector<rtx_host_scene*> snaps, std::function<float(long)> time_of,
                 long limit)
        : chain_(chain), snaps_(std::move(snaps)), time_of_(std::move(time_of)), limit_(limit),
          th_([this] { Loop(); }) {}
    ~ChainUpdater() {
        {
            std::lock_guard<std::mutex> l(m_);
            quit_ = true;
        }
        cv_.notify_all();
        th_.join();
    }
    // frame k's snapshot, once Update k has been copied into it (nullptr if the worker failed)
    rtx_host_scene* wait(long k) {
        std::unique_lock<std::mutex> l(m_);
        cv_.wait(l, [&] { return ready_ > k || failed_; });
        return failed_ ? nullptr : snaps_[k % snaps_.size()];
    }
    // frame k's upload has returned (the upload copied the arrays): its snapshot may be overwritten
    void release(long k) {
        std::lock_guard<std::mutex> l(m_);
        released_ = std::max(released_, k + 1);
        cv_.notify_all();
    }

private:
    void Loop() {
        const long D = static_cast<long>(snaps_.size());
        for (long k = 0;; ++k) {
            {
                std::lock_guard<std::mutex> l(m_);
                if (quit_ || (limit_ >= 0 && k >= limit_)) return;
            }
            rtx_host_scene_update(chain_, time_of_(k));   // Scene::Update, in the reference's order
            std::unique_lock<std::mutex> l(m_);
            cv_.wait(l, [&] { return quit_ || k < released_ + D; });
            if (quit_) return;
            l.unlock();
            const int rc = rtx_host_scene_copy_state(snaps_[k % D], chain_);
            l.lock();
            if (rc != RTX_OK) failed_ = true;
            ready_ = k + 1;
            cv_.notify_all();
            if (failed_) return;
        }
    }
    rtx_host_scene* chain_;
    std::vector<rtx_host_scene*> snaps_;
    std::function<float(long)> time_of_;
    long limit_;
    std::mutex m_;
    std::condition_variable cv_;
    long ready_ = 0, released_ = 0;
    bool quit_ = false, failed_ = false;
    std::thread th_;   // (last: started after the members above)
};

// The reference's frame loop is serial: Update, Render (into the window surface), present.
// Here `inflight` frames overlap: frame k is updated, uploaded and queued (render + D2H into
// its own page-locked host frame) on context k % inflight while frame k - 1 still runs on
// another context's stream, so the host's Update / BVH rebuild of the next frame hides
// behind the current frame's GPU work.  Every frame is still fully rendered and in host
// memory before it counts: the benchmark ticks when frame k's context has finished.
// inflight = 1 is the reference's serial loop.
// With frames in flight and more host scenes of the same catalogue scene (`extra`, D of them) the
// host side is pipelined too (ChainUpdater): `hs` is updated serially on a worker thread, one
// Update history as in the reference's loop, and each frame's state is uploaded from a snapshot
// (one of the D extra scenes) while the worker goes on with the next Updates (an upload copies the
// host arrays into page-locked staging before it returns, so the snapshot is free again after it).
// A frame's time is taken when its Update starts.
// --device-update: the animated meshes' Update (transform + BVH rebuild + scene image) runs on
// the device (rtx_anim_*); the host only computes the frame's transforms.
// With `seq` (--sequence t1,t2,...): no timer; frame k is Update(seq[k]) and is written to
// `<stem>_<k>.bmp` when it completes (the pipelined loop's frames, checked by the tests).
int run_benchmark(rtx::Renderer& r, rtx_host_scene* hs, int windows, int inflight, bool device_update,
                  const std::vector<float>* seq = nullptr, const std::string& stem = "",
                  const std::vector<rtx_host_scene*>& extra = {}, uint32_t ss = 1) {
    const bool animated = rtx_host_scene_animated(hs) == 1;
    // (pipelined host side) D = the snapshot scenes: `hs` is the chain the worker updates, frame k is
    // uploaded from snapshot extra[k % D]
    const int D = (animated && !device_update && inflight >= 2) ? static_cast<int>(extra.size()) : 0;
    const bool pipe = D > 0;
    const size_t npx = static_cast<size_t>(r.Width()) * r.Height();
    std::vector<rtx_ctx*> ctx{r.Context()};
    for (int f = 1; f < inflight; ++f) {
        rtx_ctx* c = nullptr;
        if (rtx_create(&c, 0) != RTX_OK) {
            std::fprintf(stderr, "rtx_create: %s\n", rtx_last_error(nullptr));
            for (size_t i = 1; i < ctx.size(); ++i) rtx_destroy(ctx[i]);
            return 1;
        }
        rtx_set_supersample(c, ss);   // (main checked the factor)
        ctx.push_back(c);
    }
    std::vector<std::vector<uint32_t>> buf(inflight, std::vector<uint32_t>(npx));
    std::vector<char> upd_ok(inflight, 1);   // --sequence: the device Update of the frame in buf[f] succeeded
    for (int f = 0; f < inflight; ++f) rtx_host_register(ctx[f], buf[f].data(), npx * 4);   // async D2H
    const rtx_render_params p = r.Params();
    rtx::Benchmark b(windows);
    if (!seq) std::cout << "**BENCHMARK STARTED**\n";
    double t_update = 0, t_upload = 0, t_queue = 0, t_wait = 0;
    long frames = 0, queued = 0;
    int rc = 0, last = -1;
    const Clock::time_point start = Clock::now();
    const double cpu0 = cpu_secs();
    Clock::time_point prev = start;
    std::unique_ptr<ChainUpdater> chain;
    if (pipe)
        chain.reset(new ChainUpdater(
            hs, extra, [&](long k) { return seq ? (*seq)[k] : static_cast<float>(secs(start, Clock::now())); },
            seq ? static_cast<long>(seq->size()) : -1));
    rtx_scene s;
    rtx_camera cam;
    auto ok = [&](int code, const char* what, rtx_ctx* c) {
        if (code == RTX_OK) return true;
        std::fprintf(stderr, "%s: %s\n", what, rtx_last_error(c));
        rc = 1;
        return false;
    };
    // device-side Update: register the scene's turning meshes on the first context
    rtx_anim* anim = nullptr;
    std::vector<float> mats;
    int n_anim = 0;
    // every registered mesh's device Update status (NaN vertex, a tree too deep to render)
    auto anim_ok = [&]() {
        for (int i = 0; i < n_anim; ++i) {
            uint32_t st[4];
            if (rtx_anim_status(anim, static_cast<uint32_t>(i), st) != RTX_OK) {
                std::fprintf(stderr, "device Update failed (registered mesh %d): %s\n", i, rtx_anim_last_error(anim));
                return false;
            }
        }
        return true;
    };
    if (device_update && animated) {
        std::vector<int32_t> ids(64);
        const int ns = rtx_host_scene_spinning(hs, ids.data(), static_cast<uint32_t>(ids.size()));
        if (ns > static_cast<int>(ids.size())) {   // rtx_anim_create takes at most 32 anyway
            std::fprintf(stderr, "--device-update: %d turning meshes, more than %zu\n", ns, ids.size());
            for (size_t i = 1; i < ctx.size(); ++i) rtx_destroy(ctx[i]);
            return 1;
        }
        n_anim = ns;
        std::vector<rtx_mesh_source> src(ns > 0 ? ns : 0);
        for (int i = 0; i < ns; ++i) rtx_host_scene_mesh_source(hs, static_cast<uint32_t>(ids[i]), &src[i]);
        rtx_host_scene_view(hs, &s, &cam);
        if (ns <= 0 || rtx_anim_create(&anim, ctx[0], &s, ids.data(), src.data(), static_cast<uint32_t>(ns)) != RTX_OK) {
            std::fprintf(stderr, "rtx_anim_create: %s\n", rtx_anim_last_error(nullptr));
            for (size_t i = 1; i < ctx.size(); ++i) rtx_destroy(ctx[i]);
            return 1;
        }
        mats.resize(16 * static_cast<size_t>(ns));
    }
    for (;;) {
        const int f = static_cast<int>(queued % inflight);
        if (queued >= inflight) {   // frame queued - inflight (this context's) completes
            const Clock::time_point w0 = Clock::now();
            if (!ok(rtx_synchronize(ctx[f]), "rtx_synchronize", ctx[f])) break;
            const Clock::time_point w1 = Clock::now();
            t_wait += secs(w0, w1);
            ++frames;
            last = f;
            const float elapsed = static_cast<float>(secs(prev, w1));                  // Timer::Update
            prev = w1;
            if (seq) {
                if (anim && !upd_ok[f]) { rc = 1; break; }   // never write a frame of a failed Update
                r.Pixels() = buf[f];
                if (!r.SaveBufferToImage(stem + "_" + std::to_string(frames - 1) + ".bmp")) { rc = 1; break; }
                if (frames == static_cast<long>(seq->size())) break;
            } else if (b.Tick(elapsed)) {
                break;
            }
        }
        if (seq && queued >= static_cast<long>(seq->size())) {   // drain: nothing left to queue
            ++queued;
            continue;
        }
        const Clock::time_point f0 = Clock::now();
        const float tnow = seq ? (*seq)[queued] : static_cast<float>(secs(start, f0));
        rtx_host_scene* cur = hs;
        if (pipe) {
            cur = chain->wait(queued);   // frame `queued`'s Update (the worker's chain), in its snapshot
            if (!cur) {
                std::fprintf(stderr, "rtx_host_scene_copy_state failed\n");
                rc = 1;
                break;
            }
        } else if (anim) {
            rtx_host_scene_transforms(hs, tnow, mats.data(), static_cast<uint32_t>(n_anim));   // Update(t)'s turn
        } else if (animated) {
            rtx_host_scene_update(hs, tnow);                // Scene::Update
        }
        const Clock::time_point f1 = Clock::now();
        if (!ok(rtx_host_scene_view(cur, &s, &cam), "rtx_host_scene_view", nullptr)) break;
        if (anim) {
            if (rtx_anim_update(anim, ctx[f], mats.data()) != RTX_OK) {
                std::fprintf(stderr, "rtx_anim_update: %s\n", rtx_anim_last_error(anim));
                rc = 1;
                break;
            }
            // --sequence: this Update's own status, read now (the status words are the newest
            // Update's, so with frames in flight a later one would overwrite a failure); the
            // frame is written only if it is clean.  The benchmark loop checks once at the end.
            if (seq) upd_ok[f] = anim_ok();
        } else if ((animated || queued < inflight) && !ok(rtx_upload_scene(ctx[f], &s), "rtx_upload_scene", ctx[f])) {
            break;
        }
        if (pipe) chain->release(queued);   // the upload copied the snapshot's arrays
        const Clock::time_point f2 = Clock::now();
        if (!ok(rtx_render_async(ctx[f], &cam, &p, 0), "rtx_render_async", ctx[f])) break;  // Renderer::Render
        if (!ok(rtx_gather_async(ctx[f], buf[f].data(), nullptr), "rtx_gather_async", ctx[f])) break;
        const Clock::time_point f3 = Clock::now();
        t_update += secs(f0, f1);
        t_upload += secs(f1, f2);
        t_queue += secs(f2, f3);
        ++queued;
    }
    for (int f = 0; f < inflight; ++f) rtx_synchronize(ctx[f]);
    chain.reset();   // (stops the worker after its current Update)
    if (anim) {
        if (!anim_ok()) rc = 1;
        rtx_anim_destroy(anim);
    }
    if (last >= 0) r.Pixels() = buf[last];   // the last completed frame (SaveBufferToImage)
    for (int f = 0; f < inflight; ++f) rtx_host_unregister(ctx[f], buf[f].data());
    for (size_t i = 1; i < ctx.size(); ++i) rtx_destroy(ctx[i]);
    if (rc || seq) return rc;
    rtx::WriteBenchmark(b);
    const double n = static_cast<double>(queued);
    // host CPU use of the loop: process CPU time (the build pool's spinning workers included) over
    // wall time, in cores
    const double cores = (cpu_secs() - cpu0) / std::max(1e-9, secs(start, Clock::now()));
    std::printf("frames %ld%s%s, %d in flight: per frame update %.3f ms, upload %.3f ms, queue %.3f ms, "
                "wait for GPU %.3f ms, host CPU %.2f cores\n", frames, animated ? " (animated)" : "",
                device_update ? " device Update" : "", inflight, t_update / n * 1e3,
                t_upload / n * 1e3, t_queue / n * 1e3, t_wait / std::max(1.0, double(frames)) * 1e3, cores);
    return 0;
}

// One plane of --aov as a raw file (the hosts this builds for are little-endian).
template <class T>
bool write_plane(const std::string& path, const std::vector<T>& v) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = std::fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
    return std::fclose(f) == 0 && ok;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <scene> [width height] [--time T] [--mode M] [--no-shadows] [--frames N] "
                             "[--out f.bmp] [--assets dir] [--benchmark [windows]] [--inflight F] [--device-update] [--ss K] "
                             "[--aov prefix] [--rays file] [--adaptive K,T] [--deferred] [--relight] [--resolve K] "
                             "[--move-light L,X,Y,Z]... [--in-place]\n",
                     argv[0]);
        return 2;
    }
    std::string scene = argv[1], out = "RayTracing_Buffer.bmp", assets, aov, rays_file;
    int W = 640, H = 480, mode = 3, frames = 1, bench = 0, inflight = 2, ss = 1;
    int ad_k = 0, ad_t = 0;   // --adaptive K,T (0: not asked for)
    int resolve = 0;          // --resolve K (0: not asked for)
    std::vector<float> seq;
    float t = -1.f;
    bool shadows = true, device_update = false, deferred = false, relight = false, in_place = false;
    std::vector<std::pair<uint32_t, std::array<float, 3>>> moves;   // --move-light, in the order given
    int pos = 0;
    for (int i = 2; i < argc; ++i) {
        std::string a = argv[i];
        if (a == "--time" && i + 1 < argc) t = std::strtof(argv[++i], nullptr);
        else if (a == "--mode" && i + 1 < argc) mode = std::atoi(argv[++i]);
        else if (a == "--no-shadows") shadows = false;
        else if (a == "--frames" && i + 1 < argc) frames = std::atoi(argv[++i]);
        else if (a == "--sequence" && i + 1 < argc) {
            for (const char* q = argv[++i]; *q;) {
                char* e = nullptr;
                seq.push_back(std::strtof(q, &e));
                q = (*e == ',') ? e + 1 : e;
                if (e == q && *q) break;
            }
        }
        else if (a == "--inflight" && i + 1 < argc) inflight = std::max(1, std::min(8, std::atoi(argv[++i])));
        else if (a == "--device-update") device_update = true;
        else if (a == "--deferred") deferred = true;
        else if (a == "--relight") relight = true;
        else if (a == "--in-place") in_place = true;
        else if (a == "--ss") {   // checked here: a bad factor ends the program before any device work
            ss = i + 1 < argc ? std::atoi(argv[++i]) : 0;
            if (ss != 1 && ss != 2 && ss != 4 && ss != 8) {
                std::fprintf(stderr, "--ss: the supersample factor must be 1, 2, 4 or 8\n");
                return 2;
            }
        }
        else if (a == "--resolve") {   // checked here: a bad factor ends the program before any device work
            char tail = 0;
            const int got = i + 1 < argc ? std::sscanf(argv[++i], "%d%c", &resolve, &tail) : 0;
            if (got != 1 || (resolve != 2 && resolve != 4 && resolve != 8)) {
                std::fprintf(stderr, "--resolve K: the factor K must be 2, 4 or 8\n");
                return 2;
            }
        }
        else if (a == "--adaptive") {   // checked here: a bad pair ends the program before any device work
            char tail = 0;
            const int got = i + 1 < argc ? std::sscanf(argv[++i], "%d,%d%c", &ad_k, &ad_t, &tail) : 0;
            if (got != 2 || (ad_k != 2 && ad_k != 4 && ad_k != 8) || ad_t < 0 || ad_t > 255) {
                std::fprintf(stderr, "--adaptive K,T: the factor K must be 2, 4 or 8 and the threshold T 0..255\n");
                return 2;
            }
        }
        else if (a == "--move-light") {   // checked here: a malformed move ends the program before any device work
            int l = -1;
            std::array<float, 3> o{};
            char tail = 0;
            const int got = i + 1 < argc ? std::sscanf(argv[++i], "%d,%f,%f,%f%c", &l, &o[0], &o[1], &o[2], &tail) : 0;
            if (got != 4 || l < 0) {
                std::fprintf(stderr, "--move-light L,X,Y,Z: a light index (0 or above) and three coordinates\n");
                return 2;
            }
            moves.push_back({static_cast<uint32_t>(l), o});
        }
        else if (a == "--out" && i + 1 < argc) out = argv[++i];
        else if (a == "--aov" && i + 1 < argc) aov = argv[++i];
        else if (a == "--rays" && i + 1 < argc) rays_file = argv[++i];
        else if (a == "--assets" && i + 1 < argc) assets = argv[++i];
        else if (a == "--benchmark") bench = (i + 1 < argc && std::atoi(argv[i + 1]) > 0) ? std::atoi(argv[++i]) : 10;
        else if (pos == 0) { W = std::atoi(argv[i]); ++pos; }
        else if (pos == 1) { H = std::atoi(argv[i]); ++pos; }
    }
    if (deferred && (bench || !seq.empty() || !rays_file.empty() || ad_k || ss > 1)) {   // before any device work
        std::fprintf(stderr, "--deferred shades a single frame's hit pass: not with --benchmark, --sequence, --rays, "
                             "--adaptive or --ss above 1\n");
        return 2;
    }
    if (relight && (deferred || bench || !seq.empty() || !rays_file.empty() || ad_k || ss > 1)) {   // before any device work
        std::fprintf(stderr, "--relight shades a single frame's hit pass and shadow pass: not with --deferred, --benchmark, "
                             "--sequence, --rays, --adaptive or --ss above 1\n");
        return 2;
    }
    if (in_place && (!relight || moves.empty())) {   // before any device work
        std::fprintf(stderr, "--in-place makes --relight's --move-light an edit of the uploaded scene: only with both\n");
        return 2;
    }
    if (resolve && (!relight || !aov.empty())) {   // before any device work
        std::fprintf(stderr, "--resolve K resolves a relight of K x K stored samples per pixel: only with --relight, and not "
                             "with --aov (the planes are the sample frame's)\n");
        return 2;
    }
    if (!aov.empty() && (bench || !seq.empty())) {
        std::fprintf(stderr, "--aov writes the planes of a single frame: not with --benchmark or --sequence\n");
        return 2;
    }
    if (ad_k && (bench || !seq.empty() || !aov.empty() || !rays_file.empty() || ss > 1)) {
        std::fprintf(stderr, "--adaptive renders a single frame: not with --benchmark, --sequence, --aov, --rays or --ss above 1\n");
        return 2;
    }
    std::vector<rtx_ray> rays;
    if (!rays_file.empty()) {   // checked and read here: a bad use ends the program before any device work
        if (bench || !seq.empty() || !aov.empty() || ss > 1) {
            std::fprintf(stderr, "--rays shades a single frame: not with --benchmark, --sequence, --aov or --ss above 1\n");
            return 2;
        }
        if (W <= 0 || H <= 0) {
            std::fprintf(stderr, "--rays: bad image size\n");
            return 2;
        }
        rays.resize(static_cast<size_t>(W) * static_cast<size_t>(H));
        FILE* f = std::fopen(rays_file.c_str(), "rb");
        const bool ok = f && std::fread(rays.data(), sizeof(rtx_ray), rays.size(), f) == rays.size() && std::fgetc(f) == EOF;
        if (f) std::fclose(f);
        if (!ok) {
            std::fprintf(stderr, "--rays %s: expected %d x %d rays of 8 float32 (%zu bytes)\n", rays_file.c_str(), W, H,
                         rays.size() * sizeof(rtx_ray));
            return 2;
        }
    }
    char err[512] = {0};
    rtx_host_scene* hs = nullptr;
    if (rtx_host_scene_create(scene.c_str(), assets.empty() ? nullptr : assets.c_str(), &hs, err, sizeof err) != RTX_OK) {
        std::fprintf(stderr, "scene %s: %s\n", scene.c_str(), err);
        return 1;
    }
    // --move-light: the scene's own origins are kept for --relight's first two passes; a light the scene does
    // not have is refused here, before any device work
    std::vector<std::pair<uint32_t, std::array<float, 3>>> unmoved;
    {
        rtx_scene s0;
        rtx_camera c0;
        if (!moves.empty() && rtx_host_scene_view(hs, &s0, &c0) != RTX_OK) {
            std::fprintf(stderr, "rtx_host_scene_view failed\n");
            rtx_host_scene_destroy(hs);
            return 1;
        }
        for (const auto& m : moves) {
            if (m.first >= s0.n_lights) {
                std::fprintf(stderr, "--move-light: scene %s has %u lights, no light %u\n", scene.c_str(), s0.n_lights, m.first);
                rtx_host_scene_destroy(hs);
                return 2;
            }
            const float* o = s0.lights[m.first].origin;
            unmoved.push_back({m.first, {o[0], o[1], o[2]}});
        }
    }
    auto place_lights = [](rtx_host_scene* h, const std::vector<std::pair<uint32_t, std::array<float, 3>>>& to) {
        for (const auto& m : to) rtx_host_light_set_origin(h, m.first, m.second.data());
    };
    place_lights(hs, moves);
    if (t >= 0.f) rtx_host_scene_update(hs, t);
    // the pipelined loop's second host scene (run_benchmark): animated scenes, frames in flight,
    // host Update
    // (up to two more: two Updates in flight with three or more frames in flight)
    auto more_scenes = [&]() {
        std::vector<rtx_host_scene*> v;
        if (inflight < 2 || device_update || rtx_host_scene_animated(hs) != 1) return v;
        for (int i = 0; i < std::min(inflight, 3) - 1; ++i) {
            rtx_host_scene* h = nullptr;
            char e2[512] = {0};
            if (rtx_host_scene_create(scene.c_str(), assets.empty() ? nullptr : assets.c_str(), &h, e2, sizeof e2) != RTX_OK)
                break;   // (fewer Updates in flight, or the loop unpipelined)
            place_lights(h, moves);
            v.push_back(h);
        }
        return v;
    };
    // --relight's moved scene `s` onto the device: an upload, or with --in-place an edit of each moved light
    auto move_lights = [&](rtx::Renderer& r, const rtx_scene& s) {
        if (!in_place) return r.Upload(s);
        for (const auto& m : moves) r.EditLights(m.first, {s.lights[m.first]});
        std::printf("moved %zu light(s) in place\n", moves.size());
    };
    int rc = 0;
    try {
        rtx::Renderer r(W, H);
        r.m_CurrentLightingMode = static_cast<rtx::Renderer::LightingMode>(mode);
        r.m_ShadowsEnabled = shadows;
        r.SetSupersample(static_cast<uint32_t>(ss));
        if (!seq.empty()) {
            // --sequence t1,...: the pipelined frame loop over fixed Update times, frame k
            // written to <out stem>_<k>.bmp
            const std::string stem = out.size() > 4 && out.substr(out.size() - 4) == ".bmp" ? out.substr(0, out.size() - 4) : out;
            const std::vector<rtx_host_scene*> more = more_scenes();
            rc = run_benchmark(r, hs, 0, inflight, device_update, &seq, stem, more, static_cast<uint32_t>(ss));
            for (rtx_host_scene* h : more) rtx_host_scene_destroy(h);
            rtx_host_scene_destroy(hs);
            return rc;
        }
        if (bench) {
            const std::vector<rtx_host_scene*> more = more_scenes();
            rc = run_benchmark(r, hs, bench, inflight, device_update, nullptr, "", more, static_cast<uint32_t>(ss));
            for (rtx_host_scene* h : more) rtx_host_scene_destroy(h);
        } else if (!rays.empty()) {   // the image from the caller's rays, through the same BMP writer
            r.Pixels() = r.ShadeRays(hs, rays, true).pixels;
        } else if (ad_k) {   // the adaptive frame, through the same BMP writer
            r.RenderAdaptive(hs, static_cast<uint32_t>(ad_k), static_cast<uint32_t>(ad_t), true);
            std::printf("refined %u of %d pixels\n", r.AdaptiveRefined(), W * H);
        } else if (deferred) {   // one hit pass, shaded from its planes; --aov writes the same pass
            const rtx::Renderer::AovFrame f = r.RenderAov(hs, RTX_AOV_ALL, true);
            r.ShadeAov();
            if (!aov.empty()) {
                if (!write_plane(aov + "_depth.f32", f.depth) || !write_plane(aov + "_normal.f32", f.normal) ||
                    !write_plane(aov + "_material.u32", f.material) || !write_plane(aov + "_primitive.u32", f.primitive)) {
                    std::fprintf(stderr, "cannot write %s_*\n", aov.c_str());
                    rc = 1;
                } else {
                    std::printf("wrote %s_depth.f32 _normal.f32 _material.u32 _primitive.u32\n", aov.c_str());
                }
            }
        } else if (relight && resolve) {   // the sample frame's two passes, every sample relit, each pixel's resolved
            const uint32_t k = static_cast<uint32_t>(resolve);
            place_lights(hs, {unmoved.rbegin(), unmoved.rend()});   // (--move-light: as below, at sample size)
            r.RenderSamplePasses(hs, k, true);
            if (!moves.empty()) {
                place_lights(hs, moves);
                rtx_scene s;
                rtx_camera cam;
                if (rtx_host_scene_view(hs, &s, &cam) != RTX_OK) throw std::runtime_error("rtx_host_scene_view failed");
                move_lights(r, s);
                uint32_t traced = 0;
                if (rtx_refresh_shadows_async(r.Context(), &traced) != RTX_OK)
                    throw std::runtime_error(std::string("rtx_refresh_shadows_async: ") + rtx_last_error(r.Context()));
                std::printf("refreshed the shadow plane: light mask 0x%x re-traced\n", traced);
            }
            r.RelightResolved();
        } else if (relight) {   // one hit pass, its shadow rays stored, shaded from both; --aov writes all five planes
            // (--move-light: both passes with the scene's own lights, in reverse so that a light moved twice gets
            // its first origin back; then the moved scene, and a refresh that traces the moved lights only)
            place_lights(hs, {unmoved.rbegin(), unmoved.rend()});
            const rtx::Renderer::AovFrame f = r.RenderAov(hs, RTX_AOV_ALL, true);
            std::vector<uint32_t> bits = r.RenderShadows();
            if (!moves.empty()) {
                place_lights(hs, moves);
                rtx_scene s;
                rtx_camera cam;
                if (rtx_host_scene_view(hs, &s, &cam) != RTX_OK) throw std::runtime_error("rtx_host_scene_view failed");
                move_lights(r, s);
                uint32_t traced = 0;
                bits = r.RefreshShadows(&traced);
                std::printf("refreshed the shadow plane: light mask 0x%x re-traced\n", traced);
            }
            r.Relight();
            if (!aov.empty()) {
                if (!write_plane(aov + "_depth.f32", f.depth) || !write_plane(aov + "_normal.f32", f.normal) ||
                    !write_plane(aov + "_material.u32", f.material) || !write_plane(aov + "_primitive.u32", f.primitive) ||
                    !write_plane(aov + "_shadow.u32", bits)) {
                    std::fprintf(stderr, "cannot write %s_*\n", aov.c_str());
                    rc = 1;
                } else {
                    std::printf("wrote %s_depth.f32 _normal.f32 _material.u32 _primitive.u32 _shadow.u32\n", aov.c_str());
                }
            }
        } else {
            r.Render(hs, true);
            auto t0 = Clock::now();
            for (int f = 1; f < frames; ++f) r.Render(hs, false);
            auto t1 = Clock::now();
            if (frames > 1) {
                const double s = secs(t0, t1) / (frames - 1);
                std::printf("%s %dx%d: %.3f ms/frame incl. D2H, %.1f Mpix/s\n", scene.c_str(), W, H, s * 1e3,
                            W * (double)H / s / 1e6);
            }
            if (!aov.empty()) {   // the planes of the frame just rendered (the uploaded scene, the same camera)
                const rtx::Renderer::AovFrame f = r.RenderAov(hs, RTX_AOV_ALL, false);
                if (!write_plane(aov + "_depth.f32", f.depth) || !write_plane(aov + "_normal.f32", f.normal) ||
                    !write_plane(aov + "_material.u32", f.material) || !write_plane(aov + "_primitive.u32", f.primitive)) {
                    std::fprintf(stderr, "cannot write %s_*\n", aov.c_str());
                    rc = 1;
                } else {
                    std::printf("wrote %s_depth.f32 _normal.f32 _material.u32 _primitive.u32\n", aov.c_str());
                }
            }
        }
        if (rc == 0 && !r.SaveBufferToImage(out)) { std::fprintf(stderr, "cannot write %s\n", out.c_str()); rc = 1; }
        else if (rc == 0) std::printf("wrote %s\n", out.c_str());
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        rc = 1;
    }
    rtx_host_scene_destroy(hs);
    return rc;
}
