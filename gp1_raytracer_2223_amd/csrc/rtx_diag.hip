// rtx_diag.hip — timing, counting and state read-outs behind the C-ABI (include/rtx.h, rtx_diag.h):
// rtx_time_*, rtx_count_work*, the *_info getters, the cull dump, the stamp dump and the scene image.
#include <algorithm>
#include <cstring>

#include "rtx_ctx.h"
#include "rtx_variants.h"

using namespace rtxh;

extern "C" int rtx_time_views(rtx_ctx* c, const rtx_camera* cams, int n_views, const rtx_render_params* p, int iters,
                              float* mean_ms) {
    if (!mean_ms || iters <= 0) return RTX_E_INVALID;
    FrameArgs F;
    dim3 grid;
    // every launch is prepared like a real frame: the first frame of a launch shape measures
    // tile costs, the next ones run in the cost order (and split the heavy tiles) it yields,
    // and every kSchedPeriod-th frame measures again
    int rc = prepare(c, cams, n_views, p, false, F, grid);
    if (rc != RTX_OK) return rc;
    // the first frame's prepare stays outside the timing, the later ones' and the last frame's chain inside it
    rc = timed_loop(c, iters, mean_ms, [&](int i) {
        if (i > 0) {
            remember(c, p, n_views, false);
            if (const int rc2 = prepare(c, cams, n_views, p, false, F, grid); rc2 != RTX_OK) return rc2;
        }
        if (const int rc2 = launch(c, F, grid, false); rc2 != RTX_OK) return rc2;
        return i + 1 < iters ? RTX_OK : join_split(c);
    });
    if (rc != RTX_OK) return rc;
    remember(c, p, n_views, false);
    return RTX_OK;
}

extern "C" int rtx_time_frames(rtx_ctx* c, const rtx_camera* cam, const rtx_render_params* p, int iters,
                               float* mean_ms) {
    return rtx_time_views(c, cam, 1, p, iters, mean_ms);
}

// Instrumented variant: the same traversal with per-lane work counters.
namespace {
int count_work(rtx_ctx* c, const rtx_camera* cam, const rtx_render_params* p, uint64_t* counts, int n_counts,
               int mode);
}

extern "C" int rtx_count_work_ex(rtx_ctx* c, const rtx_camera* cam, const rtx_render_params* p, uint64_t* counts,
                                 int n_counts) {
    return count_work(c, cam, p, counts, n_counts, 1);
}

extern "C" int rtx_count_work(rtx_ctx* c, const rtx_camera* cam, const rtx_render_params* p, uint64_t* counts) {
    return count_work(c, cam, p, counts, kModelCounters, 1);
}

extern "C" int rtx_count_work_culled(rtx_ctx* c, const rtx_camera* cam, const rtx_render_params* p, uint64_t* counts,
                                     int n_counts) {
    return count_work(c, cam, p, counts, n_counts, 2);
}

namespace {
// The counters of one render (mode 1: the reference's traversal; 2: the culled walk's executed
// tests), up to kNumCounters values: the kModelCounters of the FLOP model, then the per-wave
// diagnostics and the cull tests.
int count_work(rtx_ctx* c, const rtx_camera* cam, const rtx_render_params* p, uint64_t* counts, int n_counts,
               int mode) {
    if (!counts || n_counts <= 0) return RTX_E_INVALID;
    if (n_counts > kNumCounters) n_counts = kNumCounters;
    FrameArgs F;
    dim3 grid;
    int rc = prepare(c, cam, 1, p, false, F, grid);
    if (rc != RTX_OK) return rc;
    HIP_TRY(c, hipMemsetAsync(c->d_counters, 0, sizeof(unsigned long long) * kNumCounters, c->stream));
    rc = launch(c, F, grid, mode);
    if (rc != RTX_OK) return rc;
    unsigned long long tmp[kNumCounters];
    HIP_TRY(c, hipMemcpyAsync(tmp, c->d_counters, sizeof(unsigned long long) * kNumCounters, hipMemcpyDeviceToHost,
                              c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < n_counts; ++k) counts[k] = tmp[k];
    remember(c, p, 1, false);
    return RTX_OK;
}
}  // namespace

extern "C" int rtx_schedule_state(rtx_ctx* c, uint32_t* order, uint32_t* cost, uint32_t n, uint32_t* n_tiles) {
    if (!c) return RTX_E_INVALID;
    if (n_tiles) *n_tiles = c->sched_ready ? c->sched_cap : 0u;
    if (!c->sched_ready || !order || !cost) return RTX_OK;
    if (n > c->sched_cap) return fail(c, RTX_E_INVALID, "n exceeds the schedule size");
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = join_split(c); rc != RTX_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(order, c->d_order, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(cost, c->d_saved_cost, n * 4, hipMemcpyDeviceToHost));
    return RTX_OK;
}

extern "C" int rtx_schedule_xcd_order(rtx_ctx* c, uint32_t* order, uint32_t n) {
    if (!c || !order) return RTX_E_INVALID;
    if (!c->xcd_order || !c->sched_ready || !c->d_order_xcd)
        return fail(c, RTX_E_STATE, "the context has no XCD order (RTX_XCD_ORDER=1 and a measured frame)");
    if (n > c->sched_cap) return fail(c, RTX_E_INVALID, "n exceeds the schedule size");
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = join_split(c); rc != RTX_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(order, c->d_order_xcd, n * 4, hipMemcpyDeviceToHost));
    return RTX_OK;
}

extern "C" int rtx_cull_info(rtx_ctx* c, uint32_t* enabled, uint64_t* camera_updates) {
    if (!c) return RTX_E_INVALID;
    if (enabled) *enabled = c->dev.cull_stride ? 1u : 0u;
    if (camera_updates) *camera_updates = c->cull_updates;
    return RTX_OK;
}

extern "C" int rtx_spec_info(rtx_ctx* c, uint32_t* facts, int32_t* last_variant) {
    if (!c) return RTX_E_INVALID;
    if (facts) *facts = static_cast<uint32_t>(c->last_facts);
    if (last_variant) *last_variant = c->last_variant;
    return RTX_OK;
}

extern "C" int rtx_room_info(rtx_ctx* c, uint32_t* fact, float* room_M) {
    if (!c) return RTX_E_INVALID;
    if (fact) *fact = c->facts.room_fact ? 1u : 0u;
    if (room_M) *room_M = c->facts.room_M;
    return RTX_OK;
}

extern "C" int rtx_cull_dump(rtx_ctx* c, uint32_t anchor, uint32_t* n_slots, uint32_t* n_tris, float* anchor_p,
                             float* records, uint32_t* ranges, float* nodes, float* tris) {
    if (!c || anchor >= static_cast<uint32_t>(kMaxViews + kMaxCullLights)) return RTX_E_INVALID;
    if (!c->dev.cull_stride) return fail(c, RTX_E_INVALID, "the uploaded scene has no cull records");
    if (n_slots) *n_slots = c->cull_nslots;
    if (n_tris) *n_tris = c->cull_ntris;
    if (anchor_p) std::memcpy(anchor_p, c->cull_anchor[anchor], sizeof c->cull_anchor[anchor]);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const size_t ns = c->cull_nslots;
    if (records)
        HIP_TRY(c, hipMemcpy(records, reinterpret_cast<const char*>(c->dev.cull) + static_cast<size_t>(anchor) * c->dev.cull_stride,
                             ns * 32, hipMemcpyDeviceToHost));
    if (ranges) HIP_TRY(c, hipMemcpy(ranges, c->cull_rng, ns * 8, hipMemcpyDeviceToHost));
    if (nodes) HIP_TRY(c, hipMemcpy(nodes, c->dev.nodes, ns * 32, hipMemcpyDeviceToHost));
    if (tris) HIP_TRY(c, hipMemcpy(tris, c->dev.tris, static_cast<size_t>(c->cull_ntris) * 64, hipMemcpyDeviceToHost));
    return RTX_OK;
}

extern "C" int rtx_split_tune_info(rtx_ctx* c, float* factor, float* main_ms, float* chain_ms, uint32_t* done) {
    if (!c) return RTX_E_INVALID;
    if (factor) *factor = static_cast<float>(c->tuner.permille) / 1000.f;
    if (main_ms) *main_ms = c->tuner.main_ms;
    if (chain_ms) *chain_ms = c->tuner.chain_ms;
    if (done) *done = (!c->tuner.on ? 2u : (c->tuner.done ? 1u : 0u));
    return RTX_OK;
}

extern "C" int rtx_inflight_info(rtx_ctx* c, uint32_t* concurrent, uint32_t* onepiece, float* crit,
                                 float* crit_threshold, float* split_interval_ms) {
    if (!c) return RTX_E_INVALID;
    if (split_interval_ms) *split_interval_ms = c->window.interval_ms;
    if (concurrent) *concurrent = c->concurrent ? 1u : 0u;
    if (onepiece) *onepiece = c->frame_onepiece ? 1u : 0u;
    if (crit) *crit = inflight_ratio(c);
    if (crit_threshold) *crit_threshold = static_cast<float>(c->inflight_crit) / 1000.f;
    return RTX_OK;
}

extern "C" int rtx_light_major_info(rtx_ctx* c, uint32_t* last_frame, uint32_t* max_tiles) {
    if (!c) return RTX_E_INVALID;
    if (last_frame) *last_frame = c->frame_lm ? 1u : 0u;
    if (max_tiles) *max_tiles = c->lm_mode == 0 ? 0u : (c->lm_mode == 2 ? 0xffffffffu : c->lm_tiles);
    return RTX_OK;
}

extern "C" int rtx_split_info(rtx_ctx* c, uint32_t* heavy_tiles, uint32_t* parts) {
    if (!c) return RTX_E_INVALID;
    if (c->heavy.pending) {   // a measured frame is in flight: report the set it selects
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipEventSynchronize(c->ev_heavy));
    }
    const uint32_t n = c->heavy.pending ? std::min<uint32_t>(c->h_heavy_n[0], kMaxHeavyTiles) : c->heavy.n;
    const bool on = c->split_mode != 0 && c->facts.split_ok && c->sched_enabled;
    if (heavy_tiles) *heavy_tiles = on ? n : 0u;
    if (parts) *parts = c->facts.split_ok ? c->dev.n_parts : 0u;
    return RTX_OK;
}

#if RTX_STAMPS
// Diagnostic build only: render once with per-wave {start, end, hw ids} stamps.
extern "C" int rtx_debug_stamps(rtx_ctx* c, const rtx_camera* cam, const rtx_render_params* p, uint64_t* out,
                                uint64_t capacity, uint64_t* n_waves) {
    FrameArgs F;
    dim3 grid;
    int rc = prepare(c, cam, 1, p, false, F, grid);
    if (rc != RTX_OK) return rc;
    const uint64_t nw = F.n_tiles;   // one record per wave tile
    *n_waves = nw;
    if (kStampWords * nw > capacity) return RTX_E_INVALID;
    if (kStampWords * nw + 6 * kMaxParts > capacity) return RTX_E_INVALID;
    unsigned long long* d = nullptr;
    // + per (phase 1/2, part, shard) {sum, max, steps}, reduced over the shards below
    const size_t words = kStampWords * nw + 6 * kMaxParts * kStampShards;
    HIP_TRY(c, hipMalloc(&d, words * 8));
    HIP_TRY(c, hipMemsetAsync(d, 0, words * 8, c->stream));
    F.stamps = d;
    F.split_stamps = d + kStampWords * nw;
    rc = launch(c, F, grid, false);
    if (rc != RTX_OK) return rc;
    rc = join_split(c);
    if (rc != RTX_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(out, d, kStampWords * nw * 8, hipMemcpyDeviceToHost, c->stream));
    std::vector<unsigned long long> sh(6 * kMaxParts * kStampShards);
    HIP_TRY(c, hipMemcpyAsync(sh.data(), d + kStampWords * nw, sh.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    (void)hipFree(d);
    for (size_t k = 0; k < 2u * kMaxParts; ++k) {
        unsigned long long sum = 0, mx = 0, steps = 0;
        for (int j = 0; j < kStampShards; ++j) {
            const unsigned long long* x = sh.data() + 3 * (k * kStampShards + j);
            sum += x[0];
            mx = std::max(mx, x[1]);
            steps += x[2];
        }
        out[kStampWords * nw + 3 * k] = sum;
        out[kStampWords * nw + 3 * k + 1] = mx;
        out[kStampWords * nw + 3 * k + 2] = steps;
    }
    return RTX_OK;
}
#endif

// Diagnostics: a copy of the context's current scene image (after its queued work).
extern "C" int rtx_scene_image(rtx_ctx* c, void* out, size_t capacity, size_t* bytes) {
    if (!c || !bytes) return RTX_E_INVALID;
    if (!c->has_scene) return fail(c, RTX_E_STATE, "no scene uploaded");
    *bytes = c->scene_bytes;
    if (!out) return RTX_OK;
    if (capacity < c->scene_bytes) return fail(c, RTX_E_INVALID, "capacity below the image size");
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = join_split(c); rc != RTX_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(out, c->sb[c->sb_cur].d, c->scene_bytes, hipMemcpyDeviceToHost));
    return RTX_OK;
}
