// rtx_diag.hip — timing, counting and state read-outs behind the C-ABI (include/rtx.h, rtx_diag.h):
// rtx_time_*, rtx_count_work*, the *_info getters, the schedule's read-outs and its run on given costs, the
// cull dump, the stamp dump and the scene image.
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

static_assert(RTX_MAX_HEAVY_TILES == kMaxHeavyTiles, "rtx_diag.h's heavy list");

extern "C" int rtx_schedule_heavy(rtx_ctx* c, uint32_t* heavy_flag, uint32_t n, uint32_t* heavy_list,
                                  uint32_t heavy_n[4], uint64_t* threshold, uint32_t params[4]) {
    if (!c) return RTX_E_INVALID;
    if (!c->sched_ready) return fail(c, RTX_E_STATE, "no frame of the current schedule has been measured");
    if (n > c->sched_cap) return fail(c, RTX_E_INVALID, "n exceeds the schedule size");
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = join_split(c); rc != RTX_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const int k = c->sched_stage;
    if (heavy_flag) HIP_TRY(c, hipMemcpy(heavy_flag, c->d_heavy_flag[k], n * 4, hipMemcpyDeviceToHost));
    if (heavy_list) HIP_TRY(c, hipMemcpy(heavy_list, c->d_heavy_list[k], kMaxHeavyTiles * 4, hipMemcpyDeviceToHost));
    if (heavy_n) HIP_TRY(c, hipMemcpy(heavy_n, c->d_heavy_n, 16, hipMemcpyDeviceToHost));
    if (threshold) HIP_TRY(c, hipMemcpy(threshold, c->d_thr, 8, hipMemcpyDeviceToHost));
    if (params) {
        const SchedParams& P = c->sched_params;
        params[0] = P.split_slots; params[1] = P.permille; params[2] = P.split_min; params[3] = P.wave_slots;
    }
    return RTX_OK;
}

namespace {
// rtx_schedule_run's scratch: one device allocation cut into 256-byte aligned sections, freed on return.
struct SchedScratch {
    char* base = nullptr;
    size_t used = 0;
    ~SchedScratch() { (void)hipFree(base); }
    size_t reserve(size_t bytes) {
        const size_t at = used;
        used += (bytes + 255) & ~size_t(255);
        return at;
    }
    template <class T>
    T* at(size_t off) const { return reinterpret_cast<T*>(base + off); }
};
}  // namespace

extern "C" int rtx_schedule_run(rtx_ctx* c, const rtx_schedule_case* in, rtx_schedule_result* out) {
    if (!c || !in || !out) return RTX_E_INVALID;
    const uint32_t n = in->n;
    const uint64_t per_view = static_cast<uint64_t>(in->tiles_x) * in->tiles_y;
    if (n == 0 || n > (1u << 20)) return fail(c, RTX_E_INVALID, "n must be 1..2^20 tiles");
    if (!in->cost || !in->saved || !out->order || !out->cost_after || !out->saved_after || !out->heavy_flag ||
        !out->heavy_list || (in->xcd && !out->order_xcd))
        return fail(c, RTX_E_INVALID, "a required array is NULL");
    if (per_view == 0) return fail(c, RTX_E_INVALID, "tiles_x * tiles_y must not be 0");
    if (in->xcd && n % per_view != 0) return fail(c, RTX_E_INVALID, "n must be whole views for the XCD re-deal");
    HIP_TRY(c, hipSetDevice(c->device));
    // as sched_buffers (rtx_frame.hip) and rtx_create size the context's own
    const size_t nb = static_cast<size_t>(n) * 4, nch = (n + kSchedChunk - 1) / kSchedChunk;
    SchedScratch S;
    const size_t o_cost = S.reserve(nb), o_was = S.reserve(nb), o_saved = S.reserve(nb), o_order = S.reserve(nb),
                 o_xcd = S.reserve(nb), o_flag = S.reserve(nb), o_hist = S.reserve(nch * kCostBuckets * 4),
                 o_csum = S.reserve(nch * 8), o_thr = S.reserve(8), o_list = S.reserve(kMaxHeavyTiles * 4),
                 o_hn = S.reserve(16);
    HIP_TRY(c, hipMalloc(&S.base, S.used));
    hipStream_t s = c->stream;
    HIP_TRY(c, hipMemcpyAsync(S.at<char>(o_cost), in->cost, nb, hipMemcpyHostToDevice, s));
    if (in->was_heavy) HIP_TRY(c, hipMemcpyAsync(S.at<char>(o_was), in->was_heavy, nb, hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(S.at<char>(o_saved), in->saved, nb, hipMemcpyHostToDevice, s));
    // (what a run must write reads 0xffffffff where it did not)
    HIP_TRY(c, hipMemsetAsync(S.at<char>(o_order), 0xff, o_hist - o_order, s));
    HIP_TRY(c, hipMemsetAsync(S.at<char>(o_thr), 0xff, o_hn - o_thr, s));
    HIP_TRY(c, hipMemsetAsync(S.at<char>(o_hn), 0, 16, s));
    const SchedBufs B = {S.at<uint32_t>(o_cost), in->was_heavy ? S.at<uint32_t>(o_was) : nullptr,
                         S.at<uint32_t>(o_saved), S.at<uint32_t>(o_hist), S.at<unsigned long long>(o_csum),
                         S.at<unsigned long long>(o_thr), S.at<uint32_t>(o_order),
                         in->xcd ? S.at<uint32_t>(o_xcd) : nullptr, S.at<uint32_t>(o_flag), S.at<uint32_t>(o_list),
                         S.at<uint32_t>(o_hn)};
    const SchedParams P = {n, in->tiles_x, in->tiles_y, in->parts, in->split_slots, in->permille, in->split_min,
                           in->wave_slots};
    HIP_TRY(c, sched_launch(s, B, P));
    HIP_TRY(c, hipMemcpyAsync(out->order, B.order, nb, hipMemcpyDeviceToHost, s));
    if (in->xcd) HIP_TRY(c, hipMemcpyAsync(out->order_xcd, B.order_xcd, nb, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(out->cost_after, B.cost, nb, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(out->saved_after, B.saved, nb, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(out->heavy_flag, B.heavy_flag, nb, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(out->heavy_list, B.heavy_list, kMaxHeavyTiles * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(out->heavy_n, B.heavy_n, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(&out->threshold, B.thr, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
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
