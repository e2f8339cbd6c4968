// rtx_context.hip — the context's life behind the C-ABI of include/rtx.h: create (and the
// environment knobs it reads), destroy, the last error, the scene image's size.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>

#include "rtx_ctx.h"

using namespace rtxh;

extern "C" int rtx_abi_version(void) { return RTX_ABI_VERSION; }

namespace {
// Reason for the last failed rtx_create on this thread (rtx_last_error(NULL)).
thread_local std::string g_create_err;

}  // namespace

extern "C" int rtx_create(rtx_ctx** out, int device_id) {
    if (!out) return RTX_E_INVALID;
    *out = nullptr;
    g_create_err.clear();
    rtx_ctx* c = new (std::nothrow) rtx_ctx;
    if (!c) return RTX_E_NOMEM;
    int n = 0;
    const hipError_t ce = hipGetDeviceCount(&n);
    if (ce != hipSuccess || n == 0) {
        g_create_err = std::string("hipGetDeviceCount: ") + (ce != hipSuccess ? hipGetErrorString(ce) : "no device");
        delete c;
        return RTX_E_DEVICE;
    }
    if (device_id < 0 || device_id >= n) {
        g_create_err = "device id out of range";
        delete c;
        return RTX_E_INVALID;
    }
    c->device = device_id;
    // RTX_TILE_ORDER=0 disables cost-ordered tile dispatch (identity order every frame)
    if (const char* e = std::getenv("RTX_TILE_ORDER")) c->sched_enabled = std::strcmp(e, "0") != 0;
    if (const char* e = std::getenv("RTX_MOTION")) c->motion.off = std::strcmp(e, "0") == 0;
    if (const char* e = std::getenv("RTX_XCD_ORDER")) c->xcd_order = std::strcmp(e, "1") == 0;
    if (const char* e = std::getenv("RTX_THROUGHPUT")) c->throughput_off = std::strcmp(e, "0") == 0;
    if (const char* e = std::getenv("RTX_REFINE")) c->refine.off = std::strcmp(e, "0") == 0;
    if (const char* e = std::getenv("RTX_DEFER_JOIN")) c->join.off = std::strcmp(e, "0") == 0;
    if (const char* e = std::getenv("RTX_DEFER_INFLIGHT")) c->defer_inflight = std::strcmp(e, "0") != 0;
    if (const char* e = std::getenv("RTX_REFINE_ROUNDS")) c->refine.rounds = static_cast<uint32_t>(std::atoi(e));
    if (const char* e = std::getenv("RTX_REFINE_SPLITS")) c->refine.splits = static_cast<uint32_t>(std::atoi(e));
    if (const char* e = std::getenv("RTX_REFINE_TOP")) c->refine.top = static_cast<uint32_t>(std::atoi(e));
    if (const char* e = std::getenv("RTX_INFLIGHT_CRIT")) {
        const double f = std::atof(e);
        if (f >= 0 && f < 1e6) c->inflight_crit = static_cast<uint32_t>(f * 1000.0);
    }
    if (const char* e = std::getenv("RTX_SCHED_PERIOD"))
        c->sched_period = std::max<uint32_t>(1u, static_cast<uint32_t>(std::strtoul(e, nullptr, 10)));
    // RTX_SPLIT=0 renders heavy tiles in one piece; RTX_SPLIT=force splits every tile
    if (const char* e = std::getenv("RTX_NO_SPEC")) c->no_spec = std::strcmp(e, "0") != 0;
    if (const char* e = std::getenv("RTX_ROOM_SKIP")) c->room_skip_off = std::strcmp(e, "0") == 0;
    if (const char* e = std::getenv("RTX_NO_CULL")) c->no_cull = std::strcmp(e, "0") != 0;
    if (const char* e = std::getenv("RTX_CULL_RATIO")) {
        const double v = std::atof(e);
        if (v >= 0.0 && v < 1e30) c->cull_ratio = static_cast<float>(v);
    }
    if (const char* e = std::getenv("RTX_CULL_LEAVES")) c->cull_leaves = std::strcmp(e, "0") != 0;
    if (const char* e = std::getenv("RTX_CULL_ANIMATED")) c->cull_animated = std::strcmp(e, "0") != 0;
    if (const char* e = std::getenv("RTX_CULL_FAIL")) c->cull_fail_at = static_cast<uint32_t>(std::strtoul(e, nullptr, 10));
    if (const char* e = std::getenv("RTX_CULL_TOP_LDS"))
        c->cull_top_lds = std::min<uint32_t>(kCullTopLds, static_cast<uint32_t>(std::strtoul(e, nullptr, 10)));
    if (const char* e = std::getenv("RTX_CULL_MIN_SA")) {
        const double v = std::atof(e);
        if (v >= 0.0 && v < 1e30) c->cull_min_sa = v;
    }
    if (const char* e = std::getenv("RTX_LIGHT_MAJOR"))
        c->lm_mode = std::strcmp(e, "1") == 0 ? 2u : (std::strcmp(e, "auto") == 0 ? 1u : 0u);
    if (const char* e = std::getenv("RTX_LIGHT_MAJOR_TILES")) c->lm_tiles = static_cast<uint32_t>(std::strtoul(e, nullptr, 10));
    if (const char* e = std::getenv("RTX_SPLIT")) c->split_mode = std::strcmp(e, "0") == 0 ? 0u : (std::strcmp(e, "force") == 0 ? 2u : 1u);
    if (const char* e = std::getenv("RTX_SPLIT_PARTS")) {
        const int v = std::atoi(e);
        if (v >= 1 && v <= kMaxParts) c->split_parts = static_cast<uint32_t>(v);
    }
    if (const char* e = std::getenv("RTX_SPLIT_FACTOR")) {
        const double f = std::atof(e);
        if (f > 0 && f < 1e6) { c->tuner.permille = static_cast<uint32_t>(f * 1000.0); c->tuner.on = false; }
    }
    if (const char* e = std::getenv("RTX_SPLIT_TUNE")) c->tuner.on = c->tuner.on && std::strcmp(e, "0") != 0;
    if (const char* e = std::getenv("RTX_SPLIT_MIN_US")) {
        const double us = std::atof(e);
        if (us >= 0 && us < 1e6) c->split_min = static_cast<uint32_t>(us * kSplitMinCost / kSplitMinUs);
    }
    const size_t heavy_px = static_cast<size_t>(kMaxHeavyTiles) * 64;   // pixels of the heavy wave tiles
    int cus = 0, lo_prio = 0, hi_prio = 0;
#define RTX_CREATE_TRY(call)                                                             \
    do {                                                                                 \
        const hipError_t e_ = (call);                                                    \
        if (e_ != hipSuccess) {                                                          \
            g_create_err = std::string(#call) + ": " + hipGetErrorString(e_);            \
            rtx_destroy(c);                                                              \
            return RTX_E_DEVICE;                                                         \
        }                                                                                \
    } while (0)
    RTX_CREATE_TRY(hipSetDevice(device_id));
    RTX_CREATE_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    RTX_CREATE_TRY(hipEventCreate(&c->ev0));
    RTX_CREATE_TRY(hipEventCreate(&c->ev1));
    for (hipEvent_t* e : {&c->ev_heavy, &c->sb[0].done, &c->sb[1].done, &c->ev_fork, &c->ev_join, &c->ev_frame})
        RTX_CREATE_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
    for (auto& e : c->ev_tune) RTX_CREATE_TRY(hipEventCreate(&e));
    for (auto& e : c->ev_win) RTX_CREATE_TRY(hipEventCreate(&e));
    RTX_CREATE_TRY(hipEventCreateWithFlags(&c->ev_refine, hipEventDisableTiming));
    RTX_CREATE_TRY(hipDeviceGetStreamPriorityRange(&lo_prio, &hi_prio));
    if (const char* e = std::getenv("RTX_SPLIT_PRIO"); e && std::strcmp(e, "0") == 0) hi_prio = lo_prio;
    RTX_CREATE_TRY(hipStreamCreateWithPriority(&c->split_stream, hipStreamNonBlocking, hi_prio));
    RTX_CREATE_TRY(c->d_counters.alloc(kNumCounters));
    // {heavy tiles, max tile cost (rtx_sched_count), max tile cost, cost per wave slot (rtx_sched_scan)}
    RTX_CREATE_TRY(c->d_heavy_n.alloc(4));
    RTX_CREATE_TRY(hipMemset(c->d_heavy_n, 0, 16));
    RTX_CREATE_TRY(c->d_thr.alloc(1));
    RTX_CREATE_TRY(hipHostMalloc(&c->h_heavy_n, 16));
    for (auto& l : c->d_heavy_list) RTX_CREATE_TRY(l.alloc(kMaxHeavyTiles));
    RTX_CREATE_TRY(c->d_hit_key.alloc(heavy_px));
    RTX_CREATE_TRY(c->d_occ.alloc(heavy_px));
    RTX_CREATE_TRY(hipMemset(c->d_hit_key, 0xff, 8 * heavy_px));
    RTX_CREATE_TRY(hipMemset(c->d_occ, 0, 4 * heavy_px));
    // (null-stream memsets are asynchronous to the host and the context's non-blocking streams do
    // not wait for them: finish them before any launch can read these buffers)
    RTX_CREATE_TRY(hipStreamSynchronize(nullptr));
    RTX_CREATE_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id));
#undef RTX_CREATE_TRY
    // waves resident at once: 7 per SIMD, 4 SIMDs per CU at the render kernel's occupancy
    c->split_slots = static_cast<uint32_t>(cus > 0 ? cus : 1) * 28u;
    if (!std::getenv("RTX_LIGHT_MAJOR_TILES")) c->lm_tiles = c->split_slots * kLmSlotsPercent / 100u;
    c->lm_waves = static_cast<uint32_t>(cus > 0 ? cus : 1) * 32u;
    // the adaptive refinement's persistent waves: every wave slot at its kernel's occupancy, the shade
    // kernel's (RTX_ADAPTIVE_WAVES caps it: tests force the stride loop with a few waves)
    c->adapt_waves = c->split_slots;
    if (const char* e = std::getenv("RTX_ADAPTIVE_WAVES")) {
        const unsigned long v = std::strtoul(e, nullptr, 10);
        if (v >= 1 && v < c->adapt_waves) c->adapt_waves = static_cast<uint32_t>(v);
    }
    *out = c;
    return RTX_OK;
}

extern "C" void rtx_destroy(rtx_ctx* c) {
    if (!c) return;
    frames_forget(c);
    (void)hipSetDevice(c->device);
    if (c->split_stream) (void)hipStreamSynchronize(c->split_stream);   // (a deferred chain, rtx_ctx::join)
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (auto& B : c->sb) {
        B.free();
        B.cull.free();
        if (B.done) (void)hipEventDestroy(B.done);
    }
    for (DevMem* b : c->bufs) b->free();
    if (c->h_heavy_n) (void)hipHostFree(c->h_heavy_n);
    for (hipEvent_t e : {c->ev_heavy, c->ev_fork, c->ev_join, c->ev_frame, c->ev_tune[0], c->ev_tune[1], c->ev_tune[2],
                         c->ev_win[0], c->ev_win[1], c->ev_refine})
        if (e) (void)hipEventDestroy(e);
    if (c->split_stream) {
        (void)hipStreamSynchronize(c->split_stream);
        (void)hipStreamDestroy(c->split_stream);
    }
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// NULL: why the last rtx_create on this thread failed (empty if it did not).
extern "C" const char* rtx_last_error(const rtx_ctx* c) { return c ? c->err.c_str() : g_create_err.c_str(); }

extern "C" int rtx_scene_bytes(const rtx_ctx* c, uint64_t* bytes) {
    if (!c || !bytes) return RTX_E_INVALID;
    *bytes = c->scene_bytes;
    return RTX_OK;
}
