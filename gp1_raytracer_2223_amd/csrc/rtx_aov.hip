// rtx_aov.hip — the hit pass (PHASE 7) behind the C-ABI: rtx_render_aov*, its planes, its copies and
// its timing entry point.
#include "rtx_ctx.h"
#include "rtx_launch.h"

using namespace rtxh;

// ---- the hit pass (PHASE 7): rtx_render_aov* ----------------------------------------------------
namespace {

// One more plane of `n` elements of `elem` bytes (the frames queued on the stream may still write the old one).
template <class T>
int aov_alloc(rtx_ctx* c, DevBuf<T>& d, size_t n, size_t elem) {
    return d ? RTX_OK : d.grow(c, n, elem);
}

// Checks, the planes of `mask` and the launch record of a pass; nothing of the colour frames' state
// (schedule, split tuner, motion mode, frames in flight, the last-frame record) is read or written.
int aov_prepare(rtx_ctx* c, const rtx_camera* cams, int n_views, const rtx_render_params* p, uint32_t mask,
                FrameArgs& F, dim3& grid) {
    if (!c || !cams || !p) return RTX_E_INVALID;
    if (mask == 0 || (mask & ~static_cast<uint32_t>(RTX_AOV_ALL)))
        return fail(c, RTX_E_INVALID, "AOV mask must be a non-empty set of RTX_AOV_* bits (got " + std::to_string(mask) + ")");
    if (n_views < 1 || n_views > kMaxViews) return fail(c, RTX_E_INVALID, "n_views must be 1..8");
    if (!c->has_scene) return fail(c, RTX_E_STATE, "no scene uploaded");
    if (c->ss_log2)
        return fail(c, RTX_E_UNSUPPORTED, "no hit pass on a supersampled context (factor " +
                                              std::to_string(1u << c->ss_log2) + "): averaged ids mean nothing");
    if (p->width == 0 || p->height == 0 || p->width > 65536 || p->height > 65536)
        return fail(c, RTX_E_INVALID, "bad image size");
    const bool striped = p->stripe_rows != 0 && p->stripe_step > 1;
    if (striped && (p->stripe_rows % 16 != 0 || p->stripe_first >= p->stripe_step))
        return fail(c, RTX_E_INVALID, "stripe_rows must be a multiple of 16 and stripe_first < stripe_step");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t npx = static_cast<size_t>(p->width) * p->height * static_cast<size_t>(n_views);
    // the planes of every mask seen so far, each allocated when first asked for
    const uint32_t need = mask | planes_mask(device_planes(c));
    if (npx > c->aov_cap) {   // larger planes: all of them again, at the new size
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->d_aov_depth.free(); c->d_aov_normal.free();
        c->d_aov_material.free(); c->d_aov_primitive.free();
        c->aov_last_mask = 0;   // (their contents are gone)
        ++c->aov_serial;
        c->aov_cap = npx;
    }
    int rc = RTX_OK;
    if (need & RTX_AOV_DEPTH) rc = aov_alloc(c, c->d_aov_depth, c->aov_cap, 4);
    if (rc == RTX_OK && (need & RTX_AOV_NORMAL)) rc = aov_alloc(c, c->d_aov_normal, c->aov_cap, 12);
    if (rc == RTX_OK && (need & RTX_AOV_MATERIAL)) rc = aov_alloc(c, c->d_aov_material, c->aov_cap, 4);
    if (rc == RTX_OK && (need & RTX_AOV_PRIMITIVE)) rc = aov_alloc(c, c->d_aov_primitive, c->aov_cap, 4);
    if (rc != RTX_OK) return rc;
    frame_shape(c, cams, n_views, p, *p, 0u, F, grid);
    bind_planes(c, F, mask);
    return RTX_OK;
}

// Queue the pass on the context stream, like the counting launch: behind the last frame's split chain,
// every tile rendered by the one launch (no order, no costs, no heavy set), with the walk the scene's
// colour frames take (the exact cull, or the deep stacks, which walk without it).
int aov_launch(rtx_ctx* c, const FrameArgs& F, dim3 grid) {
    if (grid.x == 0) return RTX_OK;
    if (const int rc = join_split(c); rc != RTX_OK) return rc;
    if (c->facts.hbm_stack) {
        if (const int rc = ensure_hbm_stacks(c, grid.x); rc != RTX_OK) return rc;
        launch_hit_pass(true, true, false, grid, c->stream, c->dev, F);
    } else if (c->facts.deep_stack) {
        launch_hit_pass(true, false, false, grid, c->stream, c->dev, F);
    } else {
        if (c->dev.cull_stride) {   // the views' camera-anchor cull records, as a frame would
            if (const int rc = cull_views(c, F); rc != RTX_OK) return rc;
        }
        if (c->dev.cull_stride)   // (cull_views drops the records when it cannot build them)
            launch_hit_pass(false, false, true, grid, c->stream, c->dev, F);
        else
            launch_hit_pass(false, false, false, grid, c->stream, c->dev, F);
    }
    HIP_TRY(c, hipGetLastError());
    return RTX_OK;
}

// The record of the pass just queued (rtx_ctx::aov_last*): its shape for the copies, and its cameras and
// the scene's material count for deferred shading (rtx_deferred.hip).
void aov_remember(rtx_ctx* c, const rtx_camera* cams, int n_views, const rtx_render_params* p, uint32_t mask) {
    c->aov_last = *p;
    c->aov_last_views = n_views;
    c->aov_last_mask = mask;
    for (int v = 0; v < n_views; ++v) c->aov_last_cams[v] = cams[v];
    c->aov_last_materials = c->dev.n_materials;
    ++c->aov_serial;   // (a shadow plane of an earlier pass is no longer this one's: rtx_relight.hip)
}

// ... of the last hit pass (rtx_ctx::aov_last*)
int queue_aov_copy(rtx_ctx* c, const rtx_aov_planes* out) {
    if (!c || !out) return RTX_E_INVALID;
    if (!c->aov_last_mask) return fail(c, RTX_E_STATE, "no hit pass rendered yet");
    const uint32_t want = planes_mask(*out);
    if (want & ~c->aov_last_mask)
        return fail(c, RTX_E_STATE, "the last hit pass (mask " + std::to_string(c->aov_last_mask) +
                                        ") did not write every plane asked for (mask " + std::to_string(want) + ")");
    HIP_TRY(c, hipSetDevice(c->device));
    const CopyPlane planes[4] = {
        {reinterpret_cast<char*>(out->depth), reinterpret_cast<const char*>(c->d_aov_depth.get()), 4},
        {reinterpret_cast<char*>(out->normal), reinterpret_cast<const char*>(c->d_aov_normal.get()), 12},
        {reinterpret_cast<char*>(out->material), reinterpret_cast<const char*>(c->d_aov_material.get()), 4},
        {reinterpret_cast<char*>(out->primitive), reinterpret_cast<const char*>(c->d_aov_primitive.get()), 4}};
    return queue_rows(c, c->aov_last, c->aov_last_views, planes, 4);
}

}  // namespace

extern "C" int rtx_render_aov_async(rtx_ctx* c, const rtx_camera* cams, int n_views, const rtx_render_params* p,
                                    uint32_t mask) {
    FrameArgs F;
    dim3 grid;
    int rc = aov_prepare(c, cams, n_views, p, mask, F, grid);
    if (rc != RTX_OK) return rc;
    rc = aov_launch(c, F, grid);
    if (rc != RTX_OK) return rc;
    aov_remember(c, cams, n_views, p, mask);
    return RTX_OK;
}

extern "C" int rtx_gather_aov_async(rtx_ctx* c, const rtx_aov_planes* out) { return queue_aov_copy(c, out); }

extern "C" int rtx_download_aov(rtx_ctx* c, const rtx_aov_planes* out) {
    const int rc = queue_aov_copy(c, out);
    if (rc != RTX_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}

extern "C" int rtx_render_aov(rtx_ctx* c, const rtx_camera* cam, const rtx_render_params* p, uint32_t mask,
                              const rtx_aov_planes* out) {
    if (!out) return RTX_E_INVALID;
    const int rc = rtx_render_aov_async(c, cam, 1, p, mask);
    if (rc != RTX_OK) return rc;
    return rtx_download_aov(c, out);
}

extern "C" int rtx_device_aov_buffers(rtx_ctx* c, rtx_aov_planes* out) {
    if (!c || !out) return RTX_E_INVALID;
    *out = device_planes(c);
    return RTX_OK;
}

extern "C" int rtx_time_aov_frames(rtx_ctx* c, const rtx_camera* cam, const rtx_render_params* p, uint32_t mask,
                                   int iters, float* mean_ms) {
    if (!mean_ms || iters <= 0) return RTX_E_INVALID;
    FrameArgs F;
    dim3 grid;
    int rc = aov_prepare(c, cam, 1, p, mask, F, grid);
    if (rc != RTX_OK) return rc;
    // joined before ev0: aov_launch joins a colour frame's pending chain, which is not the pass's time
    if (const int rc2 = join_split(c); rc2 != RTX_OK) return rc2;
    rc = timed_loop(c, iters, mean_ms, [&](int) { return aov_launch(c, F, grid); });
    if (rc != RTX_OK) return rc;
    aov_remember(c, cam, 1, p, mask);
    return RTX_OK;
}
