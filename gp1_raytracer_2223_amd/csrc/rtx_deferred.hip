// rtx_deferred.hip — deferred shading (PHASE 8) behind the C-ABI: rtx_shade_aov* shades the records of
// the context's last hit pass into the colour frame buffer, and its timing entry point.
#include "rtx_ctx.h"
#include "rtx_launch.h"

using namespace rtxh;

namespace {

// Checks, the frame buffer and the launch record of a shade of the last pass.  The pass gives the shape
// and the cameras (rtx_ctx::aov_last*), `p` the mode, the shadows and the format.  Nothing of the colour
// frames' state (schedule, split tuner, motion mode, frames in flight) is written, and the planes and
// their record are only read.
int deferred_prepare(rtx_ctx* c, const rtx_render_params* p, bool want_rgb, FrameArgs& F, dim3& grid,
                     rtx_render_params& shape) {
    if (!c || !p) return RTX_E_INVALID;
    if (p->lighting_mode < 0 || p->lighting_mode >= RTX_MODE_COUNT) return fail(c, RTX_E_INVALID, "bad lighting mode");
    if (p->format.rshift > 24 || p->format.gshift > 24 || p->format.bshift > 24)
        return fail(c, RTX_E_INVALID, "bad pixel format");
    if (!c->has_scene) return fail(c, RTX_E_STATE, "no scene uploaded");
    if (c->ss_log2)
        return fail(c, RTX_E_UNSUPPORTED, "no deferred shading on a supersampled context (factor " +
                                              std::to_string(1u << c->ss_log2) + "): the hit pass has one record per pixel");
    if (!c->aov_last_mask) return fail(c, RTX_E_STATE, "no hit pass rendered yet");
    if (c->aov_last_mask != static_cast<uint32_t>(RTX_AOV_ALL))
        return fail(c, RTX_E_STATE, "deferred shading needs all four planes: the last hit pass wrote mask " +
                                        std::to_string(c->aov_last_mask));
    if (c->dev.n_materials < c->aov_last_materials)
        return fail(c, RTX_E_STATE, "the scene has " + std::to_string(c->dev.n_materials) +
                                        " materials, the hit pass was traced with " +
                                        std::to_string(c->aov_last_materials));
    if (c->dev.n_materials == 0) return fail(c, RTX_E_STATE, "the scene has no material");
    HIP_TRY(c, hipSetDevice(c->device));
    // behind a pending split chain, which writes the frame buffer this call sizes and writes
    if (const int rc = join_split(c); rc != RTX_OK) return rc;
    // the pass's shape with the call's mode, shadows and format: what the frame would be rendered with
    shape = c->aov_last;
    shape.lighting_mode = p->lighting_mode;
    shape.shadows_enabled = p->shadows_enabled;
    shape.format = p->format;
    const int n_views = c->aov_last_views;
    const size_t npx = static_cast<size_t>(shape.width) * shape.height * static_cast<size_t>(n_views);
    if (const int rc = frame_buffers(c, npx, want_rgb); rc != RTX_OK) return rc;
    frame_shape(c, c->aov_last_cams, n_views, &shape, shape, 0u, F, grid);
    F.out_px = c->d_px;
    F.out_rgb = want_rgb ? c->d_rgb.get() : nullptr;
    // The dispatch order of the context's last colour frames, when they had this tile set (same size, views and
    // stripes, whatever the scene and mode): read, never written.  It starts the costly tiles first, which
    // is worth more to the shade than everything it saves (W4_Bunny 1080p: the frame in tile order 0.088 ms,
    // in cost order 0.052).  Without one (no such frame yet, RTX_TILE_ORDER=0): tile order.
    const std::string tk = tiles_key(shape.width, shape.height, n_views, shape.stripe_rows, shape.stripe_first,
                                     shape.stripe_step);
    if (c->sched_enabled && c->sched_ready && c->sched_key.compare(0, tk.size(), tk) == 0)
        F.order = (c->xcd_order ? c->d_order_xcd : c->d_order).get();
    F.aov_mask = RTX_AOV_ALL;   // the planes the kernel reads
    F.aov_depth = c->d_aov_depth;
    F.aov_normal = c->d_aov_normal;
    F.aov_material = c->d_aov_material;
    F.aov_primitive = c->d_aov_primitive;
    // The shadow rays' cull records are the light anchors', which an upload leaves to its first frame
    // or pass.  After a relight upload that is this call: the boxes and the lights' records, no
    // camera's (the shade casts no primary ray), and the camera records' state stays as it was.
    if (!c->facts.deep_stack && !c->facts.hbm_stack && c->dev.cull_stride && cull_lights_due(c)) {
        FrameArgs L = F;
        L.n_views = 0;
        if (const int rc = cull_views(c, L); rc != RTX_OK) return rc;
    }
    return RTX_OK;
}

// Queue the shade on the context stream: every tile by the one launch (no costs, no heavy set), in the
// variant and with the shadow-ray walk the scene's colour frames take.
int deferred_launch(rtx_ctx* c, const FrameArgs& F, dim3 grid) {
    if (grid.x == 0) return RTX_OK;
    const bool deep = c->facts.deep_stack || c->facts.hbm_stack;
    if (c->facts.hbm_stack)
        if (const int rc = ensure_hbm_stacks(c, grid.x); rc != RTX_OK) return rc;
    const int facts = c->facts.spec | ((F.mode == RTX_MODE_COMBINED && F.shadows) ? kSpecCombShadows : 0);
    const int v = (c->no_spec || deep) ? -1 : spec_variant(facts);
    launch_deferred(v, deep, c->facts.hbm_stack, grid, c->stream, c->dev, F);
    HIP_TRY(c, hipGetLastError());
    return RTX_OK;
}

}  // namespace

extern "C" int rtx_shade_aov_async(rtx_ctx* c, const rtx_render_params* p, int want_rgb) {
    FrameArgs F;
    dim3 grid;
    rtx_render_params shape;
    int rc = deferred_prepare(c, p, want_rgb != 0, F, grid, shape);
    if (rc != RTX_OK) return rc;
    rc = deferred_launch(c, F, grid);
    if (rc != RTX_OK) return rc;
    remember(c, &shape, c->aov_last_views, want_rgb != 0);
    return RTX_OK;
}

extern "C" int rtx_shade_aov(rtx_ctx* c, const rtx_render_params* p, uint32_t* out_px, float* out_rgb) {
    if (!out_px) return RTX_E_INVALID;
    const int rc = rtx_shade_aov_async(c, p, out_rgb != nullptr);
    if (rc != RTX_OK) return rc;
    return rtx_download(c, out_px, out_rgb);
}

extern "C" int rtx_time_shade_aov(rtx_ctx* c, const rtx_render_params* p, int want_rgb, int iters, float* mean_ms) {
    if (!mean_ms || iters <= 0) return RTX_E_INVALID;
    FrameArgs F;
    dim3 grid;
    rtx_render_params shape;
    int rc = deferred_prepare(c, p, want_rgb != 0, F, grid, shape);
    if (rc != RTX_OK) return rc;
    HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
    for (int i = 0; i < iters; ++i) {
        rc = deferred_launch(c, F, grid);
        if (rc != RTX_OK) return rc;
    }
    HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
    HIP_TRY(c, hipEventSynchronize(c->ev1));
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *mean_ms = ms / static_cast<float>(iters);
    remember(c, &shape, c->aov_last_views, want_rgb != 0);
    return RTX_OK;
}
