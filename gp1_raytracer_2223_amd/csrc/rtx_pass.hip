// rtx_pass.hip — what every consumer of the stored hit pass starts from (deferred shading, the shadow pass,
// the relight and its resolve; rtx_ctx.h declares it): the checks of the pass and of a shade's parameters,
// each stated once and called by the entry points in their contract's order, the pass's shape, and the
// preamble of a launch record over the pass.  Host code only.
#include "rtx_ctx.h"

namespace rtxh {

int shade_param_checks(rtx_ctx* c, const rtx_render_params* p) {
    if (p->lighting_mode < 0 || p->lighting_mode >= RTX_MODE_COUNT) return fail(c, RTX_E_INVALID, "bad lighting mode");
    if (p->format.rshift > 24 || p->format.gshift > 24 || p->format.bshift > 24)
        return fail(c, RTX_E_INVALID, "bad pixel format");
    return RTX_OK;
}

int pass_checks(rtx_ctx* c, const char* what) {
    if (!c->has_scene) return fail(c, RTX_E_STATE, "no scene uploaded");
    if (c->ss_log2)
        return fail(c, RTX_E_UNSUPPORTED, std::string("no ") + what + " on a supersampled context (factor " +
                                              std::to_string(1u << c->ss_log2) + "): the hit pass has one record per pixel");
    if (!c->aov_last_mask) return fail(c, RTX_E_STATE, "no hit pass rendered yet");
    if (c->aov_last_mask != static_cast<uint32_t>(RTX_AOV_ALL))
        return fail(c, RTX_E_STATE, std::string(what) + " needs all four planes: the last hit pass wrote mask " +
                                        std::to_string(c->aov_last_mask));
    return RTX_OK;
}

int material_checks(rtx_ctx* c) {
    if (c->dev.n_materials < c->aov_last_materials)
        return fail(c, RTX_E_STATE, "the scene has " + std::to_string(c->dev.n_materials) +
                                        " materials, the hit pass was traced with " +
                                        std::to_string(c->aov_last_materials));
    if (c->dev.n_materials == 0) return fail(c, RTX_E_STATE, "the scene has no material");
    return RTX_OK;
}

rtx_render_params pass_shape(const rtx_ctx* c, const rtx_render_params* p) {
    rtx_render_params shape = c->aov_last;
    shape.lighting_mode = p->lighting_mode;
    shape.shadows_enabled = p->shadows_enabled;
    shape.format = p->format;
    return shape;
}

rtx_aov_planes device_planes(const rtx_ctx* c) {
    return {c->d_aov_depth, c->d_aov_normal, c->d_aov_material, c->d_aov_primitive};
}

void bind_planes(const rtx_ctx* c, FrameArgs& F, uint32_t mask) {
    const rtx_aov_planes d = device_planes(c);
    F.aov_mask = mask;
    F.aov_depth = d.depth; F.aov_normal = d.normal; F.aov_material = d.material; F.aov_primitive = d.primitive;
}

uint32_t planes_mask(const rtx_aov_planes& o) {
    return (o.depth ? RTX_AOV_DEPTH : 0u) | (o.normal ? RTX_AOV_NORMAL : 0u) | (o.material ? RTX_AOV_MATERIAL : 0u) |
           (o.primitive ? RTX_AOV_PRIMITIVE : 0u);
}

namespace {

// The dispatch order of the context's last colour frames, when they had this tile set (same size, views and
// stripes, whatever the scene and mode): read, never written.  It starts the costly tiles first, which
// is worth more to the shade than everything it saves (W4_Bunny 1080p: the frame in tile order 0.088 ms,
// in cost order 0.052).  Without one (no such frame yet, RTX_TILE_ORDER=0): tile order.
const uint32_t* frames_order(rtx_ctx* c, const rtx_render_params& shape, int n_views) {
    const std::string tk = tiles_key(shape.width, shape.height, n_views, shape.stripe_rows, shape.stripe_first,
                                     shape.stripe_step);
    if (c->sched_enabled && c->sched_ready && c->sched_key.compare(0, tk.size(), tk) == 0)
        return (c->xcd_order ? c->d_order_xcd : c->d_order).get();
    return nullptr;
}

}  // namespace

int pass_frame(rtx_ctx* c, const rtx_render_params& shape, FrameArgs& F, dim3& grid) {
    const int n_views = c->aov_last_views;
    frame_shape(c, c->aov_last_cams, n_views, &shape, shape, 0u, F, grid);
    F.order = frames_order(c, shape, n_views);
    bind_planes(c, F, RTX_AOV_ALL);   // the planes the kernel reads
    // The shadow rays' cull records are the light anchors', which an upload leaves to its first frame
    // or pass.  After a relight upload that is this call: the boxes and the lights' records, no
    // camera's (the pass casts no primary ray), and the camera records' state stays as it was.
    if (!c->facts.deep_stack && !c->facts.hbm_stack && c->dev.cull_stride && cull_lights_due(c)) {
        FrameArgs L = F;
        L.n_views = 0;
        if (const int rc = cull_views(c, L); rc != RTX_OK) return rc;
    }
    return RTX_OK;
}

}  // namespace rtxh
