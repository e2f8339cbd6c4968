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
    if (const int rc = shade_param_checks(c, p); rc != RTX_OK) return rc;
    if (const int rc = pass_checks(c, "deferred shading"); rc != RTX_OK) return rc;
    if (const int rc = material_checks(c); rc != RTX_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    // behind a pending split chain, which writes the frame buffer this call sizes and writes
    if (const int rc = join_split(c); rc != RTX_OK) return rc;
    shape = pass_shape(c, p);
    const size_t npx = static_cast<size_t>(shape.width) * shape.height * static_cast<size_t>(c->aov_last_views);
    if (const int rc = frame_buffers(c, npx, want_rgb); rc != RTX_OK) return rc;
    if (const int rc = pass_frame(c, shape, F, grid); rc != RTX_OK) return rc;
    F.out_px = c->d_px;
    F.out_rgb = want_rgb ? c->d_rgb.get() : nullptr;
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

// The shade and the record of the frame now in the frame buffer.  With `mean_ms` the timing entry point's
// form: the record is made once and `iters` shades of it are timed.
int deferred_pass(rtx_ctx* c, const rtx_render_params* p, bool want_rgb, int iters = 1, float* mean_ms = nullptr) {
    FrameArgs F;
    dim3 grid;
    rtx_render_params shape;
    int rc = deferred_prepare(c, p, want_rgb, F, grid, shape);
    if (rc != RTX_OK) return rc;
    // (the checks, the join and the frame buffer's growth are deferred_prepare's: outside the timing)
    rc = mean_ms ? timed_loop(c, iters, mean_ms, [&](int) { return deferred_launch(c, F, grid); })
                 : deferred_launch(c, F, grid);
    if (rc != RTX_OK) return rc;
    remember(c, &shape, c->aov_last_views, want_rgb);
    return RTX_OK;
}

}  // namespace

extern "C" int rtx_shade_aov_async(rtx_ctx* c, const rtx_render_params* p, int want_rgb) {
    return deferred_pass(c, p, want_rgb != 0);
}

extern "C" int rtx_shade_aov(rtx_ctx* c, const rtx_render_params* p, uint32_t* out_px, float* out_rgb) {
    if (!out_px) return RTX_E_INVALID;
    const int rc = rtx_shade_aov_async(c, p, out_rgb != nullptr);
    if (rc != RTX_OK) return rc;
    return rtx_download(c, out_px, out_rgb);
}

extern "C" int rtx_time_shade_aov(rtx_ctx* c, const rtx_render_params* p, int want_rgb, int iters, float* mean_ms) {
    if (!mean_ms || iters <= 0) return RTX_E_INVALID;
    return deferred_pass(c, p, want_rgb != 0, iters, mean_ms);
}
