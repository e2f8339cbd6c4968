// rtx_relight.hip — relighting behind the C-ABI: the shadow pass (PHASE 9: rtx_render_shadows_async, its
// plane and its copies; rtx_update_shadows_async and rtx_refresh_shadows_async, the same pass over a subset
// of the lights, merged into the plane), the relight that shades the last hit pass plus that plane without a ray
// (rtx_relight*, rtx_relight_kernel), and their timing entry points.  The checks of the hit pass and the
// preamble of its launch record are rtx_pass.hip's.
#include <cstring>

#include "rtx_ctx.h"
#include "rtx_launch.h"

using namespace rtxh;

namespace {

// ---- the shadow pass (PHASE 9) ------------------------------------------------------------------

// What every shadow pass checks first; an update's own checks follow them.
int shadows_checks(rtx_ctx* c) {
    if (!c) return RTX_E_INVALID;
    if (const int rc = pass_checks(c, "shadow pass"); rc != RTX_OK) return rc;
    if (c->dev.n_lights > static_cast<uint32_t>(kMaxShadowLights))
        return fail(c, RTX_E_UNSUPPORTED, "the shadow plane holds " + std::to_string(kMaxShadowLights) +
                                              " lights, the scene has " + std::to_string(c->dev.n_lights));
    return RTX_OK;
}

// Bit l for every uploaded light l (at most kMaxShadowLights = 32 of them, after shadows_checks).
uint32_t all_lights(const rtx_ctx* c) {
    return c->dev.n_lights >= 32u ? ~0u : (1u << c->dev.n_lights) - 1u;
}

// The plane and the launch record of a shadow pass over the last hit pass, after its checks.  The pass gives
// the shape and the cameras; the kernel runs as the Combined frame with shadows would (that decides the
// specialised variant, and with it the walk).  Nothing of the colour frames' state is written, and the
// hit planes and their record are only read.  `trace` names the lights whose shadow rays are cast and
// `keep` the bits of the stored word that are carried over, new = (old & keep) | traced: the full pass is
// every light and 0.
int shadows_build(rtx_ctx* c, FrameArgs& F, dim3& grid, uint32_t trace, uint32_t keep) {
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = join_split(c); rc != RTX_OK) return rc;   // (on the context stream, like the hit pass)
    rtx_render_params shape = c->aov_last;
    shape.lighting_mode = RTX_MODE_COMBINED;
    shape.shadows_enabled = 1;
    const size_t npx = static_cast<size_t>(shape.width) * shape.height * static_cast<size_t>(c->aov_last_views);
    if (npx > c->d_shadow.cap) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->shadow_serial = 0;   // (its contents are gone)
        if (const int rc = c->d_shadow.grow(c, npx); rc != RTX_OK) return rc;
    }
    if (const int rc = pass_frame(c, shape, F, grid); rc != RTX_OK) return rc;
    F.occ_bits = c->d_shadow;   // the word the kernel writes, in the frame's layout
    F.lm_lights = trace & all_lights(c);   // (PHASE 9 reads these two as its masks: rtx_kernels.h)
    F.heavy_n = keep & all_lights(c);
    return RTX_OK;
}

int shadows_launch(rtx_ctx* c, const FrameArgs& F, dim3 grid) {
    if (grid.x == 0) return RTX_OK;
    const bool deep = c->facts.deep_stack || c->facts.hbm_stack;
    if (c->facts.hbm_stack)
        if (const int rc = ensure_hbm_stacks(c, grid.x); rc != RTX_OK) return rc;
    const int v = (c->no_spec || deep) ? -1 : spec_variant(c->facts.spec | kSpecCombShadows);
    launch_shadows(v, deep, c->facts.hbm_stack, grid, c->stream, c->dev, F);
    HIP_TRY(c, hipGetLastError());
    return RTX_OK;
}

// What every shadow entry point does once its checks have passed: the record, the launch, and the plane's
// validity record (the hit pass it belongs to and the lights it was traced for).  With `mean_ms` the
// timing entry points' form: the record is made once and `iters` launches of it are timed.
int shadows_pass(rtx_ctx* c, uint32_t trace, uint32_t keep, int iters = 1, float* mean_ms = nullptr) {
    FrameArgs F;
    dim3 grid;
    int rc = shadows_build(c, F, grid, trace, keep);
    if (rc != RTX_OK) return rc;
    // (the join and the plane's growth are shadows_build's: outside the timing)
    rc = mean_ms ? timed_loop(c, iters, mean_ms, [&](int) { return shadows_launch(c, F, grid); })
                 : shadows_launch(c, F, grid);
    if (rc != RTX_OK) return rc;
    c->shadow_serial = c->aov_serial;
    c->shadow_lights = c->light_keys;
    return RTX_OK;
}

// The plane is the last hit pass's: a pass since then may have another shape, and its rows are what a
// copy reads.
int shadows_current(rtx_ctx* c) {
    if (!c->shadow_serial) return fail(c, RTX_E_STATE, "no shadow pass rendered yet");
    if (c->shadow_serial != c->aov_serial || !c->aov_last_mask)
        return fail(c, RTX_E_STATE, "the shadow plane belongs to an earlier hit pass: render the shadow pass again");
    return RTX_OK;
}

// ---- the incremental shadow pass ----------------------------------------------------------------

// rtx_update_shadows_async's checks: the pass's own, then a current plane, the recorded light count, a mask
// inside it, and every light outside the mask where the plane recorded it.  Nothing is changed.
int update_checks(rtx_ctx* c, uint32_t lights) {
    if (const int rc = shadows_checks(c); rc != RTX_OK) return rc;
    if (const int rc = shadows_current(c); rc != RTX_OK) return rc;
    if (c->light_keys.size() != c->shadow_lights.size())
        return fail(c, RTX_E_STATE, "the scene has " + std::to_string(c->light_keys.size()) +
                                        " lights, the shadow plane was traced for " +
                                        std::to_string(c->shadow_lights.size()) + ": refresh or render the shadow pass");
    if (lights & ~all_lights(c))
        return fail(c, RTX_E_INVALID, "the light mask names a light at or above the scene's " +
                                          std::to_string(c->dev.n_lights));
    for (size_t l = 0; l < c->light_keys.size(); ++l)
        if (!((lights >> l) & 1u) && c->light_keys[l] != c->shadow_lights[l])
            return fail(c, RTX_E_STATE, "light " + std::to_string(l) + " is outside the mask, and its origin or type is "
                                            "not the one the shadow plane was traced for");
    return RTX_OK;
}

// The lights whose bit of the plane is not valid for the uploaded scene: a changed origin or type, or a
// light the recorded pass did not have.
uint32_t dirty_lights(const rtx_ctx* c) {
    uint32_t dirty = 0;
    for (size_t l = 0; l < c->light_keys.size(); ++l)
        if (l >= c->shadow_lights.size() || c->light_keys[l] != c->shadow_lights[l]) dirty |= 1u << l;
    return dirty;
}

// Whether there is a plane of the last hit pass to merge into (shadows_current, without the message).
bool plane_current(const rtx_ctx* c) {
    return c->shadow_serial && c->shadow_serial == c->aov_serial && c->aov_last_mask;
}

int queue_shadow_copy(rtx_ctx* c, uint32_t* out) {
    if (!c || !out) return RTX_E_INVALID;
    if (const int rc = shadows_current(c); rc != RTX_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    const CopyPlane plane = {reinterpret_cast<char*>(out), reinterpret_cast<const char*>(c->d_shadow.get()), 4};
    return queue_rows(c, c->aov_last, c->aov_last_views, &plane, 1);
}

// ---- the relight --------------------------------------------------------------------------------

// A relight's checks of the last hit pass: deferred shading's, in its order, then the shadow plane's
// validity with shadows on.  Nothing is changed.
int relight_checks(rtx_ctx* c, const rtx_render_params* p) {
    if (!c || !p) return RTX_E_INVALID;
    if (const int rc = shade_param_checks(c, p); rc != RTX_OK) return rc;
    if (const int rc = pass_checks(c, "relight"); rc != RTX_OK) return rc;
    if (const int rc = material_checks(c); rc != RTX_OK) return rc;
    if (p->shadows_enabled != 0) {
        if (const int rc = shadows_current(c); rc != RTX_OK) return rc;
        if (c->light_keys != c->shadow_lights)
            return fail(c, RTX_E_STATE, "the uploaded lights' count, origins or types are not those the shadow pass was "
                                        "traced for: render the shadow pass again");
    }
    return RTX_OK;
}

// rtx_relight_resolve*'s checks, in the contract's order: the factor, the relight's own, then a pass that is a
// whole number of k x k blocks whose output stripes are a legal frame shape.  `ss` = log2 k.
int resolve_checks(rtx_ctx* c, const rtx_render_params* p, uint32_t k, uint32_t& ss) {
    if (!c || !p) return RTX_E_INVALID;
    if (k != 2 && k != 4 && k != 8) return fail(c, RTX_E_INVALID, "the resolve factor must be 2, 4 or 8");
    ss = k == 8 ? 3u : (k == 4 ? 2u : 1u);
    if (const int rc = relight_checks(c, p); rc != RTX_OK) return rc;
    const rtx_render_params& s = c->aov_last;
    if (s.width % k != 0 || s.height % k != 0)
        return fail(c, RTX_E_INVALID, "the hit pass of " + std::to_string(s.width) + "x" + std::to_string(s.height) +
                                          " is no sample frame of factor " + std::to_string(k) +
                                          ": both sides must be multiples of it");
    if (s.stripe_rows != 0 && s.stripe_step > 1 && s.stripe_rows % (16u * k) != 0)
        return fail(c, RTX_E_UNSUPPORTED, "the pass's stripes of " + std::to_string(s.stripe_rows) +
                                              " sample rows are no multiple of 16 output rows at factor " +
                                              std::to_string(k));
    return RTX_OK;
}

// The frame buffer and the launch record of a relight of the last hit pass, after relight_checks.  With
// ss > 0 (rtx_relight_resolve*, after resolve_checks) the pass is the sample frame of the frame `shape`, whose
// sides and stripes are the pass's divided by k = 1 << ss: A describes the sample frame, its rows and stripes
// count output rows (one wave walks an output row's k sample rows), and the frame buffer holds the output.
int relight_build(rtx_ctx* c, const rtx_render_params* p, bool want_rgb, uint32_t ss, RelightArgs& A, dim3& grid,
                  rtx_render_params& shape) {
    HIP_TRY(c, hipSetDevice(c->device));
    // behind a pending split chain, which writes the frame buffer this call sizes and writes
    if (const int rc = join_split(c); rc != RTX_OK) return rc;
    shape = pass_shape(c, p);
    const int n_views = c->aov_last_views;
    const size_t npx = static_cast<size_t>(shape.width >> ss) * (shape.height >> ss) * static_cast<size_t>(n_views);
    if (const int rc = frame_buffers(c, npx, want_rgb); rc != RTX_OK) return rc;
    // the frame's own launch record: its cameras, aspect and reciprocals are the relight's, value for value
    FrameArgs F;
    dim3 tiles;
    frame_shape(c, c->aov_last_cams, n_views, &shape, shape, 0u, F, tiles);
    std::memset(&A, 0, sizeof A);
    for (int v = 0; v < n_views; ++v) A.cam[v] = F.cam[v];
    A.n_views = F.n_views;
    A.aspect = F.aspect; A.inv_width = F.inv_width; A.inv_height = F.inv_height;
    A.width = F.width; A.height = F.height;
    A.mode = F.mode; A.shadows = F.shadows;
    A.rshift = F.rshift; A.gshift = F.gshift; A.bshift = F.bshift; A.amask = F.amask;
    A.segs = (F.width + 63u) / 64u;
    A.rows = F.height;
    if (F.groups_per_stripe) {   // the largest owner's stripes, row for row (a stripe taller than the frame: its rows)
        A.stripe_rows = F.groups_per_stripe * kWaveTile;
        A.stripe_first = F.stripe_first; A.stripe_step = F.stripe_step;
        if (A.stripe_rows < F.height) A.rows = F.tiles_y * kWaveTile;
    }
    const rtx_aov_planes d = device_planes(c);
    A.depth = d.depth; A.normal = d.normal; A.material = d.material; A.primitive = d.primitive;
    A.shadow = p->shadows_enabled != 0 ? c->d_shadow.get() : nullptr;
    A.out_px = c->d_px;
    A.out_rgb = want_rgb ? c->d_rgb.get() : nullptr;
    // (the resolve's divisions are exact: the sides by resolve_checks, a striped pass's stripe and owned rows as
    // multiples of 16 k.  An unstriped pass's stripe_rows means nothing and may be anything: the output's record is 0.)
    A.rows >>= ss; A.stripe_rows >>= ss;
    shape.width >>= ss; shape.height >>= ss;
    if (ss) shape.stripe_rows = F.groups_per_stripe ? shape.stripe_rows >> ss : 0u;
    const uint32_t waves = A.segs * A.rows * A.n_views, per = kRelightThreads / 64u;
    grid = dim3((waves + per - 1) / per, 1, 1);
    return RTX_OK;
}

// ss = 0: the relight; else the resolved relight of factor 1 << ss.
int relight_launch(rtx_ctx* c, const RelightArgs& A, dim3 grid, uint32_t ss) {
    if (grid.x == 0) return RTX_OK;
    if (ss) launch_relight_resolve(ss, grid, c->stream, c->dev, A);
    else launch_relight(grid, c->stream, c->dev, A);
    HIP_TRY(c, hipGetLastError());
    return RTX_OK;
}

// What the relight and its resolve (ss > 0) do once their checks have passed: the record, the launch and the
// record of the frame now in the frame buffer.  With `mean_ms` the timing entry points' form, as shadows_pass.
int relight_pass(rtx_ctx* c, const rtx_render_params* p, bool want_rgb, uint32_t ss, int iters = 1,
                 float* mean_ms = nullptr) {
    RelightArgs A;
    dim3 grid;
    rtx_render_params shape;
    int rc = relight_build(c, p, want_rgb, ss, A, grid, shape);
    if (rc != RTX_OK) return rc;
    // (the join and the frame buffer's growth are relight_build's: outside the timing)
    rc = mean_ms ? timed_loop(c, iters, mean_ms, [&](int) { return relight_launch(c, A, grid, ss); })
                 : relight_launch(c, A, grid, ss);
    if (rc != RTX_OK) return rc;
    remember(c, &shape, c->aov_last_views, want_rgb);
    return RTX_OK;
}

}  // namespace

extern "C" int rtx_render_shadows_async(rtx_ctx* c) {
    if (const int rc = shadows_checks(c); rc != RTX_OK) return rc;
    return shadows_pass(c, all_lights(c), 0u);
}

extern "C" int rtx_update_shadows_async(rtx_ctx* c, uint32_t lights) {
    if (const int rc = update_checks(c, lights); rc != RTX_OK) return rc;
    if (!lights) return RTX_OK;   // (nothing named and, by the checks, nothing changed)
    return shadows_pass(c, lights, ~lights);
}

extern "C" int rtx_refresh_shadows_async(rtx_ctx* c, uint32_t* traced) {
    if (const int rc = shadows_checks(c); rc != RTX_OK) return rc;
    const bool merge = plane_current(c);   // (a current plane holds the pass's pixels: no growth below)
    const uint32_t trace = merge ? dirty_lights(c) : all_lights(c);
    if (merge && !trace && c->shadow_lights.size() <= c->light_keys.size()) {   // nothing to trace or to clear
        if (traced) *traced = 0u;
        return RTX_OK;
    }
    if (const int rc = shadows_pass(c, trace, merge ? ~trace : 0u); rc != RTX_OK) return rc;
    if (traced) *traced = trace;
    return RTX_OK;
}

extern "C" int rtx_time_shadows(rtx_ctx* c, int iters, float* mean_ms) {
    if (!mean_ms || iters <= 0) return RTX_E_INVALID;
    if (const int rc = shadows_checks(c); rc != RTX_OK) return rc;
    return shadows_pass(c, all_lights(c), 0u, iters, mean_ms);
}

extern "C" int rtx_time_shadows_update(rtx_ctx* c, uint32_t lights, int iters, float* mean_ms) {
    if (!mean_ms || iters <= 0) return RTX_E_INVALID;
    if (const int rc = update_checks(c, lights); rc != RTX_OK) return rc;
    *mean_ms = 0.f;
    if (!lights) return RTX_OK;   // an empty mask launches nothing, as the update: exactly 0 ms
    return shadows_pass(c, lights, ~lights, iters, mean_ms);
}

extern "C" int rtx_gather_shadows_async(rtx_ctx* c, uint32_t* out) { return queue_shadow_copy(c, out); }

extern "C" int rtx_download_shadows(rtx_ctx* c, uint32_t* out) {
    const int rc = queue_shadow_copy(c, out);
    if (rc != RTX_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}

extern "C" int rtx_device_shadow_buffer(rtx_ctx* c, uint32_t** d) {
    if (!c || !d) return RTX_E_INVALID;
    *d = c->d_shadow;
    return RTX_OK;
}

extern "C" int rtx_relight_async(rtx_ctx* c, const rtx_render_params* p, int want_rgb) {
    if (const int rc = relight_checks(c, p); rc != RTX_OK) return rc;
    return relight_pass(c, p, want_rgb != 0, 0u);
}

extern "C" int rtx_relight(rtx_ctx* c, const rtx_render_params* p, uint32_t* out_px, float* out_rgb) {
    if (!out_px) return RTX_E_INVALID;
    const int rc = rtx_relight_async(c, p, out_rgb != nullptr);
    if (rc != RTX_OK) return rc;
    return rtx_download(c, out_px, out_rgb);
}

extern "C" int rtx_time_relight(rtx_ctx* c, const rtx_render_params* p, int want_rgb, int iters, float* mean_ms) {
    if (!mean_ms || iters <= 0) return RTX_E_INVALID;
    if (const int rc = relight_checks(c, p); rc != RTX_OK) return rc;
    return relight_pass(c, p, want_rgb != 0, 0u, iters, mean_ms);
}

extern "C" int rtx_relight_resolve_async(rtx_ctx* c, const rtx_render_params* p, uint32_t k, int want_rgb) {
    uint32_t ss = 0;
    if (const int rc = resolve_checks(c, p, k, ss); rc != RTX_OK) return rc;
    return relight_pass(c, p, want_rgb != 0, ss);
}

extern "C" int rtx_relight_resolve(rtx_ctx* c, const rtx_render_params* p, uint32_t k, uint32_t* out_px, float* out_rgb) {
    if (!out_px) return RTX_E_INVALID;
    const int rc = rtx_relight_resolve_async(c, p, k, out_rgb != nullptr);
    if (rc != RTX_OK) return rc;
    return rtx_download(c, out_px, out_rgb);
}

extern "C" int rtx_time_relight_resolve(rtx_ctx* c, const rtx_render_params* p, uint32_t k, int want_rgb, int iters,
                                        float* mean_ms) {
    if (!mean_ms || iters <= 0) return RTX_E_INVALID;
    uint32_t ss = 0;
    if (const int rc = resolve_checks(c, p, k, ss); rc != RTX_OK) return rc;
    return relight_pass(c, p, want_rgb != 0, ss, iters, mean_ms);
}
