// rtx_query.hip — ray queries behind the C-ABI: rtx_trace_rays*, rtx_occluded* (rtx_query_kernel,
// rtx_hip.hip) and rtx_shade_rays* (rtx_shade_kernel): their checks, the host variants' staging buffer
// and the launches.
#include <algorithm>

#include "rtx_ctx.h"
#include "rtx_launch.h"

using namespace rtxh;

namespace {

// the staging buffer's sections for `cap` rays: the rays, the four planes, the occlusion bytes; a shade
// call's pixels and colours take the depth and the normal sections (the same sizes per ray)
constexpr size_t kOffDepth = 32, kOffNormal = 36, kOffMaterial = 48, kOffPrimitive = 52, kOffOcc = 56, kPerRay = 57;
constexpr size_t kOffPixels = kOffDepth, kOffRgb = kOffNormal;

int query_check(rtx_ctx* c, const void* rays, uint32_t n, const void* out) {
    if (!c) return RTX_E_INVALID;
    if (n > 0 && (!rays || !out)) return fail(c, RTX_E_INVALID, "a ray query needs rays and an output");
    return RTX_OK;
}

int mask_check(rtx_ctx* c, uint32_t mask, const rtx_aov_planes* out) {
    if (mask == 0 || (mask & ~static_cast<uint32_t>(RTX_AOV_ALL)))
        return fail(c, RTX_E_INVALID, "a ray query's mask must be a non-empty set of RTX_AOV_* bits (got " +
                                          std::to_string(mask) + ")");
    if (!out) return RTX_OK;   // (n == 0)
    const uint32_t given = planes_mask(*out);
    if (given & ~mask)
        return fail(c, RTX_E_INVALID, "a ray query's planes (mask " + std::to_string(given) +
                                          ") must be planes of its mask (" + std::to_string(mask) + ")");
    return RTX_OK;
}

// The rays of one launch: kQueryChunkRays, and with HBM stacks what keeps them below kQueryStackBytes.
uint32_t launch_rays(const rtx_ctx* c) {
    uint32_t chunk = kQueryChunkRays;
    if (c->facts.hbm_stack) {
        const size_t per_wave = (static_cast<size_t>(c->facts.max_depth) + 1u) * (sizeof(uint4) + sizeof(unsigned long long));
        const size_t waves = std::max<size_t>(kQueryStackBytes / per_wave, static_cast<size_t>(kWavesPerBlock));
        chunk = static_cast<uint32_t>(std::min<size_t>(chunk, waves / kWavesPerBlock * kWavesPerBlock * 64u));
    }
    return chunk;
}

// Queue the launches of one call over the rays of `Q` (QueryArgs or ShadeArgs) on the context stream,
// behind the last frame's split chain like the hit pass; nothing of the frames' state is read or written.
// A large n is cut into launches of at most kQueryChunkRays rays, and with HBM stacks into launches whose
// stacks stay below kQueryStackBytes: launch(deep, hstk, grid, Q) queues one of Q.n rays, and
// advance(Q, n) moves Q's output pointers n rays on (the rays move here).
template <class Args, class Launch, class Advance>
int chunk_launch(rtx_ctx* c, Args Q, Launch launch, Advance advance) {
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = join_split(c); rc != RTX_OK) return rc;
    const uint32_t chunk = launch_rays(c);
    const uint32_t total = Q.n;
    for (uint32_t first = 0; first < total; first += chunk) {
        const uint32_t n = std::min(chunk, total - first);
        const uint32_t waves = (n + 63u) / 64u;
        const dim3 grid((waves + kWavesPerBlock - 1u) / kWavesPerBlock);
        if (c->facts.hbm_stack) {
            if (const int rc = ensure_hbm_stacks(c, grid.x); rc != RTX_OK) return rc;
        }
        Q.n = n;
        launch(c->facts.deep_stack || c->facts.hbm_stack, c->facts.hbm_stack, grid, Q);
        HIP_TRY(c, hipGetLastError());
        Q.rays += static_cast<size_t>(n) * 8u;
        advance(Q, n);
    }
    return RTX_OK;
}

int query_launch(rtx_ctx* c, bool any, const QueryArgs& Q) {
    if (!c->has_scene) return fail(c, RTX_E_STATE, "no scene uploaded");
    return chunk_launch(
        c, Q,
        [&](bool deep, bool hstk, dim3 grid, const QueryArgs& q) {
            launch_query(any, deep, hstk, grid, c->stream, c->dev, q);
        },
        [](QueryArgs& q, uint32_t n) {
            if (q.depth) q.depth += n;
            if (q.normal) q.normal += static_cast<size_t>(n) * 3u;
            if (q.material) q.material += n;
            if (q.primitive) q.primitive += n;
            if (q.occ) q.occ += n;
        });
}

int shade_launch(rtx_ctx* c, const ShadeArgs& Q) {
    return chunk_launch(
        c, Q,
        [&](bool deep, bool hstk, dim3 grid, const ShadeArgs& q) { launch_shade(deep, hstk, grid, c->stream, c->dev, q); },
        [](ShadeArgs& q, uint32_t n) {
            if (q.out_px) q.out_px += n;
            if (q.out_rgb) q.out_rgb += static_cast<size_t>(n) * 3u;
        });
}

// A shade call's checks, in the order of the error table (rtx.h); the lighting mode and the pixel
// format as rtx_render checks them.
int shade_check(rtx_ctx* c, const void* rays, uint32_t n, const rtx_render_params* p, const void* px, const void* rgb) {
    if (!c) return RTX_E_INVALID;
    if (!p) return fail(c, RTX_E_INVALID, "a shade call needs render parameters");
    if (n > 0 && !rays) return fail(c, RTX_E_INVALID, "a shade call needs rays");
    if (n > 0 && !px && !rgb) return fail(c, RTX_E_INVALID, "a shade call needs an output: pixels, rgb or both");
    return shade_param_checks(c, p);
}

QueryArgs trace_args(const rtx_ray* d_rays, uint32_t n, uint32_t mask, const rtx_aov_planes& d) {
    QueryArgs Q{};
    Q.rays = reinterpret_cast<const float*>(d_rays);
    Q.n = n;
    Q.mask = mask;
    Q.depth = d.depth;
    Q.normal = d.normal;
    Q.material = d.material;
    Q.primitive = d.primitive;
    return Q;
}

// The staging buffer for n rays (grown on demand: the queries queued so far are waited for first) ...
int stage_room(rtx_ctx* c, uint32_t n) {
    HIP_TRY(c, hipSetDevice(c->device));
    if (n <= c->d_query.cap) return RTX_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return c->d_query.grow(c, (static_cast<size_t>(n) + 63u) / 64u * 64u, kPerRay);
}
// ... and the rays in it.
int stage(rtx_ctx* c, const rtx_ray* rays, uint32_t n) {
    if (const int rc = stage_room(c, n); rc != RTX_OK) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->d_query, rays, static_cast<size_t>(n) * sizeof(rtx_ray), hipMemcpyHostToDevice,
                              c->stream));
    return RTX_OK;
}

}  // namespace

extern "C" int rtx_trace_rays_device(rtx_ctx* c, const rtx_ray* d_rays, uint32_t n, uint32_t mask,
                                     const rtx_aov_planes* d_out) {
    if (const int rc = query_check(c, d_rays, n, d_out); rc != RTX_OK) return rc;
    if (const int rc = mask_check(c, mask, d_out); rc != RTX_OK) return rc;
    if (n == 0) return RTX_OK;
    if (!c->has_scene) return fail(c, RTX_E_STATE, "no scene uploaded");
    // (a plane of the mask the caller left NULL is not asked for)
    const uint32_t given = planes_mask(*d_out);
    if (given == 0) return RTX_OK;
    return query_launch(c, false, trace_args(d_rays, n, given, *d_out));
}

extern "C" int rtx_occluded_device(rtx_ctx* c, const rtx_ray* d_rays, uint32_t n, uint8_t* d_out) {
    if (const int rc = query_check(c, d_rays, n, d_out); rc != RTX_OK) return rc;
    if (n == 0) return RTX_OK;
    if (!c->has_scene) return fail(c, RTX_E_STATE, "no scene uploaded");
    QueryArgs Q{};
    Q.rays = reinterpret_cast<const float*>(d_rays);
    Q.n = n;
    Q.occ = d_out;
    return query_launch(c, true, Q);
}

extern "C" int rtx_time_ray_queries(rtx_ctx* c, const rtx_ray* d_rays, uint32_t n, int what, uint32_t mask,
                                    const rtx_aov_planes* d_out, uint8_t* d_occ, int iters, float* mean_ms) {
    if (!c || !d_rays || !mean_ms || iters <= 0 || n == 0 || what < 0 || what > 2) return RTX_E_INVALID;
    if (what == 2)   // the staging buffer's ray section as the copy's target
        if (const int rc = stage_room(c, n); rc != RTX_OK) return rc;
    const auto once = [&]() -> int {
        if (what == 0) return rtx_trace_rays_device(c, d_rays, n, mask, d_out);
        if (what == 1) return rtx_occluded_device(c, d_rays, n, d_occ);
        HIP_TRY(c, hipMemcpyAsync(c->d_query, d_rays, static_cast<size_t>(n) * sizeof(rtx_ray), hipMemcpyDeviceToDevice,
                                  c->stream));
        return RTX_OK;
    };
    // one full call first: its checks and a pending chain's join stay outside the timing of the public entry point
    if (const int rc = once(); rc != RTX_OK) return rc;
    return timed_loop(c, iters, mean_ms, [&](int) { return once(); });
}

extern "C" int rtx_trace_rays(rtx_ctx* c, const rtx_ray* rays, uint32_t n, uint32_t mask, const rtx_aov_planes* out) {
    if (const int rc = query_check(c, rays, n, out); rc != RTX_OK) return rc;
    if (const int rc = mask_check(c, mask, out); rc != RTX_OK) return rc;
    if (n == 0) return RTX_OK;
    if (!c->has_scene) return fail(c, RTX_E_STATE, "no scene uploaded");
    if (const int rc = stage(c, rays, n); rc != RTX_OK) return rc;
    const size_t cap = c->d_query.cap;
    rtx_aov_planes d{};
    if (out->depth) d.depth = reinterpret_cast<float*>(c->d_query + kOffDepth * cap);
    if (out->normal) d.normal = reinterpret_cast<float*>(c->d_query + kOffNormal * cap);
    if (out->material) d.material = reinterpret_cast<uint32_t*>(c->d_query + kOffMaterial * cap);
    if (out->primitive) d.primitive = reinterpret_cast<uint32_t*>(c->d_query + kOffPrimitive * cap);
    if (const int rc = rtx_trace_rays_device(c, reinterpret_cast<const rtx_ray*>(c->d_query.get()), n, mask, &d); rc != RTX_OK)
        return rc;
    const size_t N = n;
    if (out->depth) HIP_TRY(c, hipMemcpyAsync(out->depth, d.depth, N * 4u, hipMemcpyDeviceToHost, c->stream));
    if (out->normal) HIP_TRY(c, hipMemcpyAsync(out->normal, d.normal, N * 12u, hipMemcpyDeviceToHost, c->stream));
    if (out->material) HIP_TRY(c, hipMemcpyAsync(out->material, d.material, N * 4u, hipMemcpyDeviceToHost, c->stream));
    if (out->primitive)
        HIP_TRY(c, hipMemcpyAsync(out->primitive, d.primitive, N * 4u, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}

extern "C" int rtx_occluded(rtx_ctx* c, const rtx_ray* rays, uint32_t n, uint8_t* out) {
    if (const int rc = query_check(c, rays, n, out); rc != RTX_OK) return rc;
    if (n == 0) return RTX_OK;
    if (!c->has_scene) return fail(c, RTX_E_STATE, "no scene uploaded");
    if (const int rc = stage(c, rays, n); rc != RTX_OK) return rc;
    uint8_t* d_occ = reinterpret_cast<uint8_t*>(c->d_query + kOffOcc * c->d_query.cap);
    if (const int rc = rtx_occluded_device(c, reinterpret_cast<const rtx_ray*>(c->d_query.get()), n, d_occ); rc != RTX_OK)
        return rc;
    HIP_TRY(c, hipMemcpyAsync(out, d_occ, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}

extern "C" int rtx_shade_rays_device(rtx_ctx* c, const rtx_ray* d_rays, uint32_t n, const rtx_render_params* p,
                                     uint32_t* d_pixels, float* d_rgb) {
    if (const int rc = shade_check(c, d_rays, n, p, d_pixels, d_rgb); rc != RTX_OK) return rc;
    if (n == 0) return RTX_OK;
    if (!c->has_scene) return fail(c, RTX_E_STATE, "no scene uploaded");
    ShadeArgs Q{};
    Q.rays = reinterpret_cast<const float*>(d_rays);
    Q.n = n;
    Q.mode = p->lighting_mode;
    Q.shadows = p->shadows_enabled ? 1 : 0;
    Q.rshift = p->format.rshift; Q.gshift = p->format.gshift; Q.bshift = p->format.bshift; Q.amask = p->format.amask;
    Q.out_px = d_pixels;
    Q.out_rgb = d_rgb;
    return shade_launch(c, Q);
}

extern "C" int rtx_shade_rays(rtx_ctx* c, const rtx_ray* rays, uint32_t n, const rtx_render_params* p, uint32_t* out_pixels,
                              float* out_rgb) {
    if (const int rc = shade_check(c, rays, n, p, out_pixels, out_rgb); rc != RTX_OK) return rc;
    if (n == 0) return RTX_OK;
    if (!c->has_scene) return fail(c, RTX_E_STATE, "no scene uploaded");
    if (const int rc = stage(c, rays, n); rc != RTX_OK) return rc;
    const size_t cap = c->d_query.cap, N = n;
    uint32_t* d_px = out_pixels ? reinterpret_cast<uint32_t*>(c->d_query + kOffPixels * cap) : nullptr;
    float* d_rgb = out_rgb ? reinterpret_cast<float*>(c->d_query + kOffRgb * cap) : nullptr;
    if (const int rc = rtx_shade_rays_device(c, reinterpret_cast<const rtx_ray*>(c->d_query.get()), n, p, d_px, d_rgb);
        rc != RTX_OK)
        return rc;
    if (out_pixels) HIP_TRY(c, hipMemcpyAsync(out_pixels, d_px, N * 4u, hipMemcpyDeviceToHost, c->stream));
    if (out_rgb) HIP_TRY(c, hipMemcpyAsync(out_rgb, d_rgb, N * 12u, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}

extern "C" int rtx_time_shade_rays(rtx_ctx* c, const rtx_ray* d_rays, uint32_t n, const rtx_render_params* p,
                                   uint32_t* d_pixels, float* d_rgb, int iters, float* mean_ms) {
    if (!c || !d_rays || !p || !mean_ms || iters <= 0 || n == 0) return RTX_E_INVALID;
    // one full call first: its checks and a pending chain's join stay outside the timing of the public entry point
    if (const int rc = rtx_shade_rays_device(c, d_rays, n, p, d_pixels, d_rgb); rc != RTX_OK) return rc;
    return timed_loop(c, iters, mean_ms, [&](int) { return rtx_shade_rays_device(c, d_rays, n, p, d_pixels, d_rgb); });
}
