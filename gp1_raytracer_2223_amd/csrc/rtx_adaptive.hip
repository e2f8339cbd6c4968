// rtx_adaptive.hip — adaptive supersampling behind the C-ABI (rtx_render_adaptive*, rtx_adaptive_refined,
// rtx_time_adaptive_frames): the contrast classifier over the frame buffer (rtx_classify_kernel), the
// checks, the pixel list and the launches.  The refinement kernel is rtx_hip.hip's rtx_adaptive_kernel.
#include <algorithm>

#include "rtx_ctx.h"
#include "rtx_launch.h"

using namespace rtxh;

namespace {

// |channel of a - channel of b| > tau in some channel (channel c = (word >> shift_c) & 255): integers only
__device__ __forceinline__ bool differs(uint32_t a, uint32_t b, const ClassifyArgs& A) {
    const int dr = static_cast<int>((a >> A.rshift) & 255u) - static_cast<int>((b >> A.rshift) & 255u);
    const int dg = static_cast<int>((a >> A.gshift) & 255u) - static_cast<int>((b >> A.gshift) & 255u);
    const int db = static_cast<int>((a >> A.bshift) & 255u) - static_cast<int>((b >> A.bshift) & 255u);
    const int t = static_cast<int>(A.tau);
    return abs(dr) > t || abs(dg) > t || abs(db) > t;
}

}  // namespace

// The mask E of rtx.h and its compaction.  One lane per pixel in row-major order, so a wave's reads of its
// own words and of each neighbour are runs of consecutive addresses.  The wave's flagged lanes are counted
// by a ballot, one atomicAdd per wave with a flagged lane reserves their range of the list, and each
// flagged lane writes y << 16 | x at its rank in the range.  Plain vector atomics and stores.
__global__ void __launch_bounds__(kClassifyThreads) rtx_classify_kernel(const ClassifyArgs A) {
    const uint32_t i = blockIdx.x * kClassifyThreads + threadIdx.x;
    const uint32_t n = A.width * A.height;
    bool e = false;
    uint32_t x = 0, y = 0;
    if (i < n) {
        y = i / A.width;
        x = i - y * A.width;
        const uint32_t w = A.px[i];
        if (x > 0) e |= differs(w, A.px[i - 1u], A);
        if (x + 1u < A.width) e |= differs(w, A.px[i + 1u], A);
        if (y > 0) e |= differs(w, A.px[i - A.width], A);
        if (y + 1u < A.height) e |= differs(w, A.px[i + A.width], A);
    }
    const unsigned long long m = __builtin_amdgcn_ballot_w64(e);
    if (m == 0) return;   // (wave-uniform)
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(A.count, static_cast<uint32_t>(__popcll(m)));
    base = __builtin_amdgcn_readfirstlane(base);   // (every lane is active here: the first one is lane 0)
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32),
                                                    __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
    if (e) A.list[base + rank] = (y << 16) | x;   // base + rank < |E| <= width * height, the list's size
}

namespace {

uint32_t factor_log2(uint32_t k) { return k == 8 ? 3u : (k == 4 ? 2u : (k == 2 ? 1u : 0u)); }

// An adaptive frame's checks in the order of rtx.h's error table; nothing is queued before they pass.
int adaptive_check(rtx_ctx* c, const rtx_camera* cam, const rtx_render_params* p, uint32_t k, uint32_t tau) {
    if (!c) return RTX_E_INVALID;
    if (k != 2 && k != 4 && k != 8)
        return fail(c, RTX_E_INVALID, "adaptive factor must be 2, 4 or 8 (got " + std::to_string(k) + ")");
    if (tau > 255) return fail(c, RTX_E_INVALID, "adaptive threshold must be 0..255 (got " + std::to_string(tau) + ")");
    if (const int rc = check_params(c, cam, 1, p); rc != RTX_OK) return rc;
    const uint32_t n = factor_log2(k);
    if ((static_cast<uint64_t>(p->width) << n) > 65536 || (static_cast<uint64_t>(p->height) << n) > 65536)
        return fail(c, RTX_E_INVALID, "bad image size: adaptive " + std::to_string(k) + "x" + std::to_string(k) +
                                          ", the sample frame exceeds 65536 per side");
    if (c->ss_log2)
        return fail(c, RTX_E_UNSUPPORTED, "an adaptive frame carries its own factor: the context's supersample factor must be 1");
    if (p->stripe_rows != 0 && p->stripe_step > 1)
        return fail(c, RTX_E_UNSUPPORTED, "an adaptive frame has no stripes: a stripe's neighbour rows belong to another context");
    return RTX_OK;
}

// Queue, behind the plain frame in the frame buffer, the counter reset, the classification and the
// refinement of the classified pixels.
int adaptive_launch(rtx_ctx* c, const rtx_camera* cam, const rtx_render_params* p, bool want_rgb, uint32_t k,
                    uint32_t tau) {
    const uint32_t n = factor_log2(k);
    const size_t npx = static_cast<size_t>(p->width) * p->height;
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = join_split(c); rc != RTX_OK) return rc;   // (the chain writes the heavy tiles' pixels)
    if (npx > c->d_adapt_list.cap) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));   // (an earlier adaptive frame may still read the old list)
        if (const int rc = c->d_adapt_list.grow(c, npx); rc != RTX_OK) return rc;
    }
    if (!c->d_adapt_count)
        if (const int rc = c->d_adapt_count.grow(c, 1); rc != RTX_OK) return rc;
    HIP_TRY(c, hipMemsetAsync(c->d_adapt_count, 0, sizeof(uint32_t), c->stream));

    ClassifyArgs K{};
    K.px = c->d_px;
    K.width = p->width; K.height = p->height;
    K.tau = tau;
    K.rshift = p->format.rshift; K.gshift = p->format.gshift; K.bshift = p->format.bshift;
    K.list = c->d_adapt_list;
    K.count = c->d_adapt_count;
    const uint32_t kblocks = static_cast<uint32_t>((npx + kClassifyThreads - 1) / kClassifyThreads);
    hipLaunchKernelGGL(rtx_classify_kernel, dim3(kblocks), dim3(kClassifyThreads), 0, c->stream, K);
    HIP_TRY(c, hipGetLastError());

    AdaptiveArgs A{};
    for (int i = 0; i < 3; ++i) {
        A.origin[i] = cam->origin[i]; A.right[i] = cam->right[i];
        A.up[i] = cam->up[i]; A.forward[i] = cam->forward[i];
    }
    A.fov = cam->fov;
    // the sample frame's, as frame_shape fills a supersampled frame's FrameArgs
    const uint32_t sw = p->width << n, sh = p->height << n;
    A.aspect = static_cast<int>(sw) / static_cast<float>(static_cast<int>(sh));   // Renderer.cpp:30
    A.inv_width = 1.f / static_cast<float>(static_cast<int>(sw));
    A.inv_height = 1.f / static_cast<float>(static_cast<int>(sh));
    A.width = sw; A.height = sh;
    A.out_width = p->width;
    A.ss_log2 = n;
    A.mode = p->lighting_mode; A.shadows = p->shadows_enabled ? 1 : 0;
    A.rshift = p->format.rshift; A.gshift = p->format.gshift; A.bshift = p->format.bshift; A.amask = p->format.amask;
    A.list = c->d_adapt_list;
    A.count = c->d_adapt_count;
    A.out_px = c->d_px;
    A.out_rgb = want_rgb ? c->d_rgb.get() : nullptr;
    // persistent waves: the device's wave slots, and never more than the items of a full list
    const size_t items = (npx + (64u >> (2u * n)) - 1u) >> (6u - 2u * n);
    const uint32_t waves = static_cast<uint32_t>(std::min<size_t>(c->adapt_waves, items));
    const dim3 grid((waves + kWavesPerBlock - 1u) / kWavesPerBlock);
    if (c->facts.hbm_stack)
        if (const int rc = ensure_hbm_stacks(c, grid.x); rc != RTX_OK) return rc;
    launch_adaptive(c->facts.deep_stack || c->facts.hbm_stack, c->facts.hbm_stack, grid, c->stream, c->dev, A);
    HIP_TRY(c, hipGetLastError());
    c->adapt_valid = true;
    return RTX_OK;
}

}  // namespace

extern "C" int rtx_render_adaptive_async(rtx_ctx* c, const rtx_camera* cam, const rtx_render_params* p, int want_rgb,
                                         uint32_t k, uint32_t threshold) {
    if (const int rc = adaptive_check(c, cam, p, k, threshold); rc != RTX_OK) return rc;
    if (const int rc = rtx_render_async(c, cam, p, want_rgb); rc != RTX_OK) return rc;   // P, as any plain frame
    return adaptive_launch(c, cam, p, want_rgb != 0, k, threshold);
}

extern "C" int rtx_render_adaptive(rtx_ctx* c, const rtx_camera* cam, const rtx_render_params* p, uint32_t k,
                                   uint32_t threshold, uint32_t* out_px, float* out_rgb) {
    if (!out_px) return RTX_E_INVALID;
    if (const int rc = rtx_render_adaptive_async(c, cam, p, out_rgb != nullptr, k, threshold); rc != RTX_OK) return rc;
    return rtx_download(c, out_px, out_rgb);
}

extern "C" int rtx_adaptive_refined(rtx_ctx* c, uint32_t* n_refined) {
    if (!c || !n_refined) return RTX_E_INVALID;
    if (!c->adapt_valid) return fail(c, RTX_E_STATE, "no adaptive frame rendered yet");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(n_refined, c->d_adapt_count, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}

extern "C" int rtx_time_adaptive_frames(rtx_ctx* c, const rtx_camera* cam, const rtx_render_params* p, uint32_t k,
                                        uint32_t threshold, int iters, float* mean_ms) {
    if (!mean_ms || iters <= 0) return RTX_E_INVALID;
    // one full call first: its checks, buffer growth and a new shape's schedule stay outside the timing
    if (const int rc = rtx_render_adaptive_async(c, cam, p, 0, k, threshold); rc != RTX_OK) return rc;
    return timed_loop(c, iters, mean_ms, [&](int) { return rtx_render_adaptive_async(c, cam, p, 0, k, threshold); });
}
