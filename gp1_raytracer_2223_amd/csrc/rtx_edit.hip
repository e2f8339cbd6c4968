// rtx_edit.hip — in-place edits of the current scene image (rtx_edit_*, rtx.h): light and material records
// replaced on the context stream by one small kernel, and the host state an upload would have derived from
// them.  The records and the derived values are the packer's own (rtx_pack.h: pack_light_edit,
// pack_material_edit), so an edited image is the image an upload of the edited scene writes, byte for byte.
#include <algorithm>
#include <cstring>

#include "rtx_ctx.h"

using namespace rtxh;

// The host forms' payload travels BY VALUE in the kernel arguments, at most kPatchWords words a launch: no
// staging buffer whose lifetime would need an event, no copy from pageable memory that blocks, and no race
// with an earlier upload's still-pending copy out of the pinned image.  A launch carries up to kPatchSegs
// contiguous pieces of the image (a light edit's records, the room-skip record and the cull bounds).
constexpr uint32_t kPatchWords = 768;   // 3 KB
constexpr int kPatchSegs = 3;
enum PatchMode : uint32_t { kPatchWordsMode = 0, kPatchLightValues = 1, kPatchMaterialValues = 2 };
struct PatchArgs {
    uint32_t mode;
    uint32_t n;                            // words of payload (kPatchWordsMode), else records
    unsigned long long seg_dst[kPatchSegs];   // kPatchWordsMode: each piece's first word in the image; else
                                              // [0] = the first edited record's
    uint32_t seg_end[kPatchSegs];          // one past each piece's last payload word (pieces in payload order)
    uint32_t w[kPatchWords];
};
static_assert(kPatchSegs == 3, "rtx_patch_kernel finds a word's piece with two compares");
static_assert(sizeof(PatchArgs) + 16 <= 4096, "the kernel arguments' limit");

// kPatchWordsMode: thread i stores payload word i.  The value modes read the caller's device floats, one
// record a thread: a light's {color, intensity} becomes its second record; a material's {color, kd, ks,
// exponent, metalness, roughness} its three records but for the kind, with the Lambert term (color * kd) / PI
// as material_records computes it on the host: the product rounded (no contraction), then the correctly
// rounded IEEE division every input range takes (-fhip-fp32-correctly-rounded-divide-sqrt), so every finite
// input gives the host's bits.  `src` needs no more than a float's alignment.
__global__ void __launch_bounds__(256) rtx_patch_kernel(uint32_t* __restrict__ image, const float* __restrict__ src,
                                                        const PatchArgs A) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= A.n) return;
    if (A.mode == kPatchWordsMode) {
        // the piece word i belongs to (an unused piece ends at UINT32_MAX)
        const bool p1 = i >= A.seg_end[0], p2 = i >= A.seg_end[1];
        const unsigned long long dst = p2 ? A.seg_dst[2] : (p1 ? A.seg_dst[1] : A.seg_dst[0]);
        const uint32_t base = p2 ? A.seg_end[1] : (p1 ? A.seg_end[0] : 0u);
        image[dst + (i - base)] = A.w[i];
    } else if (A.mode == kPatchLightValues) {
        const float* v = src + 4ull * i;
        float4* rec = reinterpret_cast<float4*>(image + A.seg_dst[0]) + 2ull * i;
        rec[1] = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        const float* v = src + 8ull * i;
        const float cr = v[0], cg = v[1], cb = v[2], kd = v[3];
        float* rec = reinterpret_cast<float*>(image + A.seg_dst[0]) + 12ull * i;
        const float lr = (cr * kd) / RTX_PI, lg = (cg * kd) / RTX_PI, lb = (cb * kd) / RTX_PI;
        rec[1] = cr; rec[2] = cg; rec[3] = cb;   // (word 0 is the kind)
        reinterpret_cast<float4*>(rec)[1] = make_float4(kd, v[4], v[5], v[6]);
        reinterpret_cast<float4*>(rec)[2] = make_float4(v[7], lr, lg, lb);
    }
}

namespace {

int patch_launch(rtx_ctx* c, const PatchArgs& A, const float* src) {
    uint32_t* image = reinterpret_cast<uint32_t*>(c->sb[c->sb_cur].d);
    hipLaunchKernelGGL(rtx_patch_kernel, dim3((A.n + 255u) / 256u), dim3(256), 0, c->stream, image, src, A);
    HIP_TRY(c, hipGetLastError());
    return RTX_OK;
}

// Queue the ranges' words, kPatchWords and kPatchSegs a launch, in order.
int patch_ranges(rtx_ctx* c, const std::vector<EditRange>& ranges) {
    PatchArgs A{};
    int n_seg = 0;
    auto flush = [&]() {
        for (int k = n_seg; k < kPatchSegs; ++k) A.seg_end[k] = UINT32_MAX;
        const int rc = A.n ? patch_launch(c, A, nullptr) : RTX_OK;
        A.n = 0;
        n_seg = 0;
        return rc;
    };
    for (const EditRange& r : ranges)
        for (size_t pos = 0; pos < r.words.size();) {
            if (n_seg == kPatchSegs || A.n == kPatchWords)
                if (const int rc = flush(); rc != RTX_OK) return rc;
            const uint32_t take = static_cast<uint32_t>(std::min<size_t>(r.words.size() - pos, kPatchWords - A.n));
            A.seg_dst[n_seg] = r.off / 4 + pos;
            std::memcpy(A.w + A.n, r.words.data() + pos, 4 * static_cast<size_t>(take));
            A.n += take;
            A.seg_end[n_seg++] = A.n;
            pos += take;
        }
    return flush();
}

// What every edit checks before its own records, in rtx.h's order.
int edit_checks(rtx_ctx* c, const void* records, uint32_t first, uint32_t n, size_t count, const char* what) {
    if (!c) return RTX_E_INVALID;
    if (n && !records) return fail(c, RTX_E_INVALID, std::string("NULL ") + what + " with n > 0");
    if (c->has_scene && (first > count || n > count - first))   // (first + n without overflow)
        return fail(c, RTX_E_INVALID, std::string(what) + " " + std::to_string(first) + " .. +" + std::to_string(n) +
                                          " beyond the uploaded " + std::to_string(count));
    if (!c->has_scene) return fail(c, RTX_E_STATE, "no scene uploaded");
    return RTX_OK;
}

int edit_registered(rtx_ctx* c) {
    if (c->edit_ok) return RTX_OK;
    return fail(c, RTX_E_UNSUPPORTED, "the current image belongs to a device Update's registration: upload the scene to edit it");
}

// The edit's place on the context stream: behind the last frame's split chain, which reads the image.
int edit_begin(rtx_ctx* c) {
    HIP_TRY(c, hipSetDevice(c->device));
    return join_split(c);
}

int edit_values_device(rtx_ctx* c, uint32_t first, uint32_t n, const float* d_values, PatchMode mode) {
    const bool lights = mode == kPatchLightValues;
    const size_t count = lights ? c->edit.lights.size() : c->edit.kinds.size();
    if (const int rc = edit_checks(c, d_values, first, n, count, lights ? "lights" : "materials"); rc != RTX_OK) return rc;
    if (const int rc = edit_registered(c); rc != RTX_OK) return rc;
    if (n == 0) return RTX_OK;
    if (const int rc = edit_begin(c); rc != RTX_OK) return rc;
    // (values only: no host state follows them.  The pinned image and EditInputs' copies of the lights keep the
    // earlier colours; nothing reads either again: later copies come from a new emit, edits from the caller's records)
    PatchArgs A{};
    A.mode = mode;
    A.n = n;
    A.seg_dst[0] = lights ? (c->edit.off_lights + 32 * static_cast<size_t>(first)) / 4
                          : (c->edit.off_mats + 48 * static_cast<size_t>(first)) / 4;
    return patch_launch(c, A, d_values);
}

}  // namespace

extern "C" int rtx_edit_lights(rtx_ctx* c, uint32_t first, uint32_t n, const rtx_light* lights) {
    if (const int rc = edit_checks(c, lights, first, n, c ? c->edit.lights.size() : 0, "lights"); rc != RTX_OK) return rc;
    LightPatch patch;
    std::string err;
    if (const int rc = pack_light_edit(c->edit, first, n, lights, patch, err); rc != RTX_OK) return fail(c, rc, err);
    if (const int rc = edit_registered(c); rc != RTX_OK) return rc;
    if (n == 0) return RTX_OK;
    if (const int rc = edit_begin(c); rc != RTX_OK) return rc;
    if (const int rc = patch_ranges(c, patch.ranges); rc != RTX_OK) return rc;
    // the pinned image too (only copies queued before this call read it)
    apply_ranges(patch.ranges, c->sb[c->sb_cur].h);
    if (patch.moved) {   // the host's share of what an upload derives from the lights' origins
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t l = first + i;
            if (!patch.moved_l[l]) continue;
            std::memcpy(c->light_keys[l].data(), patch.ranges[0].words.data() + 8 * static_cast<size_t>(i), 16);
            if (c->dev.cull_stride && l < c->cull_lights.size()) {   // its exact-cull anchor (cull_records)
                const float T = patch.cull_T.empty() ? 0.f : patch.cull_T[i];
                const rtx_light& L = patch.lights[l];
                c->cull_lights[l] = {L.origin[0], L.origin[1], L.origin[2], T > 0.f ? T : 1.f};
                if (!c->cull_boxes_pending) c->cull_lights_dirty |= 1u << l;   // (a pending build takes every light)
            }
        }
        c->facts.room_fact = patch.room_fact;
        c->facts.room_M = patch.room_M;
    }
    commit_light_edit(c->edit, patch);
    return RTX_OK;
}

extern "C" int rtx_edit_materials(rtx_ctx* c, uint32_t first, uint32_t n, const rtx_material* materials) {
    if (const int rc = edit_checks(c, materials, first, n, c ? c->edit.kinds.size() : 0, "materials"); rc != RTX_OK)
        return rc;
    MaterialPatch patch;
    std::string err;
    if (const int rc = pack_material_edit(c->edit, first, n, materials, patch, err); rc != RTX_OK) return fail(c, rc, err);
    if (const int rc = edit_registered(c); rc != RTX_OK) return rc;
    if (n == 0) return RTX_OK;
    if (const int rc = edit_begin(c); rc != RTX_OK) return rc;
    if (const int rc = patch_ranges(c, patch.ranges); rc != RTX_OK) return rc;
    apply_ranges(patch.ranges, c->sb[c->sb_cur].h);
    return RTX_OK;
}

extern "C" int rtx_edit_light_values_device(rtx_ctx* c, uint32_t first, uint32_t n, const float* d_values) {
    if (!c) return RTX_E_INVALID;
    return edit_values_device(c, first, n, d_values, kPatchLightValues);
}

extern "C" int rtx_edit_material_values_device(rtx_ctx* c, uint32_t first, uint32_t n, const float* d_values) {
    if (!c) return RTX_E_INVALID;
    return edit_values_device(c, first, n, d_values, kPatchMaterialValues);
}
