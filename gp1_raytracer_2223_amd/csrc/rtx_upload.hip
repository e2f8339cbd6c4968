// rtx_upload.hip — the commit of a packed scene (rtx_pack.h) to the context: its next HBM image,
// the copies, DevScene and the context's scene state.  The upload-time knobs are read here.
#include <cstdlib>
#include <cstring>

#include "rtx_ctx.h"

using namespace rtxh;

extern "C" int rtx_upload_scene(rtx_ctx* c, const rtx_scene* s) {
    if (c) {   // the upload pattern the cull decision reads (see rtx_ctx::cull_animated)
        c->short_uploads = (c->has_scene && c->renders_since_upload <= 1) ? c->short_uploads + 1 : 0;
        c->renders_since_upload = 0;
        c->motion.upload_motion = c->short_uploads >= 1;
        if (const int rc = join_split(c); rc != RTX_OK) return rc;   // (the last chain reads the current image)
    }
    PackedScene P;
    return upload_scene(c, s, {}, P);
}

namespace rtxh {

int next_image(rtx_ctx* c, size_t total, int& k) {
    k = c->sb_cur < 0 ? 0 : (c->sb_cur ^ 1);
    rtx_ctx::SceneBuf& B = c->sb[k];
    if (B.pending) {   // frames queued against image k (two uploads ago) must be done with it
        HIP_TRY(c, hipEventSynchronize(B.done));
        B.pending = false;
    }
    if (total > B.cap) HIP_TRY(c, B.grow(total));
    return RTX_OK;
}

int adopt_image(rtx_ctx* c, int k, size_t total) {
    if (c->sb_cur >= 0) {   // every frame queued so far reads the previous image
        rtx_ctx::SceneBuf& O = c->sb[c->sb_cur];
        HIP_TRY(c, hipEventRecord(O.done, c->stream));
        O.pending = true;
    }
    c->sb_cur = k;
    c->scene_bytes = total;
    return RTX_OK;
}

namespace {

// What the packer reads from the context, and from the environment at every upload.
PackOptions pack_options(const rtx_ctx* c, const rtx_scene* s, const std::vector<uint8_t>& reserve) {
    PackOptions o;
    if (const char* ev = std::getenv("RTX_PART_REFINE"))   // experiment: split the listed parts once more
        for (const char* q = ev; *q;) {
            char* end = nullptr;
            const long v = std::strtol(q, &end, 10);
            if (end == q) break;
            o.part_refine.push_back(static_cast<int>(v));
            q = *end ? end + 1 : end;
        }
    o.no_octant = std::getenv("RTX_NO_OCTANT") != nullptr;
    o.split_parts = c->split_parts;
    o.cull_min_sa = c->cull_min_sa;
    // exact cull (DevScene::cull): host uploads (a device-animated image is rebuilt in place and
    // carries no records), at most kMaxCullLights lights
    o.want_cull = reserve.empty() && !c->no_cull && s->n_lights <= static_cast<uint32_t>(kMaxCullLights) &&
                  (c->short_uploads < 2 || c->cull_animated);
    o.worth_reuse = c->short_uploads >= 1 && c->cull_worth >= 0 && c->cull_worth_age + 1 < kCullWorthReuse;
    o.worth = c->cull_worth == 1;
    o.worth_sig = c->cull_worth_sig;
    o.room_skip_off = c->room_skip_off;
    o.reserve = reserve;
    return o;
}

// Large node arrays send copy 0 only and the device writes copies 1..7 (rtx_octant_expand):
// 1/8 of the node bytes over PCIe and of the host's staging writes (an upload per animated
// frame).  Small ones are cheaper as host writes than as one more launch.
int queue_copies(rtx_ctx* c, const PackedScene& P, rtx_ctx::SceneBuf& B, bool oct_dev) {
    if (!oct_dev) {
        HIP_TRY(c, hipMemcpyAsync(B.d, B.h, P.total, hipMemcpyHostToDevice, c->stream));
        return RTX_OK;
    }
    // everything but copies 1..7, which the device writes
    const size_t c0 = P.sec[kSecNodes].off, c1 = c0 + P.node_bytes, c8 = c0 + 8 * P.node_bytes;
    HIP_TRY(c, hipMemcpyAsync(B.d, B.h, c1, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(B.d + c8, B.h + c8, P.total - c8, hipMemcpyHostToDevice, c->stream));
    octant_expand(reinterpret_cast<float4*>(B.d + c0), static_cast<uint32_t>(P.node_bytes / 32),
                  static_cast<uint32_t>(P.node_bytes / 16), c->stream);
    HIP_TRY(c, hipGetLastError());
    return RTX_OK;
}

DevScene dev_scene(const PackedScene& P, const rtx_ctx::SceneBuf& B) {
    DevScene d{};
    auto at = [&](Section i) { return B.d + P.sec[i].off; };
    d.spheres = reinterpret_cast<const float4*>(at(kSecSpheres));
    d.sphere_mat = reinterpret_cast<const uint32_t*>(at(kSecSphereMat));
    d.planes = reinterpret_cast<const float4*>(at(kSecPlanes));
    d.tris = reinterpret_cast<const Tri*>(at(kSecTris));
    d.nodes = reinterpret_cast<const float4*>(at(kSecNodes));
    d.meshes = reinterpret_cast<const int4*>(at(kSecMeshes));
    d.lights = reinterpret_cast<const float4*>(at(kSecLights));
    d.materials = reinterpret_cast<const float4*>(at(kSecMaterials));
    d.parts = reinterpret_cast<const int4*>(at(kSecParts));
    d.n_parts = P.n_parts;
    d.n_spheres = P.n_spheres; d.n_planes = P.n_planes; d.n_meshes = P.n_meshes;
    d.n_lights = P.n_lights; d.n_materials = P.n_materials;
    d.tri_fast = P.tri_fast;
    d.oct_bytes = P.oct_bytes;
    d.n_tris = P.n_tris; d.n_nodes = P.n_nodes;
    if (P.cull_on) {
        d.cull = B.cull;
        d.cull_T = reinterpret_cast<const float*>(at(kSecCullT));
        d.cull_stride = static_cast<uint32_t>(P.cull_stride);
    }
    return d;
}

// The context's scene state, in one block after the last call of an upload that can fail.
void set_scene_state(rtx_ctx* c, const PackedScene& P, const rtx_ctx::SceneBuf& B) {
    if (P.worth_from == PackedScene::kWorthReused) ++c->cull_worth_age;
    if (P.worth_from == PackedScene::kWorthComputed) {
        c->cull_worth = P.worth ? 1 : 0;
        c->cull_worth_age = 0;
        c->cull_worth_sig = P.worth_sig;
    }
    if (P.cull_on) {
        c->cull_rng = reinterpret_cast<const uint2*>(B.d + P.sec[kSecCullRng].off);
        c->cull_nslots = P.n_nodes;
        for (int a = 0; a < 3; ++a) { c->cull_bmin[a] = P.bmin[a]; c->cull_bmax[a] = P.bmax[a]; }
        c->cull_ntris = P.n_tris;
        c->cull_n = P.cull_n;
    }
    c->cull_view_valid = 0;
    c->dev = dev_scene(P, B);
    c->cull_boxes_pending = false;
    c->cull_lights_dirty = 0;
    c->facts = P.facts;
    c->last_facts = c->facts.spec;   // (rtx_spec_info before the first frame)
    c->last_variant = -1;
    c->refinable = P.refinable && c->facts.split_ok && !c->refine.off;
    c->h_parts.assign(P.parts.begin(), P.parts.begin() + static_cast<std::ptrdiff_t>(P.n_parts));
    c->h_parts_base = c->h_parts;
    c->parts_dev = reinterpret_cast<int4*>(B.d + P.sec[kSecParts].off);
    c->refine.reset_upload(c->refinable);
    // the lights a shadow ray depends on (origin and type, bit for bit): rtx_relight's validity check
    c->light_keys.resize(P.n_lights);
    for (uint32_t i = 0; i < P.n_lights; ++i) {
        const float4 l = P.lights[2 * i];
        std::memcpy(c->light_keys[i].data(), &l, 16);
    }
    c->has_scene = true;
    ++c->scene_gen;
}

}  // namespace

int upload_scene(rtx_ctx* c, const rtx_scene* s, const std::vector<uint8_t>& reserve, PackedScene& P) {
    if (!c || !s) return RTX_E_INVALID;
    std::string err;
    const PackOptions opt = pack_options(c, s, reserve);
    if (const int rc = pack_scene(s, opt, P, err); rc != RTX_OK) return fail(c, rc, err);
    HIP_TRY(c, hipSetDevice(c->device));
    int k = 0;
    if (const int rc = next_image(c, P.total, k); rc != RTX_OK) return rc;
    rtx_ctx::SceneBuf& B = c->sb[k];
    // cull records: one copy of the node slots per anchor (kMaxViews cameras, then the lights)
    const size_t cull_bytes = P.cull_on ? (kMaxViews + static_cast<size_t>(P.n_lights)) * P.cull_stride : 0;
    if (cull_bytes > B.cull.cap)
        if (const int rc = B.cull.grow(c, cull_bytes, 1); rc != RTX_OK) return rc;
    const bool oct_dev = P.oct_ok && P.node_bytes >= kOctantDeviceMinBytes;
    emit(P, B.h, oct_dev ? 1 : 8);
    if (const int rc = queue_copies(c, P, B, oct_dev); rc != RTX_OK) return rc;
    if (const int rc = adopt_image(c, k, P.total); rc != RTX_OK) return rc;
    set_scene_state(c, P, B);
    edit_inputs(s, opt, P, c->edit);   // (what rtx_edit_* needs of this scene)
    c->edit_ok = reserve.empty();
    if (P.cull_on) cull_records(c, P.cull_T, s->lights, s->n_lights);   // (built before the first frame)
    return RTX_OK;
}

}  // namespace rtxh
