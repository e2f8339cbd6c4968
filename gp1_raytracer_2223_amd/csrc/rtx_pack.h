// rtx_pack.h — a host scene packed into the bytes of a scene image (rtx_kernels.h's layout), before
// any device is touched: the device numbering of the BVHs, the split frontier, the cull records'
// inputs, the kernel facts.  Plain C++ (no HIP runtime call, no environment, no context), so
// tests/pack_harness.cpp drives it on the CPU; rtx_upload.hip commits the result to the context.
#pragma once

#include <hip/hip_vector_types.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "rtx.h"
#include "rtx_kernels.h"

namespace rtxh {

// What the frame code needs to know of the uploaded scene besides its DevScene (rtx_ctx::facts; a
// registered animation keeps its registration's, rtx_anim::facts).
struct SceneFacts {
    bool split_ok = false;    // the scene admits split rendering
    bool deep_stack = false;  // it needs rtx_render_kernel<..., DEEP = true>: kStackDepth or more levels
    bool hbm_stack = false;   // ... with its stacks in HBM (HSTK = true): kStackDepthDeep or more levels
    uint32_t max_depth = 0;   // deepest BVH level
    int spec = 0;             // kSpec* facts (kernel specialisation)
    float room_p0[5] = {};    // kSpecRoomPlanes: plane k's origin on axis kRoomAxes[k]
    // room skip (room_skip in rtx_pack.cpp): every light strictly inside the room, and the bound on the
    // shadow origins' plane distances; RTX_ROOM_SKIP=0: off (the fact is then reported false)
    bool room_fact = false;
    float room_M = 0.f;
    std::string sig;          // topology (keeps the tile schedule across re-uploads)
};

// What the packer reads from the context and the environment.
struct PackOptions {
    uint32_t split_parts = rtxd::kPartsPerMesh;   // frontier target per mesh
    double cull_min_sa = 1.5;                     // the worth test's ratio
    // Cull inputs wanted: a host upload (a device-animated image is rebuilt in place and carries no
    // records) of a context whose cull is on; the packer adds the scene's own conditions.
    bool want_cull = false;
    // The worth cache: the caller's side of the reuse condition (an animated loop, a verdict
    // young enough), the cached verdict and the counts it was made for (PackedScene::worth_sig).
    bool worth_reuse = false;
    bool worth = false;
    std::string worth_sig;
    bool room_skip_off = false;
    bool no_octant = false;          // DevScene::oct_bytes 0 (the image keeps its copies)
    std::vector<int> part_refine;    // experiment: frontier entries of each mesh to split once more
    // Per mesh (empty: none), for a device Update's registration: a mesh with reserve[i] set owns 2T
    // node slots from its root (the most a rebuild can number) and exactly `target` frontier entries
    // (unused ones are {-1, ...}), so a device rebuild can rewrite it in place without moving
    // anything else.
    std::vector<uint8_t> reserve;
};

enum Section {
    kSecSpheres, kSecSphereMat, kSecPlanes, kSecTris, kSecNodes, kSecMeshes, kSecLights, kSecMaterials, kSecParts,
    kSecCullRng, kSecCullT, kSecCount
};

struct PackedScene {
    // the sections' records (the node section is written from `nodes` by emit: 1 or 8 copies)
    std::vector<float4> sph, pl, tri, nodes, lights, mats;
    std::vector<uint32_t> sph_mat;
    std::vector<int4> meshes, parts;
    std::vector<uint2> cull_rng;   // per device node slot: its triangles (slot_ranges)
    std::vector<float> cull_T;     // per light: the tmax up to which its shadow rays are culled
    struct Sec { size_t n, off; };   // bytes, and offset in the image (a multiple of 256)
    Sec sec[kSecCount] = {};
    size_t total = 0;
    size_t node_bytes = 0;         // one copy of the node array, padded: the octant copies' stride
    bool oct_ok = false;           // the node section holds 8 octant copies
    // DevScene's counts and flags
    uint32_t n_spheres = 0, n_planes = 0, n_meshes = 0, n_lights = 0, n_materials = 0, n_tris = 0, n_nodes = 0;
    uint32_t n_parts = 0;          // the frontier's real entries (parts[0 .. n_parts))
    uint32_t tri_fast = 0, oct_bytes = 0;
    SceneFacts facts;
    bool refinable = false;        // the parts section reserves kMaxParts entries for the refinement
    // cull inputs (DevScene::cull): the verdict, the records' copy stride, the meshes' box, the
    // segment trees' leaf count (a power of two >= the triangles)
    bool cull_on = false;
    size_t cull_stride = 0;
    double bmin[3] = {}, bmax[3] = {};
    uint32_t cull_n = 0;
    // the worth estimate: whether this upload made one or used the cached one (none: the cache
    // stays as it is), its verdict and the counts it holds for
    enum Worth { kWorthNone, kWorthReused, kWorthComputed } worth_from = kWorthNone;
    bool worth = false;
    std::string worth_sig;
    // per mesh, for a device Update's registration (part0 / part_cap of reserved meshes only)
    struct MeshLayout { uint32_t tri0 = 0, root = 0, part0 = 0, part_cap = 0; int depth = 0; };
    std::vector<MeshLayout> mesh_layout;
    double max_ee = 0.0;           // max |e1| * |e2| over the triangles (DevScene::tri_fast)
    double max_se = 0.0;           // max (|v0|_1 + 2^40) (|e1|_1 + |e2|_1): bounds every |o - v0| x e term (tri_fast)
};

// Pack `s`.  RTX_OK, or the refusal's code with its reason in `err` (`out` is then unspecified).
int pack_scene(const rtx_scene* s, const PackOptions& opt, PackedScene& out, std::string& err);

// Write the image (P.total bytes) to `dst`: sections in place, the node section as 8 octant copies
// when P.oct_ok and host_octant_copies is 8 (1: copy 0 only; the device writes the rest), and only
// the padding up to the next section cleared (an upload per animated frame: no full-image memset, no
// intermediate node image).
void emit(const PackedScene& P, char* dst, int host_octant_copies);

// ---- in-place edits of the light and material records (rtx_edit.hip) --------------------------------
// What the values derived from the lights and materials need of the packed scene besides the edited
// records themselves: a context retains it at upload, so an edit never needs the caller's scene again.
struct EditInputs {
    bool room = false;             // the five planes are the room's (kSpecRoomPlanes)
    bool room_skip_off = false;    // PackOptions::room_skip_off
    float room_p0[5] = {}, room_n[5] = {};   // plane k's origin and normal on axis kRoomAxes[k]
    bool has_cull_T = false;       // the image holds a kSecCullT entry per light
    double bmin[3] = {}, bmax[3] = {};       // the meshes' box (cull_tmax)
    size_t off_planes = 0, off_lights = 0, off_mats = 0, off_cull_T = 0;   // the sections' offsets in the image
    std::vector<rtx_light> lights;           // as uploaded, then as edited (direction unused)
    std::vector<int32_t> kinds;              // per material
    SceneFacts facts;              // room_fact and room_M follow the edits
};
void edit_inputs(const rtx_scene* s, const PackOptions& opt, const PackedScene& P, EditInputs& E);

// The bytes an edit replaces: 32-bit words at byte offset `off` of the image, in the packer's own encoding.
struct EditRange {
    size_t off = 0;
    std::vector<uint32_t> words;
};
struct LightPatch {
    std::vector<EditRange> ranges;   // the light records; with a moved light, the room-skip record and cull_T too
    uint32_t moved = 0;              // lights whose origin bits changed, counted
    std::vector<uint8_t> moved_l;    // per light of the scene: its origin changed
    std::vector<rtx_light> lights;   // every light of the edited scene (EditInputs::lights after the edit)
    std::vector<float> cull_T;       // per edited light (first + i), when the image holds them
    bool room_fact = false;          // the edited scene's facts
    float room_M = 0.f;
};
struct MaterialPatch {
    std::vector<EditRange> ranges;
};
// The patch that turns the image of E's scene into the image of the scene with lights [first, first + n)
// (materials, for the second) replaced.  RTX_OK; RTX_E_INVALID for a range beyond the uploaded count;
// RTX_E_UNSUPPORTED for a changed light type or material kind, the first one named in `err`.  E is not
// changed: commit_light_edit makes it the edited scene's once the bytes are on their way.
int pack_light_edit(const EditInputs& E, uint32_t first, uint32_t n, const rtx_light* lights, LightPatch& out,
                    std::string& err);
int pack_material_edit(const EditInputs& E, uint32_t first, uint32_t n, const rtx_material* materials,
                       MaterialPatch& out, std::string& err);
void commit_light_edit(EditInputs& E, LightPatch& patch);
// Apply a patch's ranges to an image in host memory.
void apply_ranges(const std::vector<EditRange>& ranges, char* image);

}  // namespace rtxh
