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

}  // namespace rtxh
