// rtx_pack.cpp — pack_scene and emit (rtx_pack.h).  Every float computed here that reaches a pixel
// restates the reference in binary32 (same flags as the kernels: -ffp-contract=off).
#include "rtx_pack.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <functional>

using namespace rtxd;

namespace rtxh {
namespace {

inline float4 f4(float x, float y, float z, float w) { return make_float4(x, y, z, w); }
inline float bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
inline float bitsi(int32_t i) { float f; std::memcpy(&f, &i, 4); return f; }
inline int32_t bitsi_f(float f) { int32_t i; std::memcpy(&i, &f, 4); return i; }
inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }
inline int refuse(std::string& err, const char* msg) { err = msg; return RTX_E_INVALID; }
// link and triangle count of device node slot `sl`
inline uint32_t ubits(const float& f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
inline uint32_t node_link(const std::vector<float4>& nodes, size_t sl) { return ubits(nodes[2 * sl + 1].z); }
inline uint32_t node_ntri(const std::vector<float4>& nodes, size_t sl) { return ubits(nodes[2 * sl + 1].w); }

// binary32 values as integers in the floats' own order (-inf .. +inf, -0 below +0), and back
inline uint32_t fkey(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
inline float fkey_inv(uint32_t k) { return bits((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// the room's planes (kSpecRoomPlanes): normal +-1 on axis kRoomAxes[k], zero elsewhere,
// origins finite within 2^64
bool room_planes(const rtx_scene* s) {
    bool room = s->n_planes == 5;
    for (uint32_t i = 0; room && i < 5; ++i) {
        const rtx_plane& p = s->planes[i];
        for (int a = 0; a < 3; ++a) {
            const float n = p.normal[a], o = p.origin[a];
            room = room && (a == kRoomAxes[i] ? (n == 1.f || n == -1.f) : n == 0.f) && std::isfinite(o) &&
                   std::fabs(o) <= 0x1p64f;
        }
    }
    return room;
}

// plane k's origin and normal on its axis kRoomAxes[k] (zeros when the planes are not the room's)
void room_axes(const rtx_scene* s, bool room, float* p0, float* nrm) {
    for (int k = 0; k < 5; ++k) {
        p0[k] = room ? s->planes[k].origin[kRoomAxes[k]] : 0.f;
        nrm[k] = room ? s->planes[k].normal[kRoomAxes[k]] : 0.f;
    }
}

// The room skip's host fact (render_tile's room_clear).  The five planes bound a convex
// room; when every light lies strictly inside it, a shadow ray that starts strictly inside cannot meet
// a room plane before its light.  The kernel may skip the reference's plane tests only where the
// reference's own binary32 test provably fails, which render_tile's comment derives for a shadow
// origin o with, for every plane k (axis A, normal component s = +-1, a_k = RN(p0_A - o_A)):
//     s * a_k < 0   and   |a_k| <= M,   M = RD(2^20 * min margin),
// the margin of light L at plane k being m_k(L) = s * (L_A - p0_A) (in double: the sign is exact, the
// value within 2^-53, far inside the proof's slack), provided also max margin <= 2^100 * min margin
// (the proof's bound on a denormal direction component).
// Both conditions are monotone in o_A (RN(x - p0) is non-decreasing in x), so per axis they hold on an
// interval of floats, whose open ends lo_A < o_A < hi_A are found here by bisection over the floats'
// order, evaluating the very predicate: 6 compares per lane in the kernel instead of 5 differences,
// 5 sign tests and 5 magnitude tests, and a NaN or infinite origin fails them.  When the fact does
// not hold (or RTX_ROOM_SKIP=0) the interval is empty (lo = +inf, hi = -inf) and M = 0.
struct RoomSkip {
    bool fact = false;
    float M = 0.f;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
};
// (the planes as EditInputs keeps them: plane k's origin p0[k] and normal nrm[k] on axis kRoomAxes[k])
RoomSkip room_skip(const float* p0s, const float* nrm, const rtx_light* lights, uint32_t n_lights, bool room, bool off) {
    RoomSkip r;
    if (!room || off || n_lights == 0) return r;
    double mmin = INFINITY, mmax = 0.0;
    for (uint32_t i = 0; i < n_lights; ++i) {
        if (lights[i].type != RTX_LIGHT_POINT) return r;
        for (int k = 0; k < 5; ++k) {
            const int A = kRoomAxes[k];
            const double m = static_cast<double>(nrm[k]) *
                             (static_cast<double>(lights[i].origin[A]) - static_cast<double>(p0s[k]));
            if (!(std::isfinite(m) && m > 0.0)) return r;
            mmin = std::fmin(mmin, m);
            mmax = std::fmax(mmax, m);
        }
    }
    if (!(mmax <= 0x1p100 * mmin)) return r;
    const double Md = std::fmin(0x1p20 * mmin, static_cast<double>(FLT_MAX));
    float M = static_cast<float>(Md);
    if (static_cast<double>(M) > Md) M = std::nextafter(M, 0.f);   // rounded down
    if (!(M > 0.f)) return r;
    float lo[3] = {-INFINITY, -INFINITY, -INFINITY}, hi[3] = {INFINITY, INFINITY, INFINITY};
    for (int k = 0; k < 5; ++k) {
        const int A = kRoomAxes[k];
        const float p0 = p0s[k];
        const bool up = nrm[k] == 1.f;   // inside: o > p0 (else o < p0)
        // |a_k| <= M as the kernel's binary32 difference would have it
        auto near = [&](float o) {
            const volatile float a = up ? o - p0 : p0 - o;
            return a <= M;
        };
        // the float farthest from p0 on the inside that is still `near` (p0 itself is)
        uint32_t in = fkey(p0), out = fkey(up ? INFINITY : -INFINITY);
        while ((up ? out - in : in - out) > 1u) {
            const uint32_t mid = up ? in + (out - in) / 2u : out + (in - out) / 2u;
            (near(fkey_inv(mid)) ? in : out) = mid;
        }
        const float far = fkey_inv(out);   // the first float beyond it: an open end
        if (up) {
            lo[A] = std::fmax(lo[A], p0);
            hi[A] = std::fmin(hi[A], far);
        } else {
            hi[A] = std::fmin(hi[A], p0);
            lo[A] = std::fmax(lo[A], far);
        }
    }
    r.fact = true;
    r.M = M;
    for (int a = 0; a < 3; ++a) { r.lo[a] = lo[a]; r.hi[a] = hi[a]; }
    return r;
}

// What the steps of one pack_scene share besides the PackedScene.
struct Work {
    bool cull_want = false;     // the cull's inputs are being collected
    bool reuse_worth = false;   // ... without the worth estimate's (the cached verdict serves)
    bool split_ok = false;
    bool room = false;
    RoomSkip rs;
    std::vector<std::pair<uint32_t, uint32_t>> mesh_slots;   // node slots [first, end) of each mesh's tree
    std::vector<uint2> slot_rng;   // per device node slot: its triangles (slot_ranges)
    bool ordered_all = true;
    std::vector<float> tbox;       // per triangle (lo, hi) per axis: the cull's worth estimate
    double max_ee2_lo = 0.0;
    int max_depth = 0;             // deepest BVH node over the meshes (stack variant)
};

int check_counts(const rtx_scene* s, std::string& err) {
    if ((s->n_spheres && !s->spheres) || (s->n_planes && !s->planes) || (s->n_meshes && !s->meshes) ||
        (s->n_lights && !s->lights) || (s->n_materials && !s->materials))
        return refuse(err, "null array with non-zero count");
    if (s->n_materials == 0 || s->n_materials > 256) return refuse(err, "need 1..256 materials");
    return RTX_OK;
}

// Reserves, and what the cull decision starts from: the worth estimate's per-triangle boxes are
// collected only when no cached verdict serves.
void begin(const rtx_scene* s, const PackOptions& opt, PackedScene& P, Work& W) {
    size_t nt = 0, nn = 0;
    for (uint32_t mi = 0; mi < s->n_meshes; ++mi) { nt += s->meshes[mi].n_indices / 3; nn += s->meshes[mi].n_nodes; }
    P.tri.reserve(4 * nt);
    P.nodes.reserve(2 * nn + 4 * s->n_meshes + 4);
    P.mesh_layout.assign(s->n_meshes, PackedScene::MeshLayout{});
    W.split_ok = s->n_lights <= static_cast<uint32_t>(kMaxSplitLights);
    W.cull_want = opt.want_cull;
    for (int a = 0; a < 3; ++a) { P.bmin[a] = INFINITY; P.bmax[a] = -INFINITY; }   // mesh vertices
    if (W.cull_want) {
        // (not the node count: an animated loop's host rebuilds its trees, whose sizes vary)
        P.worth_sig = std::to_string(s->n_spheres) + "/" + std::to_string(s->n_planes) + "/" + std::to_string(s->n_meshes) +
                      "/" + std::to_string(nt) + "/" + std::to_string(s->n_lights);
        W.reuse_worth = opt.worth_reuse && opt.worth_sig == P.worth_sig;
        if (!W.reuse_worth) W.tbox.reserve(6 * nt);
    }
}

int pack_prims(const rtx_scene* s, const PackOptions& opt, PackedScene& P, Work& W, std::string& err) {
    const uint32_t nm = s->n_materials;
    for (uint32_t i = 0; i < s->n_spheres; ++i) {
        const rtx_sphere& p = s->spheres[i];
        if (p.material >= nm) return refuse(err, "sphere material out of range");
        P.sph.push_back(f4(p.origin[0], p.origin[1], p.origin[2], p.radius * p.radius));   // Square(radius)
        P.sph_mat.push_back(p.material);
    }
    for (uint32_t i = 0; i < s->n_planes; ++i) {
        const rtx_plane& p = s->planes[i];
        if (p.material >= nm) return refuse(err, "plane material out of range");
        P.pl.push_back(f4(p.origin[0], p.origin[1], p.origin[2], bits(p.material)));
        P.pl.push_back(f4(p.normal[0], p.normal[1], p.normal[2], 0.f));
    }
    // the room skip's record behind the room's five planes (inside the section's padding, so no
    // offset moves): {lo, M}, {hi, 0}
    W.room = room_planes(s);
    float p0[5] = {}, nrm[5] = {};
    room_axes(s, W.room, p0, nrm);
    W.rs = room_skip(p0, nrm, s->lights, s->n_lights, W.room, opt.room_skip_off);
    if (W.room) {
        P.pl.push_back(f4(W.rs.lo[0], W.rs.lo[1], W.rs.lo[2], W.rs.M));
        P.pl.push_back(f4(W.rs.hi[0], W.rs.hi[1], W.rs.hi[2], 0.f));
    }
    return RTX_OK;
}

// One mesh's triangle records, the meshes' box and max_ee.
int pack_tris(const rtx_mesh& m, uint32_t ntri, PackedScene& P, Work& W, std::string& err) {
    std::vector<float4>& tri = P.tri;
    double max_ee = P.max_ee, max_ee2_lo = W.max_ee2_lo;   // (locals: the loop's stores cannot alias them)
    double max_se = P.max_se;
    double bmin[3] = {P.bmin[0], P.bmin[1], P.bmin[2]}, bmax[3] = {P.bmax[0], P.bmax[1], P.bmax[2]};
    const bool boxes = W.cull_want && !W.reuse_worth;
    for (uint32_t k = 0; k < ntri; ++k) {
        const int32_t i0 = m.indices[3 * k], i1 = m.indices[3 * k + 1], i2 = m.indices[3 * k + 2];
        if (i0 < 0 || i1 < 0 || i2 < 0 || static_cast<uint32_t>(i0) >= m.n_positions ||
            static_cast<uint32_t>(i1) >= m.n_positions || static_cast<uint32_t>(i2) >= m.n_positions)
            return refuse(err, "mesh index out of range");
        const float* v0 = m.positions + 3 * i0;
        const float* v1 = m.positions + 3 * i1;
        const float* v2 = m.positions + 3 * i2;
        const float* n = m.normals + 3 * k;
        // edge1 = v1 - v0, edge2 = v2 - v0 (Utils.h:139-140), same binary32 ops as on device
        const float4 e1 = f4(v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2], n[1]);
        const float4 e2 = f4(v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2], n[2]);
        tri.push_back(f4(v0[0], v0[1], v0[2], n[0]));
        tri.push_back(e1);
        tri.push_back(e2);
        // |e1| |e2| (two square roots) only for a triangle that can raise the maximum: below
        // max_ee^2 (1 - 2^-40) the product of the roots cannot reach max_ee (their rounding is
        // ~2^-51); NaN always takes the exact path
        const double a2 = double(e1.x) * e1.x + double(e1.y) * e1.y + double(e1.z) * e1.z;
        const double b2 = double(e2.x) * e2.x + double(e2.y) * e2.y + double(e2.z) * e2.z;
        if (!(a2 * b2 < max_ee2_lo)) {
            const double ee = std::sqrt(a2) * std::sqrt(b2);
            max_ee = (ee > max_ee || ee != ee) ? ee : max_ee;   // NaN sticks
            max_ee2_lo = max_ee * max_ee * (1.0 - 0x1p-40);
        }
        // (|v0|_1 + 2^40) (|e1|_1 + |e2|_1) bounds every product of the cross products (o - v0) x e1
        // and d x e2 for |o_k| <= 2^40, |d_k| <= 1; sums, not maxima: a NaN or inf coordinate sticks
        const double se = (std::fabs(double(v0[0])) + std::fabs(double(v0[1])) + std::fabs(double(v0[2])) + 0x1p40) *
                          (std::fabs(double(e1.x)) + std::fabs(double(e1.y)) + std::fabs(double(e1.z)) +
                           std::fabs(double(e2.x)) + std::fabs(double(e2.y)) + std::fabs(double(e2.z)));
        max_se = (se > max_se || se != se) ? se : max_se;
        tri.push_back(f4(bits(m.material), 0.f, 0.f, 0.f));
        for (int a = 0; a < 3; ++a) {
            const float lo = std::fmin(v0[a], std::fmin(v1[a], v2[a])), hi = std::fmax(v0[a], std::fmax(v1[a], v2[a]));
            bmin[a] = std::fmin(bmin[a], lo);
            bmax[a] = std::fmax(bmax[a], hi);
            if (boxes) { W.tbox.push_back(lo); W.tbox.push_back(hi); }
        }
    }
    P.max_ee = max_ee;
    P.max_se = max_se;
    W.max_ee2_lo = max_ee2_lo;
    for (int a = 0; a < 3; ++a) { P.bmin[a] = bmin[a]; P.bmax[a] = bmax[a]; }
    return RTX_OK;
}

// Re-lay one mesh's tree out for the device: the root at an odd slot, every child pair
// (left, left + 1) at an even slot so one 64-B scalar load fetches both boxes.
// Only the numbering changes; the tree and the left-then-right order do not.  The same
// walk validates the tree (child indices, cycles) and finds its depth: the deepest DFS
// stack a wave can need (pending right siblings on a path).
int relayout(const rtx_mesh& m, uint32_t tri0, std::vector<float4>& nodes, uint32_t& root, int& depth, std::string& err) {
    if ((nodes.size() / 2) % 2 == 0) { nodes.push_back(f4(0, 0, 0, 0)); nodes.push_back(f4(0, 0, 0, 0)); }
    root = static_cast<uint32_t>(nodes.size() / 2);
    struct Item { uint32_t src, dst; int depth; };   // (mesh-local node, device slot, depth)
    std::vector<Item> work;
    work.reserve(64);
    work.push_back({0u, root, 0});
    nodes.resize(nodes.size() + 2);
    depth = 0;
    size_t visited = 0;
    while (!work.empty()) {
        const Item w = work.back();
        work.pop_back();
        const uint32_t src = w.src, dst = w.dst;
        if (++visited > 4ull * m.n_nodes + 4) return refuse(err, "BVH has a cycle");
        depth = w.depth > depth ? w.depth : depth;
        const rtx_bvh_node& nd = m.nodes[src];
        uint32_t link, cnt;
        if (nd.idx_count == 0 && (nd.left_node + 1 >= m.n_nodes || nd.left_node == 0))
            return refuse(err, "BVH child index out of range");
        if (nd.idx_count > 0) {
            if (nd.first_idx % 3 || nd.idx_count % 3 || nd.first_idx + nd.idx_count > m.n_indices)
                return refuse(err, "BVH leaf range invalid");
            link = tri0 + nd.first_idx / 3;
            cnt = nd.idx_count / 3;
        } else {
            link = static_cast<uint32_t>(nodes.size() / 2);   // even: sizes stay even after the root
            cnt = 0;
            nodes.resize(nodes.size() + 4);
            work.push_back({nd.left_node + 1, link + 1, w.depth + 1});
            work.push_back({nd.left_node, link, w.depth + 1});
        }
        // device layout: {min.x, max.x, min.y, max.y}, {min.z, max.z, link, ntri} (slab_mask)
        nodes[2 * dst] = f4(nd.min[0], nd.max[0], nd.min[1], nd.max[1]);
        nodes[2 * dst + 1] = f4(nd.min[2], nd.max[2], bits(link), bits(cnt));
    }
    return RTX_OK;
}

// Per device node slot of one mesh's re-laid-out tree, slots [r0, r1): the range of device
// triangles under it (children's slots follow their parent's, so one backward sweep).  `contig`:
// every subtree's leaves hold consecutive triangles in left-then-right order (build_parts'
// condition); `ordered`: every left child's range ends at or before its sibling's starts (the
// ordered walk's, DevScene::cull).  One sweep serves both (an animated loop uploads every frame).
void slot_ranges(const std::vector<float4>& nodes, uint32_t r0, uint32_t r1, std::vector<uint2>& rng, bool& contig,
                 bool& ordered) {
    if (rng.size() < r1) rng.resize(r1, make_uint2(0u, 0u));
    contig = ordered = true;
    for (uint32_t sl = r1; sl-- > r0;) {
        const uint32_t link = node_link(nodes, sl), cnt = node_ntri(nodes, sl);
        if (cnt) {
            rng[sl] = make_uint2(link, link + cnt);
        } else {
            const uint2 l = rng[link], r = rng[link + 1];
            contig = contig && l.y == r.x;
            ordered = ordered && l.y <= r.x;
            rng[sl] = make_uint2(std::min(l.x, r.x), std::max(l.y, r.y));
        }
    }
}

// Frontier of one re-laid-out mesh BVH for split rendering: start from the root and split
// the part with the most triangles until kPartsPerMesh parts (or only leaves) remain; then, as an
// experiment, the parts listed in `refine` once more.
// Returns false when the tree's left-then-right DFS does not visit the triangles in
// increasing index order (`contig`, slot_ranges) — the property that makes the min-key merge of
// the parts equal to the reference's first-found closest hit — so the scene is rendered unsplit.
bool build_parts(const std::vector<float4>& nodes, uint32_t root, uint32_t mesh, uint32_t target,
                 const std::vector<uint2>& rng, bool contig, std::vector<int> refine, std::vector<int4>& parts) {
    if (!contig) return false;
    auto sub = [&](uint32_t n) { return rng[n].y - rng[n].x; };   // triangles under slot n
    struct Part { uint32_t node, path, depth; };
    std::vector<Part> fr{{root, 0u, 0u}};
    auto split = [&](size_t k) {   // entry k becomes its left child, its right child follows it
        const Part e = fr[k];
        const uint32_t l = node_link(nodes, e.node);
        fr[k] = {l, e.path, e.depth + 1};
        fr.insert(fr.begin() + static_cast<std::ptrdiff_t>(k) + 1, Part{l + 1, e.path | (1u << e.depth), e.depth + 1});
    };
    while (fr.size() < target) {
        int best = -1;
        for (size_t k = 0; k < fr.size(); ++k)
            if (!node_ntri(nodes, fr[k].node) && fr[k].depth < 31 && (best < 0 || sub(fr[k].node) > sub(fr[best].node)))
                best = static_cast<int>(k);
        if (best < 0) break;
        split(static_cast<size_t>(best));
    }
    std::sort(refine.begin(), refine.end(), std::greater<int>());
    for (int k : refine) {
        if (k < 0 || k >= static_cast<int>(fr.size())) continue;
        if (node_ntri(nodes, fr[k].node) || fr[k].depth >= 31) continue;
        split(static_cast<size_t>(k));
    }
    for (const Part& e : fr)
        parts.push_back(make_int4(static_cast<int>(mesh), static_cast<int>(e.node), static_cast<int>(e.path),
                                  static_cast<int>(e.depth)));
    return true;
}

// One mesh: its checks, triangles, tree, record and frontier entries.
int pack_mesh(const rtx_scene* s, uint32_t mi, const PackOptions& opt, PackedScene& P, Work& W, std::string& err) {
    const rtx_mesh& m = s->meshes[mi];
    std::vector<float4>& nodes = P.nodes;
    PackedScene::MeshLayout& L = P.mesh_layout[mi];
    const bool reserve = mi < opt.reserve.size() && opt.reserve[mi];
    if (m.material >= s->n_materials) return refuse(err, "mesh material out of range");
    if (m.cull_mode < RTX_CULL_FRONT || m.cull_mode > RTX_CULL_NONE) return refuse(err, "bad cull mode");
    if (m.n_indices % 3) return refuse(err, "mesh index count not a multiple of 3");
    const uint32_t tri0 = static_cast<uint32_t>(P.tri.size() / 4), ntri = m.n_indices / 3;
    if (ntri && (!m.positions || !m.indices || !m.normals)) return refuse(err, "mesh arrays missing");
    if (const int rc = pack_tris(m, ntri, P, W, err); rc != RTX_OK) return rc;
    uint32_t root = 0;
    bool contig_m = true, ordered_m = true;
    if (m.n_nodes) {
        if (!m.nodes) return refuse(err, "mesh nodes missing");
        if (const int rc = relayout(m, tri0, nodes, root, L.depth, err); rc != RTX_OK) return rc;
        W.max_depth = std::max(W.max_depth, L.depth);
        W.mesh_slots.push_back({root, static_cast<uint32_t>(nodes.size() / 2)});
        slot_ranges(nodes, root, static_cast<uint32_t>(nodes.size() / 2), W.slot_rng, contig_m, ordered_m);
        W.ordered_all = W.ordered_all && ordered_m;
        if (reserve) {   // slots root .. root + 2T - 1 belong to this mesh
            const size_t want = 2 * (static_cast<size_t>(root) + 2 * static_cast<size_t>(ntri));
            if (nodes.size() < want) nodes.resize(want + (want / 2) % 2 * 2, f4(0, 0, 0, 0));
        }
    }
    L.tri0 = tri0;
    L.root = root;
    const float cs = m.cull_mode == RTX_CULL_FRONT ? -1.f : (m.cull_mode == RTX_CULL_BACK ? 1.f : 0.f);
    // {root node byte offset, node count, cull sign bits, material}
    P.meshes.push_back(make_int4(static_cast<int>(root * 32u), static_cast<int>(m.n_nodes), bitsi_f(cs), m.material));
    // ~48 triangles per part at least: finer parts of a small mesh cost more than they spread
    const uint32_t target = std::max(2u, std::min(opt.split_parts, ntri / 48u));
    const size_t p0 = P.parts.size();
    if (m.n_nodes && !build_parts(nodes, root, mi, target, W.slot_rng, contig_m, opt.part_refine, P.parts)) W.split_ok = false;
    if (reserve) {   // exactly `target` entries, the unused ones {-1, ...}
        P.parts.resize(p0 + target, make_int4(-1, 0, 0, 0));
        L.part0 = static_cast<uint32_t>(p0);
        L.part_cap = target;
    }
    return RTX_OK;
}

// The frontier's size in the image: static uploads reserve kMaxParts entries for the frontier
// refinement (refine_round); meshes with device-rebuild reserves keep theirs exactly.
void size_frontier(const PackOptions& opt, PackedScene& P, Work& W) {
    if (P.parts.size() > static_cast<size_t>(kMaxParts)) W.split_ok = false;
    if (!W.split_ok) P.parts.clear();
    bool any_reserve = false;
    for (uint8_t r : opt.reserve) any_reserve = any_reserve || r != 0;
    P.n_parts = static_cast<uint32_t>(P.parts.size());
    P.refinable = W.split_ok && P.n_parts > 0 && !any_reserve;
    if (P.refinable) P.parts.resize(kMaxParts, make_int4(-1, 0, 0, 0));
}

// Is the cull worth it?  The surface areas of the reference's boxes over those of the tight boxes,
// summed over the nodes (the SAH estimate of how many more slab tests the reference's
// boxes pass): below cull_min_sa the records cost more than they save (measured: W4_Bunny
// 1.19, -11 %; W4_Optional 2.40, +48 %; Synthetic100k 9.26, +182 %; profiles/r04).
bool cull_worth(const PackedScene& P, const Work& W, double cull_min_sa) {
    const std::vector<float4>& nodes = P.nodes;
    const std::vector<float>& tbox = W.tbox;
    std::vector<float> nb(6 * (nodes.size() / 2));
    double sa_ref = 0.0, sa_tight = 0.0;
    auto sa = [](double x, double y, double z) { return 2.0 * (x * y + y * z + z * x); };
    for (const auto& [r0, r1] : W.mesh_slots)
        for (uint32_t sl = r1; sl-- > r0;) {
            const uint32_t link = node_link(nodes, sl), cnt = node_ntri(nodes, sl);
            float* b = &nb[6 * sl];
            if (cnt) {
                for (int a = 0; a < 3; ++a) { b[2 * a] = INFINITY; b[2 * a + 1] = -INFINITY; }
                for (uint32_t t = link; t < link + cnt && t < tbox.size() / 6; ++t)
                    for (int a = 0; a < 3; ++a) {
                        b[2 * a] = std::fmin(b[2 * a], tbox[6 * t + 2 * a]);
                        b[2 * a + 1] = std::fmax(b[2 * a + 1], tbox[6 * t + 2 * a + 1]);
                    }
            } else {
                for (int a = 0; a < 3; ++a) {
                    b[2 * a] = std::fmin(nb[6 * link + 2 * a], nb[6 * (link + 1) + 2 * a]);
                    b[2 * a + 1] = std::fmax(nb[6 * link + 2 * a + 1], nb[6 * (link + 1) + 2 * a + 1]);
                }
            }
            const float4 r0v = nodes[2 * sl], r1v = nodes[2 * sl + 1];
            sa_ref += sa(double(r0v.y) - r0v.x, double(r0v.w) - r0v.z, double(r1v.y) - r1v.x);
            sa_tight += sa(std::fmax(double(b[1]) - b[0], 0.0), std::fmax(double(b[3]) - b[2], 0.0),
                           std::fmax(double(b[5]) - b[4], 0.0));
        }
    return sa_ref >= cull_min_sa * sa_tight;   // false for NaN
}

// Per light the tmax up to which its shadow rays are culled: 4x the farthest mesh-box corner + 1
// (longer rays pass).
float cull_tmax(const float* origin, const double* bmin, const double* bmax) {
    double R = 0.0;
    for (int k = 0; k < 8; ++k) {
        const double cx = (k & 1) ? bmax[0] : bmin[0], cy = (k & 2) ? bmax[1] : bmin[1], cz = (k & 4) ? bmax[2] : bmin[2];
        const double dx = origin[0] - cx, dy = origin[1] - cy, dz = origin[2] - cz;
        R = std::fmax(R, std::sqrt(dx * dx + dy * dy + dz * dz));
    }
    const double T = 4.0 * R + 1.0;
    return std::isfinite(T) && T < 0x1p60 ? static_cast<float>(T) : 0.f;   // 0: never culled
}

// Cull records' inputs: per node slot the range of device triangles under it (leaf order is
// contiguous within a subtree), the worth verdict (computed, or the cached one) and the lights' tmax.
void cull_inputs(const rtx_scene* s, const PackOptions& opt, PackedScene& P, Work& W) {
    bool on = W.cull_want && !P.tri.empty() && !W.mesh_slots.empty();
    for (int a = 0; a < 3; ++a) on = on && std::isfinite(P.bmin[a]) && std::isfinite(P.bmax[a]);
    if (!on) return;
    P.cull_rng = std::move(W.slot_rng);
    P.cull_rng.resize(P.nodes.size() / 2, make_uint2(0u, 0u));
    P.worth_from = W.reuse_worth ? PackedScene::kWorthReused : PackedScene::kWorthComputed;
    P.worth = W.reuse_worth ? opt.worth : cull_worth(P, W, opt.cull_min_sa);
    P.cull_on = W.ordered_all && P.worth;   // the ordered walk needs left-then-right = increasing index
    for (uint32_t i = 0; i < s->n_lights; ++i) P.cull_T.push_back(cull_tmax(s->lights[i].origin, P.bmin, P.bmax));
}

// Device links are byte offsets (s_load with an SGPR offset, no address arithmetic):
// inner node -> its child pair (2 slots x 32 B), leaf -> its first 64-B triangle.
int links_to_offsets(PackedScene& P, std::string& err) {
    if (P.tri.size() * 16 >= (1ull << 32) || P.nodes.size() * 16 >= (1ull << 32) || P.sph.size() * 16 >= (1ull << 32) ||
        P.pl.size() * 16 >= (1ull << 32))
        return refuse(err, "scene too large for 32-bit record offsets");
    for (size_t sl = 0; sl < P.nodes.size() / 2; ++sl) {
        const uint32_t link = node_link(P.nodes, sl);
        P.nodes[2 * sl + 1].z = bits(node_ntri(P.nodes, sl) ? link * 64u : link * 32u);
    }
    return RTX_OK;
}

// Octant copies of the node array (DevScene::oct_bytes, slab_mask<kSlabOct>): possible
// when every box is ordered lo <= hi per axis (no NaN).  The reference's quirky bounds
// (max initialised with FLT_MIN) stay ordered; an empty box would not.
// Large trees keep one copy: 8 copies of a multi-MB node array crowd the L2 (Synthetic100k,
// ~2 MB per copy, is 2.5 % faster without them; W4_Optional, 117 KB, 2.5 % faster with).
void octant_decision(PackedScene& P) {
    const std::vector<float4>& nodes = P.nodes;
    P.node_bytes = align256(nodes.size() * 16);
    bool ok = !nodes.empty() && P.node_bytes <= kOctantMaxNodeBytes && 8 * P.node_bytes < (1ull << 32);
    for (size_t n = 0; ok && n < nodes.size(); n += 2)
        ok = nodes[n].x <= nodes[n].y && nodes[n].z <= nodes[n].w && nodes[n + 1].x <= nodes[n + 1].y;
    P.oct_ok = ok;
}

// The two record encoders (an upload's and an edit's): a light's 2 records, a material's 3.
void light_records(const rtx_light& l, float4* out) {
    out[0] = f4(l.origin[0], l.origin[1], l.origin[2], bitsi(l.type));
    out[1] = f4(l.color[0], l.color[1], l.color[2], l.intensity);
}
void material_records(const rtx_material& m, float4* out) {
    // BRDF::Lambert(kd, cd) = (cd * kd) / PI (BRDFs.h:14-17), exact binary32 on host
    const float lr = (m.color[0] * m.kd) / RTX_PI, lg = (m.color[1] * m.kd) / RTX_PI, lb = (m.color[2] * m.kd) / RTX_PI;
    out[0] = f4(bitsi(m.kind), m.color[0], m.color[1], m.color[2]);
    out[1] = f4(m.kd, m.ks, m.exponent, m.metalness);
    out[2] = f4(m.roughness, lr, lg, lb);
}

void pack_lights_materials(const rtx_scene* s, PackedScene& P) {
    float4 r[3];
    for (uint32_t i = 0; i < s->n_lights; ++i) {
        light_records(s->lights[i], r);
        P.lights.insert(P.lights.end(), r, r + 2);
    }
    for (uint32_t i = 0; i < s->n_materials; ++i) {
        material_records(s->materials[i], r);
        P.mats.insert(P.mats.end(), r, r + 3);
    }
}

// The section table (every section 256-B aligned, an empty one 256 B), DevScene's counts, and the
// cull's sizes: one copy of the node slots per anchor, cull_stride apart.
void layout(const rtx_scene* s, const PackOptions& opt, PackedScene& P) {
    // the node section: 8 octant copies (node_bytes apart, written straight into the image by
    // emit) or the one array
    const size_t n[kSecCount] = {P.sph.size() * 16,    P.sph_mat.size() * 4, P.pl.size() * 16,
                                 P.tri.size() * 16,    P.oct_ok ? 8 * P.node_bytes : P.nodes.size() * 16,
                                 P.meshes.size() * 16, P.lights.size() * 16, P.mats.size() * 16,
                                 P.parts.size() * 16,  P.cull_rng.size() * 8, P.cull_T.size() * 4};
    P.total = 0;
    for (int i = 0; i < kSecCount; ++i) {
        P.sec[i] = {n[i], P.total};
        P.total += align256(n[i] ? n[i] : 16);
    }
    P.n_spheres = s->n_spheres; P.n_planes = s->n_planes; P.n_meshes = s->n_meshes;
    P.n_lights = s->n_lights; P.n_materials = s->n_materials;
    P.n_tris = static_cast<uint32_t>(P.tri.size() / 4); P.n_nodes = static_cast<uint32_t>(P.nodes.size() / 2);
    P.tri_fast = (P.max_ee <= 0x1p56 && P.max_se <= 0x1p126) ? 1u : 0u;
    P.oct_bytes = (P.oct_ok && !opt.no_octant) ? static_cast<uint32_t>(P.node_bytes) : 0u;
    P.cull_stride = P.node_bytes;
    if (P.cull_on && (P.cull_stride >= (1ull << 32) || 2 * P.tri.size() >= (1ull << 32))) P.cull_on = false;
    P.cull_n = kCullTreeWG;
    while (P.cull_on && P.cull_n < P.n_tris) P.cull_n *= 2u;
}

// A BVH kStackDepth or more levels deep renders with the deep-stack variant, unsplit;
// kStackDepthDeep or more with its stacks in HBM.  The uniform facts for the specialised kernels
// (kSpec*): the material kinds the geometry references, every light a point light, the sphere /
// plane / mesh counts.
void scene_facts(const rtx_scene* s, PackedScene& P, const Work& W) {
    SceneFacts& f = P.facts;
    f.deep_stack = W.max_depth >= kStackDepth;
    f.hbm_stack = W.max_depth >= kStackDepthDeep;
    f.max_depth = static_cast<uint32_t>(W.max_depth);
    int kinds = 0;
    bool point = true;
    auto kind = [&](uint32_t m) {
        const int k = s->materials[m].kind;
        kinds |= (k >= RTX_MAT_SOLID_COLOR && k <= RTX_MAT_COOK_TORRANCE) ? (1 << k) : kSpecKindAll;
    };
    for (uint32_t i = 0; i < s->n_spheres; ++i) kind(s->spheres[i].material);
    for (uint32_t i = 0; i < s->n_planes; ++i) kind(s->planes[i].material);
    for (uint32_t i = 0; i < s->n_meshes; ++i) kind(s->meshes[i].material);
    for (uint32_t i = 0; i < s->n_lights; ++i) point = point && s->lights[i].type == RTX_LIGHT_POINT;
    bool cull_back = true;   // kSpecCullBack: every mesh culls back faces
    for (uint32_t i = 0; i < s->n_meshes; ++i) cull_back = cull_back && s->meshes[i].cull_mode == RTX_CULL_BACK;
    // the room's planes (kSpecRoomPlanes, room_planes above) and the room skip's fact
    for (uint32_t i = 0; W.room && i < 5; ++i) f.room_p0[i] = s->planes[i].origin[kRoomAxes[i]];
    f.room_fact = W.rs.fact;
    f.room_M = W.rs.M;
    f.spec = kinds | (point ? kSpecPoint : 0) | (s->n_spheres == 0 ? kSpecNoSpheres : 0) |
             (s->n_planes == 5 ? kSpecFivePlanes : 0) | (s->n_meshes == 1 ? kSpecOneMesh : 0) |
             (s->n_meshes == 0 ? kSpecNoMesh : 0) | (W.room ? kSpecRoomPlanes : 0) | (cull_back ? kSpecCullBack : 0);
    f.split_ok = W.split_ok && !P.parts.empty() && !f.deep_stack;
    f.sig = std::to_string(P.n_spheres) + "/" + std::to_string(P.n_planes) + "/" + std::to_string(P.n_meshes) + "/" +
            std::to_string(P.n_tris) + "/" + std::to_string(P.n_lights) + "/" + std::to_string(P.n_materials);
}

}  // namespace

int pack_scene(const rtx_scene* s, const PackOptions& opt, PackedScene& P, std::string& err) {
    P = PackedScene{};
    Work W;
    if (const int rc = check_counts(s, err); rc != RTX_OK) return rc;
    begin(s, opt, P, W);
    if (const int rc = pack_prims(s, opt, P, W, err); rc != RTX_OK) return rc;
    for (uint32_t mi = 0; mi < s->n_meshes; ++mi)
        if (const int rc = pack_mesh(s, mi, opt, P, W, err); rc != RTX_OK) return rc;
    size_frontier(opt, P, W);
    cull_inputs(s, opt, P, W);
    if (const int rc = links_to_offsets(P, err); rc != RTX_OK) return rc;
    octant_decision(P);
    pack_lights_materials(s, P);
    layout(s, opt, P);
    scene_facts(s, P, W);
    return RTX_OK;
}

void emit(const PackedScene& P, char* dst, int host_octant_copies) {
    const void* const src[kSecCount] = {P.sph.data(),    P.sph_mat.data(), P.pl.data(),   P.tri.data(),
                                        P.nodes.data(),  P.meshes.data(),  P.lights.data(), P.mats.data(),
                                        P.parts.data(),  P.cull_rng.data(), P.cull_T.data()};
    const std::vector<float4>& nodes = P.nodes;
    for (int i = 0; i < kSecCount; ++i) {
        const PackedScene::Sec& x = P.sec[i];
        const size_t end = i + 1 < kSecCount ? P.sec[i + 1].off : P.total;
        if (i == kSecNodes && x.n && P.oct_ok) {   // octant copy k stores (hi, lo) on the axes set in k
            for (int k = 0; k < host_octant_copies; ++k) {
                float4* out = reinterpret_cast<float4*>(dst + x.off + k * P.node_bytes);
                const bool mx = k & 1, my = k & 2, mz = k & 4;
                for (size_t n = 0; n < nodes.size(); n += 2) {
                    const float4 a = nodes[n], b = nodes[n + 1];
                    out[n] = f4(mx ? a.y : a.x, mx ? a.x : a.y, my ? a.w : a.z, my ? a.z : a.w);
                    out[n + 1] = f4(mz ? b.y : b.x, mz ? b.x : b.y, b.z, b.w);
                }
                std::memset(reinterpret_cast<char*>(out + nodes.size()), 0, P.node_bytes - nodes.size() * 16);
            }
        } else if (x.n) {
            std::memcpy(dst + x.off, src[i], x.n);
        }
        std::memset(dst + x.off + x.n, 0, end - x.off - x.n);
    }
}

// ---- in-place edits ---------------------------------------------------------------------------------
void edit_inputs(const rtx_scene* s, const PackOptions& opt, const PackedScene& P, EditInputs& E) {
    // (every field is set: an animated loop's upload per frame reuses the vectors' storage)
    E.room = (P.facts.spec & kSpecRoomPlanes) != 0;
    E.room_skip_off = opt.room_skip_off;
    room_axes(s, E.room, E.room_p0, E.room_n);
    E.has_cull_T = !P.cull_T.empty();
    for (int a = 0; a < 3; ++a) { E.bmin[a] = P.bmin[a]; E.bmax[a] = P.bmax[a]; }
    E.off_planes = P.sec[kSecPlanes].off; E.off_lights = P.sec[kSecLights].off;
    E.off_mats = P.sec[kSecMaterials].off; E.off_cull_T = P.sec[kSecCullT].off;
    E.lights.assign(s->lights, s->lights + s->n_lights);
    E.kinds.resize(s->n_materials);
    for (uint32_t i = 0; i < s->n_materials; ++i) E.kinds[i] = s->materials[i].kind;
    E.facts = P.facts;
}

namespace {
void push_records(EditRange& r, const float4* rec, int n) {
    const size_t at = r.words.size();
    r.words.resize(at + 4 * static_cast<size_t>(n));
    std::memcpy(r.words.data() + at, rec, 16 * static_cast<size_t>(n));
}
}  // namespace

int pack_light_edit(const EditInputs& E, uint32_t first, uint32_t n, const rtx_light* lights, LightPatch& out,
                    std::string& err) {
    out = LightPatch{};
    const size_t count = E.lights.size();
    if ((n && !lights) || first > count || n > count - first) return refuse(err, "light range beyond the uploaded lights");
    for (uint32_t i = 0; i < n; ++i)
        if (lights[i].type != E.lights[first + i].type) {
            err = "light " + std::to_string(first + i) + " changes its type: that is an upload";
            return RTX_E_UNSUPPORTED;
        }
    out.lights = E.lights;
    out.moved_l.assign(count, 0);
    out.room_fact = E.facts.room_fact;
    out.room_M = E.facts.room_M;
    EditRange rec;
    rec.off = E.off_lights + 32 * static_cast<size_t>(first);
    for (uint32_t i = 0; i < n; ++i) {
        rtx_light& l = out.lights[first + i];
        if (std::memcmp(l.origin, lights[i].origin, 12) != 0) { out.moved_l[first + i] = 1; ++out.moved; }
        std::memcpy(l.origin, lights[i].origin, 12);
        std::memcpy(l.color, lights[i].color, 12);
        l.intensity = lights[i].intensity;
        float4 r[2];
        light_records(l, r);
        push_records(rec, r, 2);
    }
    if (n) out.ranges.push_back(std::move(rec));
    if (!out.moved) return RTX_OK;
    // what pack_scene derives from the lights' origins: the room-skip record and facts, the lights' cull_T
    if (E.room) {
        const RoomSkip rs = room_skip(E.room_p0, E.room_n, out.lights.data(), static_cast<uint32_t>(count), true, E.room_skip_off);
        const float4 r[2] = {f4(rs.lo[0], rs.lo[1], rs.lo[2], rs.M), f4(rs.hi[0], rs.hi[1], rs.hi[2], 0.f)};
        EditRange room;
        room.off = E.off_planes + 5 * 32;
        push_records(room, r, 2);
        out.ranges.push_back(std::move(room));
        out.room_fact = rs.fact;
        out.room_M = rs.M;
    }
    if (E.has_cull_T) {
        EditRange t;
        t.off = E.off_cull_T + 4 * static_cast<size_t>(first);
        for (uint32_t i = 0; i < n; ++i) {
            out.cull_T.push_back(cull_tmax(out.lights[first + i].origin, E.bmin, E.bmax));
            t.words.push_back(ubits(out.cull_T.back()));
        }
        out.ranges.push_back(std::move(t));
    }
    return RTX_OK;
}

void commit_light_edit(EditInputs& E, LightPatch& patch) {
    E.lights.swap(patch.lights);
    E.facts.room_fact = patch.room_fact;
    E.facts.room_M = patch.room_M;
}

int pack_material_edit(const EditInputs& E, uint32_t first, uint32_t n, const rtx_material* materials,
                       MaterialPatch& out, std::string& err) {
    out = MaterialPatch{};
    const size_t count = E.kinds.size();
    if ((n && !materials) || first > count || n > count - first)
        return refuse(err, "material range beyond the uploaded materials");
    for (uint32_t i = 0; i < n; ++i)
        if (materials[i].kind != E.kinds[first + i]) {
            err = "material " + std::to_string(first + i) + " changes its kind: that is an upload";
            return RTX_E_UNSUPPORTED;
        }
    EditRange rec;
    rec.off = E.off_mats + 48 * static_cast<size_t>(first);
    for (uint32_t i = 0; i < n; ++i) {
        float4 r[3];
        material_records(materials[i], r);
        push_records(rec, r, 3);
    }
    if (n) out.ranges.push_back(std::move(rec));
    return RTX_OK;
}

void apply_ranges(const std::vector<EditRange>& ranges, char* image) {
    for (const EditRange& r : ranges) std::memcpy(image + r.off, r.words.data(), 4 * r.words.size());
}

}  // namespace rtxh
