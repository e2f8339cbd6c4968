// rtx_upload.hip — a host scene packed into the context's next HBM image (rtx_kernels.h's layout):
// the device numbering of the BVHs, the split frontier, the cull records' inputs, the kernel facts.
// Every float computed here that reaches a pixel restates the reference in binary32 (same flags as
// the kernels: -ffp-contract=off).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "rtx_ctx.h"

using namespace rtxh;

namespace {


inline float4 f4(float x, float y, float z, float w) { return make_float4(x, y, z, w); }
inline float bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
inline float bitsi(int32_t i) { float f; std::memcpy(&f, &i, 4); return f; }
inline int32_t bitsi_f(float f) { int32_t i; std::memcpy(&i, &f, 4); return i; }
inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

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
        uint32_t link, cnt;
        std::memcpy(&link, &nodes[2 * sl + 1].z, 4);
        std::memcpy(&cnt, &nodes[2 * sl + 1].w, 4);
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
// the part with the most triangles until kPartsPerMesh parts (or only leaves) remain.
// Returns false when the tree's left-then-right DFS does not visit the triangles in
// increasing index order (`contig`, slot_ranges) — the property that makes the min-key merge of
// the parts equal to the reference's first-found closest hit — so the scene is rendered unsplit.
bool build_parts(const std::vector<float4>& nodes, uint32_t root, uint32_t mesh, uint32_t target,
                 const std::vector<uint2>& rng, bool contig, std::vector<int4>& parts) {
    if (!contig) return false;
    auto link = [&](uint32_t n) { uint32_t u; std::memcpy(&u, &nodes[2 * n + 1].z, 4); return u; };
    auto ntri = [&](uint32_t n) { uint32_t u; std::memcpy(&u, &nodes[2 * n + 1].w, 4); return u; };
    auto sub = [&](uint32_t n) { return rng[n].y - rng[n].x; };   // triangles under slot n
    struct P { uint32_t node, path, depth; };
    std::vector<P> fr{{root, 0u, 0u}};
    while (fr.size() < target) {
        int best = -1;
        for (size_t k = 0; k < fr.size(); ++k)
            if (!ntri(fr[k].node) && fr[k].depth < 31 && (best < 0 || sub(fr[k].node) > sub(fr[best].node)))
                best = static_cast<int>(k);
        if (best < 0) break;
        const P e = fr[best];
        fr[best] = {link(e.node), e.path, e.depth + 1};
        fr.insert(fr.begin() + best + 1, P{link(e.node) + 1, e.path | (1u << e.depth), e.depth + 1});
    }
    if (const char* ev = std::getenv("RTX_PART_REFINE")) {   // experiment: split the listed parts once more
        std::vector<int> idx;
        for (const char* q = ev; *q;) {
            char* end = nullptr;
            const long v = std::strtol(q, &end, 10);
            if (end == q) break;
            idx.push_back(static_cast<int>(v));
            q = *end ? end + 1 : end;
        }
        std::sort(idx.begin(), idx.end(), std::greater<int>());
        for (int k : idx) {
            if (k < 0 || k >= static_cast<int>(fr.size())) continue;
            const P e = fr[k];
            if (ntri(e.node) || e.depth >= 31) continue;
            fr[k] = {link(e.node), e.path, e.depth + 1};
            fr.insert(fr.begin() + k + 1, P{link(e.node) + 1, e.path | (1u << e.depth), e.depth + 1});
        }
    }
    for (const P& e : fr)
        parts.push_back(make_int4(static_cast<int>(mesh), static_cast<int>(e.node), static_cast<int>(e.path),
                                  static_cast<int>(e.depth)));
    return true;
}

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

// binary32 values as integers in the floats' own order (-inf .. +inf, -0 below +0), and back
inline uint32_t fkey(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
inline float fkey_inv(uint32_t k) { return bits((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

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
RoomSkip room_skip(const rtx_scene* s, bool room, bool off) {
    RoomSkip r;
    if (!room || off || s->n_lights == 0) return r;
    double mmin = INFINITY, mmax = 0.0;
    for (uint32_t i = 0; i < s->n_lights; ++i) {
        if (s->lights[i].type != RTX_LIGHT_POINT) return r;
        for (int k = 0; k < 5; ++k) {
            const int A = kRoomAxes[k];
            const double m = static_cast<double>(s->planes[k].normal[A]) *
                             (static_cast<double>(s->lights[i].origin[A]) - static_cast<double>(s->planes[k].origin[A]));
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
        const float p0 = s->planes[k].origin[A];
        const bool up = s->planes[k].normal[A] == 1.f;   // inside: o > p0 (else o < p0)
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

}  // namespace

extern "C" int rtx_upload_scene(rtx_ctx* c, const rtx_scene* s) {
    if (c) {   // the upload pattern the cull decision reads (see rtx_ctx::cull_animated)
        c->short_uploads = (c->has_scene && c->renders_since_upload <= 1) ? c->short_uploads + 1 : 0;
        c->renders_since_upload = 0;
        c->motion.upload_motion = c->short_uploads >= 1;
        if (const int rc = join_split(c); rc != RTX_OK) return rc;   // (the last chain reads the current image)
    }
    return upload_scene(c, s, nullptr);
}

namespace rtxh {
int upload_scene(rtx_ctx* c, const rtx_scene* s, UploadLayout* lay) {
    if (!c || !s) return RTX_E_INVALID;
    if ((s->n_spheres && !s->spheres) || (s->n_planes && !s->planes) || (s->n_meshes && !s->meshes) ||
        (s->n_lights && !s->lights) || (s->n_materials && !s->materials))
        return fail(c, RTX_E_INVALID, "null array with non-zero count");
    if (s->n_materials == 0 || s->n_materials > 256) return fail(c, RTX_E_INVALID, "need 1..256 materials");
    const uint32_t nm = s->n_materials;
    std::vector<float4> sph, pl, tri, nodes, lights, mats;
    std::vector<uint32_t> sph_mat;
    std::vector<int4> meshes, parts;
    {
        size_t nt = 0, nn = 0;
        for (uint32_t mi = 0; mi < s->n_meshes; ++mi) { nt += s->meshes[mi].n_indices / 3; nn += s->meshes[mi].n_nodes; }
        tri.reserve(4 * nt);
        nodes.reserve(2 * nn + 4 * s->n_meshes + 4);
    }
    bool split_ok = s->n_lights <= static_cast<uint32_t>(kMaxSplitLights);
    // exact cull (DevScene::cull): host uploads (a device-animated image is rebuilt in place and
    // carries no records), at most kMaxCullLights lights
    bool cull_on = !lay && !c->no_cull && s->n_lights <= static_cast<uint32_t>(kMaxCullLights) &&
                   (c->short_uploads < 2 || c->cull_animated);
    double bmin[3] = {INFINITY, INFINITY, INFINITY}, bmax[3] = {-INFINITY, -INFINITY, -INFINITY};   // mesh vertices
    std::vector<std::pair<uint32_t, uint32_t>> mesh_slots;   // node slots [first, end) of each mesh's tree
    std::vector<uint2> slot_rng;   // per device node slot: its triangles (slot_ranges)
    bool ordered_all = true;
    std::vector<float> tbox;   // per triangle (lo, hi) per axis: the cull's worth estimate below
    std::string worth_sig;
    bool reuse_worth = false;
    if (cull_on) {
        // (not the node count: an animated loop's host rebuilds its trees, whose sizes vary)
        size_t nt = 0;
        for (uint32_t mi = 0; mi < s->n_meshes; ++mi) nt += s->meshes[mi].n_indices / 3;
        worth_sig = std::to_string(s->n_spheres) + "/" + std::to_string(s->n_planes) + "/" + std::to_string(s->n_meshes) +
                    "/" + std::to_string(nt) + "/" + std::to_string(s->n_lights);
        reuse_worth = c->short_uploads >= 1 && c->cull_worth >= 0 && c->cull_worth_age + 1 < kCullWorthReuse &&
                      c->cull_worth_sig == worth_sig;
        if (!reuse_worth) tbox.reserve(6 * nt);
    }
    double max_ee = 0.0;   // max |e1| * |e2| over the triangles (DevScene::tri_fast)
    double max_ee2_lo = 0.0;
    int max_depth = 0;     // deepest BVH node over the meshes (stack variant)
    for (uint32_t i = 0; i < s->n_spheres; ++i) {
        const rtx_sphere& p = s->spheres[i];
        if (p.material >= nm) return fail(c, RTX_E_INVALID, "sphere material out of range");
        sph.push_back(f4(p.origin[0], p.origin[1], p.origin[2], p.radius * p.radius));   // Square(radius)
        sph_mat.push_back(p.material);
    }
    for (uint32_t i = 0; i < s->n_planes; ++i) {
        const rtx_plane& p = s->planes[i];
        if (p.material >= nm) return fail(c, RTX_E_INVALID, "plane material out of range");
        pl.push_back(f4(p.origin[0], p.origin[1], p.origin[2], bits(p.material)));
        pl.push_back(f4(p.normal[0], p.normal[1], p.normal[2], 0.f));
    }
    // the room skip's record behind the room's five planes (inside the section's padding, so no
    // offset moves): {lo, M}, {hi, 0}
    const bool room = room_planes(s);
    const RoomSkip rs = room_skip(s, room, c->room_skip_off);
    if (room) {
        pl.push_back(f4(rs.lo[0], rs.lo[1], rs.lo[2], rs.M));
        pl.push_back(f4(rs.hi[0], rs.hi[1], rs.hi[2], 0.f));
    }
    for (uint32_t mi = 0; mi < s->n_meshes; ++mi) {
        const rtx_mesh& m = s->meshes[mi];
        if (m.material >= nm) return fail(c, RTX_E_INVALID, "mesh material out of range");
        if (m.cull_mode < RTX_CULL_FRONT || m.cull_mode > RTX_CULL_NONE) return fail(c, RTX_E_INVALID, "bad cull mode");
        if (m.n_indices % 3) return fail(c, RTX_E_INVALID, "mesh index count not a multiple of 3");
        const uint32_t tri0 = static_cast<uint32_t>(tri.size() / 4), node0 = static_cast<uint32_t>(nodes.size() / 2);
        const uint32_t ntri = m.n_indices / 3;
        if (ntri && (!m.positions || !m.indices || !m.normals)) return fail(c, RTX_E_INVALID, "mesh arrays missing");
        for (uint32_t k = 0; k < ntri; ++k) {
            const int32_t i0 = m.indices[3 * k], i1 = m.indices[3 * k + 1], i2 = m.indices[3 * k + 2];
            if (i0 < 0 || i1 < 0 || i2 < 0 || static_cast<uint32_t>(i0) >= m.n_positions ||
                static_cast<uint32_t>(i1) >= m.n_positions || static_cast<uint32_t>(i2) >= m.n_positions)
                return fail(c, RTX_E_INVALID, "mesh index out of range");
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
            tri.push_back(f4(bits(m.material), 0.f, 0.f, 0.f));
            for (int a = 0; a < 3; ++a) {
                const float lo = std::fmin(v0[a], std::fmin(v1[a], v2[a])), hi = std::fmax(v0[a], std::fmax(v1[a], v2[a]));
                bmin[a] = std::fmin(bmin[a], lo);
                bmax[a] = std::fmax(bmax[a], hi);
                if (cull_on && !reuse_worth) { tbox.push_back(lo); tbox.push_back(hi); }
            }
        }
        uint32_t root = 0;
        bool contig_m = true, ordered_m = true;
        if (m.n_nodes) {
            if (!m.nodes) return fail(c, RTX_E_INVALID, "mesh nodes missing");
            // Re-lay the tree out for the device: the root at an odd slot, every child pair
            // (left, left + 1) at an even slot so one 64-B scalar load fetches both boxes.
            // Only the numbering changes; the tree and the left-then-right order do not.  The same
            // walk validates the tree (child indices, cycles) and finds its depth: the deepest DFS
            // stack a wave can need (pending right siblings on a path).
            if ((nodes.size() / 2) % 2 == 0) { nodes.push_back(f4(0, 0, 0, 0)); nodes.push_back(f4(0, 0, 0, 0)); }
            root = static_cast<uint32_t>(nodes.size() / 2);
            struct Work { uint32_t src, dst; int depth; };   // (mesh-local node, device slot, depth)
            std::vector<Work> work;
            work.reserve(64);
            work.push_back({0u, root, 0});
            nodes.resize(nodes.size() + 2);
            int depth = 0;
            size_t visited = 0;
            while (!work.empty()) {
                const Work w = work.back();
                work.pop_back();
                const uint32_t src = w.src, dst = w.dst;
                if (++visited > 4ull * m.n_nodes + 4) return fail(c, RTX_E_INVALID, "BVH has a cycle");
                depth = w.depth > depth ? w.depth : depth;
                const rtx_bvh_node& nd = m.nodes[src];
                uint32_t link, cnt;
                if (nd.idx_count == 0 && (nd.left_node + 1 >= m.n_nodes || nd.left_node == 0))
                    return fail(c, RTX_E_INVALID, "BVH child index out of range");
                if (nd.idx_count > 0) {
                    if (nd.first_idx % 3 || nd.idx_count % 3 || nd.first_idx + nd.idx_count > m.n_indices)
                        return fail(c, RTX_E_INVALID, "BVH leaf range invalid");
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
            max_depth = std::max(max_depth, depth);
            if (lay) lay->depth[mi] = depth;
            mesh_slots.push_back({root, static_cast<uint32_t>(nodes.size() / 2)});
            slot_ranges(nodes, root, static_cast<uint32_t>(nodes.size() / 2), slot_rng, contig_m, ordered_m);
            ordered_all = ordered_all && ordered_m;
            if (lay && lay->reserve[mi]) {   // slots root .. root + 2T - 1 belong to this mesh
                const size_t want = 2 * (static_cast<size_t>(root) + 2 * static_cast<size_t>(ntri));
                if (nodes.size() < want) nodes.resize(want + (want / 2) % 2 * 2, f4(0, 0, 0, 0));
            }
        }
        if (lay) { lay->tri0[mi] = tri0; lay->root[mi] = root; }
        const float cs = m.cull_mode == RTX_CULL_FRONT ? -1.f : (m.cull_mode == RTX_CULL_BACK ? 1.f : 0.f);
        // {root node byte offset, node count, cull sign bits, material}
        meshes.push_back(make_int4(static_cast<int>(root * 32u), static_cast<int>(m.n_nodes), bitsi_f(cs), m.material));
        (void)node0;
        // ~48 triangles per part at least: finer parts of a small mesh cost more than they spread
        const uint32_t target = std::max(2u, std::min(c->split_parts, ntri / 48u));
        const size_t p0 = parts.size();
        if (m.n_nodes && !build_parts(nodes, root, mi, target, slot_rng, contig_m, parts)) split_ok = false;
        if (lay && lay->reserve[mi]) {   // exactly `target` entries, the unused ones {-1, ...}
            parts.resize(p0 + target, make_int4(-1, 0, 0, 0));
            lay->part0[mi] = static_cast<uint32_t>(p0);
            lay->part_cap[mi] = target;
        }
    }
    if (parts.size() > static_cast<size_t>(kMaxParts)) split_ok = false;
    if (!split_ok) parts.clear();
    // static uploads reserve kMaxParts entries for the frontier refinement (refine_round); meshes
    // with device-rebuild reserves keep theirs exactly
    bool any_reserve = false;
    if (lay)
        for (uint8_t r : lay->reserve) any_reserve = any_reserve || r != 0;
    const size_t n_parts_real = parts.size();
    const bool refinable = split_ok && n_parts_real > 0 && !any_reserve;
    if (refinable) parts.resize(kMaxParts, make_int4(-1, 0, 0, 0));
    // Cull records' inputs: per node slot the range of device triangles under it (leaf order is
    // contiguous within a subtree; children's slots follow their parent's, so one backward sweep)
    // and per light the tmax up to which its shadow rays are culled: 4x the farthest mesh-box
    // corner + 1 (longer rays pass).
    std::vector<uint2> cull_rng;
    std::vector<float> cull_T;
    if (cull_on) {
        cull_on = !tri.empty() && !mesh_slots.empty();
        for (int a = 0; a < 3; ++a) cull_on = cull_on && std::isfinite(bmin[a]) && std::isfinite(bmax[a]);
    }
    if (cull_on) {
        // Worth it?  The surface areas of the reference's boxes over those of the tight boxes,
        // summed over the nodes (the SAH estimate of how many more slab tests the reference's
        // boxes pass): below c->cull_min_sa the records cost more than they save (measured: W4_Bunny
        // 1.19, -11 %; W4_Optional 2.40, +48 %; Synthetic100k 9.26, +182 %; profiles/r04).
        cull_rng = slot_rng;
        cull_rng.resize(nodes.size() / 2, make_uint2(0u, 0u));
        const bool increasing = ordered_all;   // the ordered walk needs left-then-right = increasing index
        if (reuse_worth) {
            ++c->cull_worth_age;
            cull_on = increasing && c->cull_worth == 1;
        } else {
            std::vector<float> nb(6 * (nodes.size() / 2));
            double sa_ref = 0.0, sa_tight = 0.0;
            auto sa = [](double x, double y, double z) { return 2.0 * (x * y + y * z + z * x); };
            for (const auto& [r0, r1] : mesh_slots)
                for (uint32_t sl = r1; sl-- > r0;) {
                    uint32_t link, cnt;
                    std::memcpy(&link, &nodes[2 * sl + 1].z, 4);
                    std::memcpy(&cnt, &nodes[2 * sl + 1].w, 4);
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
            const bool worth = sa_ref >= c->cull_min_sa * sa_tight;   // false for NaN
            c->cull_worth = worth ? 1 : 0;
            c->cull_worth_age = 0;
            c->cull_worth_sig = worth_sig;
            cull_on = increasing && worth;
        }
        for (uint32_t i = 0; i < s->n_lights; ++i) {
            double R = 0.0;
            for (int k = 0; k < 8; ++k) {
                const double cx = (k & 1) ? bmax[0] : bmin[0], cy = (k & 2) ? bmax[1] : bmin[1],
                             cz = (k & 4) ? bmax[2] : bmin[2];
                const double dx = s->lights[i].origin[0] - cx, dy = s->lights[i].origin[1] - cy,
                             dz = s->lights[i].origin[2] - cz;
                R = std::fmax(R, std::sqrt(dx * dx + dy * dy + dz * dz));
            }
            const double T = 4.0 * R + 1.0;
            cull_T.push_back(std::isfinite(T) && T < 0x1p60 ? static_cast<float>(T) : 0.f);   // 0: never culled
        }
    }
    // Device links are byte offsets (s_load with an SGPR offset, no address arithmetic):
    // inner node -> its child pair (2 slots x 32 B), leaf -> its first 64-B triangle.
    if (tri.size() * 16 >= (1ull << 32) || nodes.size() * 16 >= (1ull << 32) || sph.size() * 16 >= (1ull << 32) ||
        pl.size() * 16 >= (1ull << 32))
        return fail(c, RTX_E_INVALID, "scene too large for 32-bit record offsets");
    for (size_t n = 0; n < nodes.size(); n += 2) {
        uint32_t link, cnt;
        std::memcpy(&link, &nodes[n + 1].z, 4);
        std::memcpy(&cnt, &nodes[n + 1].w, 4);
        nodes[n + 1].z = bits(cnt ? link * 64u : link * 32u);
    }
    // Octant copies of the node array (DevScene::oct_bytes, slab_mask<kSlabOct>): possible
    // when every box is ordered lo <= hi per axis (no NaN).  The reference's quirky bounds
    // (max initialised with FLT_MIN) stay ordered; an empty box would not.
    // Large trees keep one copy: 8 copies of a multi-MB node array crowd the L2 (Synthetic100k,
    // ~2 MB per copy, is 2.5 % faster without them; W4_Optional, 117 KB, 2.5 % faster with).
    const size_t node_bytes = align256(nodes.size() * 16);
    bool oct_ok = !nodes.empty() && node_bytes <= kOctantMaxNodeBytes && 8 * node_bytes < (1ull << 32);
    for (size_t n = 0; oct_ok && n < nodes.size(); n += 2)
        oct_ok = nodes[n].x <= nodes[n].y && nodes[n].z <= nodes[n].w && nodes[n + 1].x <= nodes[n + 1].y;
    // the node section: 8 octant copies (node_bytes apart, written straight into the
    // staging image below) or the one array
    const size_t node_sec = oct_ok ? 8 * node_bytes : nodes.size() * 16;
    for (uint32_t i = 0; i < s->n_lights; ++i) {
        const rtx_light& l = s->lights[i];
        lights.push_back(f4(l.origin[0], l.origin[1], l.origin[2], bitsi(l.type)));
        lights.push_back(f4(l.color[0], l.color[1], l.color[2], l.intensity));
    }
    for (uint32_t i = 0; i < nm; ++i) {
        const rtx_material& m = s->materials[i];
        // BRDF::Lambert(kd, cd) = (cd * kd) / PI (BRDFs.h:14-17), exact binary32 on host
        const float lr = (m.color[0] * m.kd) / RTX_PI, lg = (m.color[1] * m.kd) / RTX_PI, lb = (m.color[2] * m.kd) / RTX_PI;
        mats.push_back(f4(bitsi(m.kind), m.color[0], m.color[1], m.color[2]));
        mats.push_back(f4(m.kd, m.ks, m.exponent, m.metalness));
        mats.push_back(f4(m.roughness, lr, lg, lb));
    }

    struct Sec { const void* p; size_t n; size_t off; };
    Sec secs[] = {{sph.data(), sph.size() * 16, 0},       {sph_mat.data(), sph_mat.size() * 4, 0},
                  {pl.data(), pl.size() * 16, 0},         {tri.data(), tri.size() * 16, 0},
                  {nullptr, node_sec, 0},
                  {meshes.data(), meshes.size() * 16, 0}, {lights.data(), lights.size() * 16, 0},
                  {mats.data(), mats.size() * 16, 0},     {parts.data(), parts.size() * 16, 0},
                  {cull_rng.data(), cull_rng.size() * 8, 0}, {cull_T.data(), cull_T.size() * 4, 0}};
    size_t total = 0;
    for (auto& x : secs) { x.off = total; total += align256(x.n ? x.n : 16); }
    HIP_TRY(c, hipSetDevice(c->device));
    const int k = c->sb_cur < 0 ? 0 : (c->sb_cur ^ 1);
    rtx_ctx::SceneBuf& B = c->sb[k];
    if (B.pending) {   // frames queued against image k (two uploads ago) must be done with it
        HIP_TRY(c, hipEventSynchronize(B.done));
        B.pending = false;
    }
    if (total > B.cap) HIP_TRY(c, B.grow(total));
    // cull records: one copy of the node slots per anchor (kMaxViews cameras, then the lights)
    const size_t cull_stride = align256(nodes.size() * 16);
    const size_t cull_bytes = cull_on ? (kMaxViews + static_cast<size_t>(s->n_lights)) * cull_stride : 0;
    if (cull_on && (cull_stride >= (1ull << 32) || 2 * tri.size() >= (1ull << 32))) cull_on = false;
    if (cull_on && cull_bytes > B.cull.cap) {
        if (const int rc = B.cull.grow(c, cull_bytes, 1); rc != RTX_OK) return rc;
    }
    // Large node arrays send copy 0 only and the device writes copies 1..7 (rtx_octant_expand):
    // 1/8 of the node bytes over PCIe and of the host's staging writes (an upload per animated
    // frame).  Small ones are cheaper as host writes than as one more launch.
    const bool oct_dev = oct_ok && node_bytes >= kOctantDeviceMinBytes;
    // sections in place; only the padding up to the next section is cleared (an upload per
    // animated frame: no full-image memset, no intermediate node image)
    for (size_t i = 0; i < sizeof secs / sizeof secs[0]; ++i) {
        const Sec& x = secs[i];
        const size_t end = i + 1 < sizeof secs / sizeof secs[0] ? secs[i + 1].off : total;
        if (x.p && x.n) std::memcpy(B.h + x.off, x.p, x.n);
        if (!x.p && x.n && oct_ok) {   // octant copy k stores (hi, lo) on the axes set in k
            for (int k = 0; k < (oct_dev ? 1 : 8); ++k) {
                float4* dst = reinterpret_cast<float4*>(B.h + x.off + k * node_bytes);
                const bool mx = k & 1, my = k & 2, mz = k & 4;
                for (size_t n = 0; n < nodes.size(); n += 2) {
                    const float4 a = nodes[n], b = nodes[n + 1];
                    dst[n] = f4(mx ? a.y : a.x, mx ? a.x : a.y, my ? a.w : a.z, my ? a.z : a.w);
                    dst[n + 1] = f4(mz ? b.y : b.x, mz ? b.x : b.y, b.z, b.w);
                }
                std::memset(reinterpret_cast<char*>(dst + nodes.size()), 0, node_bytes - nodes.size() * 16);
            }
        } else if (!x.p && x.n) {
            std::memcpy(B.h + x.off, nodes.data(), x.n);
        }
        std::memset(B.h + x.off + x.n, 0, end - x.off - x.n);
    }
    if (oct_dev) {   // everything but copies 1..7, which the device writes
        const size_t c1 = secs[4].off + node_bytes, c8 = secs[4].off + 8 * node_bytes;
        HIP_TRY(c, hipMemcpyAsync(B.d, B.h, c1, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(B.d + c8, B.h + c8, total - c8, hipMemcpyHostToDevice, c->stream));
        const uint32_t n2 = static_cast<uint32_t>(node_bytes / 32);
        octant_expand(reinterpret_cast<float4*>(B.d + secs[4].off), n2, static_cast<uint32_t>(node_bytes / 16), c->stream);
        HIP_TRY(c, hipGetLastError());
    } else {
        HIP_TRY(c, hipMemcpyAsync(B.d, B.h, total, hipMemcpyHostToDevice, c->stream));
    }
    if (c->sb_cur >= 0) {   // every frame queued so far reads the previous image
        rtx_ctx::SceneBuf& O = c->sb[c->sb_cur];
        HIP_TRY(c, hipEventRecord(O.done, c->stream));
        O.pending = true;
    }
    c->sb_cur = k;
    c->scene_bytes = total;
    char* base = B.d;
    DevScene d{};
    d.spheres = reinterpret_cast<const float4*>(base + secs[0].off);
    d.sphere_mat = reinterpret_cast<const uint32_t*>(base + secs[1].off);
    d.planes = reinterpret_cast<const float4*>(base + secs[2].off);
    d.tris = reinterpret_cast<const Tri*>(base + secs[3].off);
    d.nodes = reinterpret_cast<const float4*>(base + secs[4].off);
    d.meshes = reinterpret_cast<const int4*>(base + secs[5].off);
    d.lights = reinterpret_cast<const float4*>(base + secs[6].off);
    d.materials = reinterpret_cast<const float4*>(base + secs[7].off);
    d.parts = reinterpret_cast<const int4*>(base + secs[8].off);
    d.n_parts = static_cast<uint32_t>(n_parts_real);
    d.n_spheres = s->n_spheres; d.n_planes = s->n_planes; d.n_meshes = s->n_meshes;
    d.n_lights = s->n_lights; d.n_materials = nm;
    d.tri_fast = max_ee <= 0x1p56 ? 1u : 0u;
    d.oct_bytes = (oct_ok && !std::getenv("RTX_NO_OCTANT")) ? static_cast<uint32_t>(node_bytes) : 0u;
    d.n_tris = static_cast<uint32_t>(tri.size() / 4); d.n_nodes = static_cast<uint32_t>(nodes.size() / 2);
    if (cull_on) {
        d.cull = B.cull;
        d.cull_T = reinterpret_cast<const float*>(base + secs[10].off);
        d.cull_stride = static_cast<uint32_t>(cull_stride);
        c->cull_rng = reinterpret_cast<const uint2*>(base + secs[9].off);
        c->cull_nslots = d.n_nodes;
        for (int a = 0; a < 3; ++a) { c->cull_bmin[a] = bmin[a]; c->cull_bmax[a] = bmax[a]; }
        c->cull_ntris = d.n_tris;
        c->cull_n = kCullTreeWG;   // the segment trees' leaves: a power of two >= the triangles
        while (c->cull_n < d.n_tris) c->cull_n *= 2u;
    }
    c->cull_view_valid = 0;
    c->dev = d;
    c->cull_boxes_pending = false;
    if (cull_on) cull_records(c, cull_T, s->lights, s->n_lights);   // (built before the first frame)
    // a BVH kStackDepth or more levels deep renders with the deep-stack variant, unsplit;
    // kStackDepthDeep or more with its stacks in HBM
    c->deep_stack = max_depth >= kStackDepth;
    c->hbm_stack = max_depth >= kStackDepthDeep;
    c->max_depth = static_cast<uint32_t>(max_depth);
    {   // uniform facts for the specialised kernels (kSpec*): the material kinds the geometry
        // references, every light a point light, the sphere / plane / mesh counts
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
        for (uint32_t i = 0; room && i < 5; ++i) c->room_p0[i] = s->planes[i].origin[kRoomAxes[i]];
        c->room_fact = rs.fact;
        c->room_M = rs.M;
        c->scene_spec = kinds | (point ? kSpecPoint : 0) | (s->n_spheres == 0 ? kSpecNoSpheres : 0) |
                        (s->n_planes == 5 ? kSpecFivePlanes : 0) | (s->n_meshes == 1 ? kSpecOneMesh : 0) |
                        (s->n_meshes == 0 ? kSpecNoMesh : 0) | (room ? kSpecRoomPlanes : 0) |
                        (cull_back ? kSpecCullBack : 0);
        c->last_facts = c->scene_spec;   // (rtx_spec_info before the first frame)
        c->last_variant = -1;
    }
    c->split_ok = split_ok && !parts.empty() && !c->deep_stack;
    c->refinable = refinable && c->split_ok && !c->refine.off;
    c->h_parts.assign(parts.begin(), parts.begin() + static_cast<std::ptrdiff_t>(n_parts_real));
    c->h_parts_base = c->h_parts;
    c->parts_dev = reinterpret_cast<int4*>(base + secs[8].off);
    c->refine.reset_upload(c->refinable);
    c->has_scene = true;
    ++c->scene_gen;
    c->scene_sig = std::to_string(d.n_spheres) + "/" + std::to_string(d.n_planes) + "/" + std::to_string(d.n_meshes) +
                   "/" + std::to_string(d.n_tris) + "/" + std::to_string(d.n_lights) + "/" + std::to_string(nm);
    if (lay) {
        lay->max_ee = max_ee;
        lay->total = total;
        lay->oct_bytes = d.oct_bytes;
        lay->tri_off = secs[3].off;
        lay->node_off = secs[4].off;
        lay->part_off = secs[8].off;
        lay->mesh_off = secs[5].off;
    }
    return RTX_OK;
}
}  // namespace rtxh
