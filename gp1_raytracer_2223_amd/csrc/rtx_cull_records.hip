// rtx_cull_records.hip — the exact-cull records of an uploaded image (rtx_cull.h): the
// segment-tree kernels, their launches before a frame, and the device's octant copies of a node array.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "rtx_ctx.h"

using namespace rtxh;

// Octant copies 1..7 of an uploaded node array from copy 0 (blockIdx.y + 1 = octant k):
// copy k stores (hi, lo) on the axes set in k, the same swap the host applies for small
// arrays (upload_scene).  Zero padding maps to zero padding.  `n2` node records of 32 B per
// copy (padding included), copies `stride` float4 apart.
__global__ void __launch_bounds__(256) rtx_octant_expand(float4* __restrict__ nodes, uint32_t n2, uint32_t stride) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n2) return;
    const uint32_t k = blockIdx.y + 1u;
    const float4 a = nodes[2u * i], b = nodes[2u * i + 1u];
    const bool mx = k & 1u, my = k & 2u, mz = k & 4u;
    float4* dst = nodes + static_cast<size_t>(k) * stride;
    dst[2u * i] = make_float4(mx ? a.y : a.x, mx ? a.x : a.y, my ? a.w : a.z, my ? a.z : a.w);
    dst[2u * i + 1u] = make_float4(mz ? b.y : b.x, mz ? b.x : b.y, b.z, b.w);
}

// ---------------------------------------------------------------- exact cull records
// (rtx_cull.h; DevScene::cull).  Each node slot's record needs, over the node's
// triangle range (contiguous in leaf order: children partition their parent's range), the union
// of the triangles' boxes and, per anchor, the largest margin and dt.  Those range reductions
// run over SEGMENT TREES of the per-triangle values: a perfect binary tree over n = 2^k leaves
// (leaf n + i = triangle i, padding leaves hold the identity; node i = comb(2i, 2i + 1)), so a
// slot's range [x, y) is the combination of at most 2 log2(y - x) tree nodes (cull_tree_query),
// found by one thread in log2(y - x) + 1 dependent steps.  The tree is built in the launch that
// computes the leaves: levels 0-6 across the wave, 7-8 in LDS across the 256-thread workgroup,
// and the levels above by the last workgroup of the tree to arrive (an arrival counter).  Total
// work O(N) for the trees and O(S log N) for S slots; critical path O(log N) — the round-4 kernels
// re-reduced each slot's whole range (the root's wave walked every triangle once per anchor:
// 0.57-1.47 ms for Synthetic100k).  Launches, all on the context stream before the frames:
//   rtx_cull_tris        per triangle: the box of (v0, v0 + E1, v0 + E2), rounded outward (after an
//                        upload), and per (anchor, triangle) rtx_cull.h's (margin, dt); the trees
//   rtx_cull_nodes<BOX>  per node slot: the box (queried after an upload, then kept per context)
//                        widened by the range's largest margin and the kernel test's own padding
//                        -> the anchors' records
// Built before the first frame after an upload (the box, every light's anchor and the frame's
// camera anchors: two launches), then again for a view's camera anchor when a frame's view origin
// is not the one its records were made for.  A NaN, infinite or huge (> 2^40) coordinate anywhere gives +inf (the
// record then always passes: the bound's finite-arithmetic domain, rtx_cull.h).
struct CullAnchors {
    float p[kMaxViews + kMaxCullLights][4];   // xyz: the anchor point; w = 0: camera origin, > 0: light with tmax <= w
    float bt[kMaxViews + kMaxCullLights];     // the t bound of the records' dt (lights: = w)
    uint32_t idx[kMaxViews + kMaxCullLights]; // record copy the anchor writes
    uint32_t n;
};

__device__ __forceinline__ float f_rd(double x) {   // largest float <= x (NaN stays NaN)
    float f = static_cast<float>(x);
    if (static_cast<double>(f) > x) f = nextafterf(f, -INFINITY);
    return f;
}
__device__ __forceinline__ float f_ru(double x) {   // smallest float >= x
    float f = static_cast<float>(x);
    if (static_cast<double>(f) < x) f = nextafterf(f, INFINITY);
    return f;
}
__device__ __forceinline__ bool cull_domain(float x) { return fabsf(x) <= 0x1p40f; }   // false for NaN / inf

// The two kinds of tree values.  Margins and dt are >= 0 or +inf (never NaN: the margin kernel
// maps NaN to +inf), so their identity is 0; box bounds never hold a NaN either (an out-of-domain
// triangle's box is (-inf, +inf)), so min / max are exact folds in any order (only the sign of a
// zero bound can depend on the order, and no record test observes it).
// (CullMD, CullBox: rtx_ctx.h)
__device__ __forceinline__ CullMD cull_ident(CullMD*) { return {0.f, 0.f}; }
__device__ __forceinline__ CullBox cull_ident(CullBox*) {
    return {{INFINITY, INFINITY, INFINITY}, 0.f, {-INFINITY, -INFINITY, -INFINITY}, 0.f};
}
__device__ __forceinline__ CullMD cull_comb(const CullMD& a, const CullMD& b) { return {fmaxf(a.m, b.m), fmaxf(a.dt, b.dt)}; }
__device__ __forceinline__ CullBox cull_comb(const CullBox& a, const CullBox& b) {
    CullBox r;
    for (int k = 0; k < 3; ++k) { r.lo[k] = fminf(a.lo[k], b.lo[k]); r.hi[k] = fmaxf(a.hi[k], b.hi[k]); }
    r.pad0 = r.pad1 = 0.f;
    return r;
}
__device__ __forceinline__ CullMD cull_xor(const CullMD& a, int o) { return {__shfl_xor(a.m, o, 64), __shfl_xor(a.dt, o, 64)}; }
__device__ __forceinline__ CullBox cull_xor(const CullBox& a, int o) {
    CullBox r;
    for (int k = 0; k < 3; ++k) { r.lo[k] = __shfl_xor(a.lo[k], o, 64); r.hi[k] = __shfl_xor(a.hi[k], o, 64); }
    r.pad0 = r.pad1 = 0.f;
    return r;
}

// Write-through (sc1) 8-byte stores and loads of tree values: the workgroup roots are handed to
// the last workgroup INSIDE the launch, across XCDs whose L2s are not coherent.  A plain store
// stays in the writer's L2 (a release fence writes it back, but the reader's L2 may still hold an
// older copy of the line: an acquire invalidates only L1), so the roots are stored write-through
// by the one lane that then adds to the arrival counter after its stores drained, and the last
// workgroup reads them write-through too (MI355X_MICROARCH.md, inter-workgroup visibility: the
// "one lane per storing workgroup, last arriver by the add's value" form).
template <class V>
__device__ __forceinline__ void cull_st_wt(V* p, const V& v) {
    static_assert(sizeof(V) % 8 == 0, "8-byte pieces");
    unsigned long long w[sizeof(V) / 8];
    __builtin_memcpy(w, &v, sizeof(V));
    for (size_t k = 0; k < sizeof(V) / 8; ++k)
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(p) + k, w[k], __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}
template <class V>
__device__ __forceinline__ V cull_ld_wt(const V* p) {
    unsigned long long w[sizeof(V) / 8];
    for (size_t k = 0; k < sizeof(V) / 8; ++k)
        w[k] = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p) + k, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
    V v;
    __builtin_memcpy(&v, w, sizeof(V));
    return v;
}

// Leaf i = blockIdx.x * kCullTreeWG + threadIdx.x holds v; writes the tree levels of `t` (2n
// entries, n = gridDim.x * kCullTreeWG).  `arrive`: the tree's arrival counter (0 before the
// launch, 0 again after it); `top_lds` (<= kCullTopLds): the most workgroup roots the last
// workgroup combines in LDS (tests lower it to exercise the global-memory path).  Levels below
// the workgroup roots are read only by later launches (plain stores).
template <class V>
__device__ void cull_tree_build(V v, V* __restrict__ t, uint32_t* arrive, uint32_t top_lds) {
    __shared__ V part[kCullTreeWG / 64];
    __shared__ V top[kCullTopLds / 2];
    __shared__ uint32_t last;
    const uint32_t tid = threadIdx.x, nwg = gridDim.x, n = nwg * kCullTreeWG;
    const uint32_t leaf = n + blockIdx.x * kCullTreeWG + tid;
    t[leaf] = v;
    for (int k = 1; k <= 6; ++k) {   // levels 1-6: butterflies over aligned 2^k lanes
        v = cull_comb(v, cull_xor(v, 1 << (k - 1)));
        if ((tid & ((1u << k) - 1u)) == 0u) t[leaf >> k] = v;
    }
    if ((tid & 63u) == 0u) part[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) {   // levels 7 and 8 (kCullTreeWG = 256 = 4 waves); the root write-through
        const V a = cull_comb(part[0], part[1]), b = cull_comb(part[2], part[3]), r = cull_comb(a, b);
        t[leaf >> 7] = a;
        t[(leaf >> 7) + 1u] = b;
        cull_st_wt(t + (leaf >> 8), r);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the root has left before the arrival
        last = atomicAdd(arrive, 1u) == nwg - 1u ? 1u : 0u;
    }
    __syncthreads();
    if (!last) return;
    // levels above 8: the workgroup roots are nodes [nwg, 2 nwg); node j of a level = comb(2j, 2j + 1)
    if (nwg == 1u) {
        // the workgroup's root is the tree's
    } else if (nwg <= top_lds) {
        for (uint32_t w = tid; w < nwg / 2u; w += kCullTreeWG)
            top[w] = cull_comb(cull_ld_wt(t + nwg + 2u * w), cull_ld_wt(t + nwg + 2u * w + 1u));
        for (uint32_t c = nwg / 2u;; c >>= 1) {   // `top` holds level-nodes [c, 2c)
            __syncthreads();
            for (uint32_t w = tid; w < c; w += kCullTreeWG) t[c + w] = top[w];
            if (c == 1u) break;
            V r[kCullTopLds / 2 / kCullTreeWG];
            uint32_t q = 0;
            for (uint32_t w = tid; w < c / 2u; w += kCullTreeWG) r[q++] = cull_comb(top[2u * w], top[2u * w + 1u]);
            __syncthreads();
            q = 0;
            for (uint32_t w = tid; w < c / 2u; w += kCullTreeWG) top[w] = r[q++];
        }
    } else {   // level by level through memory, every access write-through (this workgroup's own
               // stores are read back by its other waves: past their L1s)
        for (uint32_t c = nwg / 2u; c >= 1u; c >>= 1) {
            for (uint32_t w = tid; w < c; w += kCullTreeWG)
                cull_st_wt(t + c + w, cull_comb(cull_ld_wt(t + 2u * (c + w)), cull_ld_wt(t + 2u * (c + w) + 1u)));
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
    }
    if (tid == 0) __hip_atomic_store(arrive, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // next launch
}

// the combination of the leaves [x, y) (x <= y <= n)
template <class V>
__device__ __forceinline__ V cull_tree_query(const V* __restrict__ t, uint32_t n, uint32_t x, uint32_t y) {
    V acc = cull_ident(static_cast<V*>(nullptr));
    for (uint32_t l = x + n, r = y + n; l < r; l >>= 1, r >>= 1) {
        if (l & 1u) acc = cull_comb(acc, t[l++]);
        if (r & 1u) acc = cull_comb(acc, t[--r]);
    }
    return acc;
}

// grid (n / kCullTreeWG, A.n + box): blockIdx.y = j < A.n builds anchor j's (margin, dt) tree at
// trees + 2n j (counter arrive[j]); j = A.n (when `box`) the box tree (counter arrive[kCullMaxAnchors]).
__global__ void __launch_bounds__(kCullTreeWG) rtx_cull_tris(const Tri* __restrict__ tris, uint32_t nt,
                                                             const CullAnchors A, CullMD* __restrict__ trees,
                                                             CullBox* __restrict__ btree, uint32_t* arrive,
                                                             uint32_t top_lds) {
    const uint32_t i = blockIdx.x * kCullTreeWG + threadIdx.x, j = blockIdx.y;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a, c = a;
    if (i < nt) { a = tris[i].a; b = tris[i].b; c = tris[i].c; }
    const float v0[3] = {a.x, a.y, a.z}, e1[3] = {b.x, b.y, b.z}, e2[3] = {c.x, c.y, c.z};
    if (j == A.n) {   // the per-triangle box of (v0, v0 + E1, v0 + E2), rounded outward
        CullBox v = cull_ident(static_cast<CullBox*>(nullptr));
        if (i < nt) {
            bool ok = true;
            for (int k = 0; k < 3; ++k) {
                ok = ok && cull_domain(v0[k]) && cull_domain(e1[k]) && cull_domain(e2[k]);
                const double p = v0[k], q = p + static_cast<double>(e1[k]), r = p + static_cast<double>(e2[k]);
                const double mn = fmin(p, fmin(q, r)), mx = fmax(p, fmax(q, r));
                // the double sums are exact unless the exponents differ by > 29: widen by 2^-40 anyway
                v.lo[k] = f_rd(mn - fabs(mn) * 0x1p-40);
                v.hi[k] = f_ru(mx + fabs(mx) * 0x1p-40);
            }
            if (!ok)   // out of the domain: every box holding it passes every ray
                for (int k = 0; k < 3; ++k) { v.lo[k] = -INFINITY; v.hi[k] = INFINITY; }
        }
        cull_tree_build(v, btree, arrive + kCullMaxAnchors, top_lds);
        return;
    }
    CullMD v{0.f, 0.f};
    if (i < nt) {   // anchor j's bound for triangle i (rtx_cull.h), NaN -> inf
        rtx_cull_tri T;
        rtx_cull_tri_setup(&T, v0, e1, e2);
        const float* p = A.p[j];
        const rtx_cull_bound bd = p[3] > 0.f ? rtx_cull_light_bounds(&T, p, p[3]) : rtx_cull_point_bounds(&T, p, A.bt[j]);
        v.m = (bd.margin >= 0.0 && bd.margin < 0x1p100) ? f_ru(bd.margin) : INFINITY;
        v.dt = (bd.dt >= 0.0 && bd.dt < 0x1p100) ? f_ru(bd.dt) : INFINITY;
    }
    cull_tree_build(v, trees + 2ull * gridDim.x * kCullTreeWG * j, arrive + j, top_lds);
}

// Which records the walk tests (CullParams): a box some axis of which the reference's box (node
// copy 0) exceeds `ratio` times — the reference's FLT_MIN-inflated boxes, DataTypes.h:315 — and,
// with `leaves`, only leaf nodes.  Unflagged records are loaded but cost no vector work.
struct CullParams {
    const float4* nodes;   // node copy 0 (reference boxes, {min.x, max.x, min.y, max.y}, {min.z, max.z, link, ntri})
    float ratio;
    uint32_t leaves;
};
// the record of `slot` for anchor copy `a`: tight box [lo, hi] widened by `m` and the padding
// 16u (E + |c|) of cull_mask's rounding (2^-20 = 16u); w of its second half = the test flag
__device__ __forceinline__ void cull_write(float4* __restrict__ cull, uint32_t stride4, uint32_t a, uint32_t slot,
                                           const float* lo, const float* hi, bool bad, float m, float dt,
                                           const CullParams& P) {
    float cf[3], Ef[3];
    for (int k = 0; k < 3; ++k) {
        const double c = 0.5 * (static_cast<double>(lo[k]) + hi[k]);
        cf[k] = static_cast<float>(c);
        double E = 0.5 * (static_cast<double>(hi[k]) - lo[k]) + fabs(c - cf[k]) + static_cast<double>(m);
        E = (E + 0x1p-20 * (E + fabs(static_cast<double>(cf[k])))) * (1.0 + 0x1p-40) +
            0x1p-50 * (fabs(static_cast<double>(lo[k])) + fabs(static_cast<double>(hi[k])));
        Ef[k] = (!bad && E < 0x1p100) ? f_ru(E) : INFINITY;   // NaN and empty boxes pass every ray
        if (bad || !(E < 0x1p100)) cf[k] = 0.f;
    }
    const float4 n0 = P.nodes[2u * slot], n1 = P.nodes[2u * slot + 1u];
    const float ref[3] = {n0.y - n0.x, n0.w - n0.z, n1.y - n1.x};
    bool worth = false;
    for (int k = 0; k < 3; ++k) worth = worth || ref[k] > P.ratio * 2.f * Ef[k];   // false for inf / NaN
    if (P.leaves && __float_as_uint(n1.w) == 0u) worth = false;
    float4* r = cull + static_cast<size_t>(a) * stride4 + 2u * slot;
    r[0] = make_float4(cf[0], cf[1], cf[2], Ef[0]);
    r[1] = make_float4(Ef[1], Ef[2], (bad || !(dt < 0x1p100f)) ? INFINITY : dt, __uint_as_float(worth ? 1u : 0u));
}

// One thread per node slot.  BOX (after an upload): the slot's box from the box tree, kept in `nbox`
// for the camera anchors' later launches; else read from `nbox`.  An empty range (padding slot)
// or a box with an infinite bound (an out-of-domain triangle below) gives the always-pass record.
// (Reducing the box and several anchors' trees in one walk up the levels, their loads issued
// together, measured slower: Synthetic100k camera records 11.2 -> 34.8 us, profiles/r05.)
template <bool BOX>
__global__ void __launch_bounds__(256) rtx_cull_nodes(const uint2* __restrict__ rng, uint32_t nslots, uint32_t ntris,
                                                      uint32_t n, const CullBox* __restrict__ btree,
                                                      CullBox* __restrict__ nbox, const CullMD* __restrict__ trees,
                                                      const CullAnchors A, float4* __restrict__ cull, uint32_t stride4,
                                                      const CullParams P) {
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s >= nslots) return;
    const uint2 r = rng[s];
    const bool empty = r.y <= r.x || r.y > ntris;
    CullBox b;
    if (BOX) {
        b = empty ? cull_ident(static_cast<CullBox*>(nullptr)) : cull_tree_query(btree, n, r.x, r.y);
        nbox[s] = b;
    } else {
        b = nbox[s];
    }
    bool bad = empty;
    for (int k = 0; k < 3; ++k) bad = bad || !(fabsf(b.lo[k]) < INFINITY) || !(fabsf(b.hi[k]) < INFINITY);
    for (uint32_t j = 0; j < A.n; ++j) {
        const CullMD md = bad ? CullMD{0.f, 0.f} : cull_tree_query(trees + 2ull * n * j, n, r.x, r.y);
        cull_write(cull, stride4, A.idx[j], s, b.lo, b.hi, bad, md.m, md.dt, P);
    }
}

namespace {
// Queue the record launches on the context stream: with `boxes` (at upload) the box tree and
// every slot's box, then, for the anchors in A, their margin trees and records.  Grows the
// scratch (after a stream sync: queued launches may still read the old buffers).
int cull_launch(rtx_ctx* c, const CullAnchors& A, bool boxes) {
    const uint32_t nt = c->cull_ntris;
    const uint32_t n = c->cull_n;
    if (c->cull_fail_at && ++c->cull_launches == c->cull_fail_at)   // RTX_CULL_FAIL (tests of the error path)
        return fail(c, RTX_E_NOMEM, "cull records: injected failure (RTX_CULL_FAIL)");
    // the anchors' margin trees: 2n entries per anchor of THIS launch (an upload's first launch has the
    // lights and the views, later ones the views that moved), grown on demand
    const size_t mtree_need = 2 * static_cast<size_t>(n) * std::max<uint32_t>(A.n, 1u);
    if (n > c->d_cull_btree.cap || mtree_need > c->d_cull_mtree.cap || c->cull_nslots > c->d_cull_nbox.cap ||
        !c->d_cull_arrive) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        int rc = RTX_OK;
        if (n > c->d_cull_btree.cap) rc = c->d_cull_btree.grow(c, n, 2 * sizeof(CullBox));
        if (rc == RTX_OK && mtree_need > c->d_cull_mtree.cap)
            rc = c->d_cull_mtree.grow(c, mtree_need);
        if (rc == RTX_OK && c->cull_nslots > c->d_cull_nbox.cap)
            rc = c->d_cull_nbox.grow(c, c->cull_nslots);
        if (rc != RTX_OK) return rc;
        if (!c->d_cull_arrive) {
            if (const int rc2 = c->d_cull_arrive.grow(c, kCullMaxAnchors + 1); rc2 != RTX_OK) return rc2;
            // on the context stream: a plain hipMemset runs on the null stream, which this
            // non-blocking stream does not wait for (the first tree launch then read whatever the
            // recycled allocation held as its arrival counts)
            HIP_TRY(c, hipMemsetAsync(c->d_cull_arrive, 0, (kCullMaxAnchors + 1) * sizeof(uint32_t), c->stream));
        }
    }
    for (uint32_t j = 0; j < A.n; ++j) {
        for (int k = 0; k < 4; ++k) c->cull_anchor[A.idx[j]][k] = A.p[j][k];
        c->cull_anchor[A.idx[j]][4] = A.bt[j];
    }
    const uint32_t nwg = n / kCullTreeWG, sb = (c->cull_nslots + 255u) / 256u;
    float4* rec = const_cast<float4*>(c->dev.cull);
    const uint32_t stride4 = c->dev.cull_stride / 16u;
    const CullParams P{c->dev.nodes, c->cull_ratio, c->cull_leaves ? 1u : 0u};
    if (A.n || boxes) {
        hipLaunchKernelGGL(rtx_cull_tris, dim3(nwg, A.n + (boxes ? 1u : 0u)), dim3(kCullTreeWG), 0, c->stream,
                           c->dev.tris, nt, A, c->d_cull_mtree, c->d_cull_btree, c->d_cull_arrive, c->cull_top_lds);
        HIP_TRY(c, hipGetLastError());
    }
    if (boxes) {
        hipLaunchKernelGGL(rtx_cull_nodes<true>, dim3(sb), dim3(256), 0, c->stream, c->cull_rng, c->cull_nslots, nt, n,
                           c->d_cull_btree, c->d_cull_nbox, c->d_cull_mtree, A, rec, stride4, P);
    } else if (A.n) {
        hipLaunchKernelGGL(rtx_cull_nodes<false>, dim3(sb), dim3(256), 0, c->stream, c->cull_rng, c->cull_nslots, nt,
                           n, c->d_cull_btree, c->d_cull_nbox, c->d_cull_mtree, A, rec, stride4, P);
    }
    HIP_TRY(c, hipGetLastError());
    return RTX_OK;
}
}  // namespace

namespace rtxh {

void octant_expand(float4* nodes, uint32_t n2, uint32_t stride, hipStream_t s) {
    hipLaunchKernelGGL(rtx_octant_expand, dim3((n2 + 255) / 256, 7), dim3(256), 0, s, nodes, n2, stride);
}

// At upload: the light anchors (tmax bound T[l]) the first frame's record launches build, with the
// per-triangle boxes (cull_views).
void cull_records(rtx_ctx* c, const std::vector<float>& T, const rtx_light* lights, uint32_t n_lights) {
    c->cull_lights.clear();
    for (uint32_t l = 0; l < n_lights; ++l)
        c->cull_lights.push_back({lights[l].origin[0], lights[l].origin[1], lights[l].origin[2],
                                  T[l] > 0.f ? T[l] : 1.f});   // T = 0: never culled (cull_ray), any bound will do
    c->cull_boxes_pending = true;
}

// Before a frame: after an upload the boxes and the lights' records, and the records of every view
// whose camera origin is not the one its records of the current image were made for (bitwise).
// The records' state (pending boxes, valid views) is committed only once their launches are queued:
// when building them fails (an allocation), the image renders without the cull from then on — the
// unculled walk, the same pixels — instead of a later frame trusting records never written.
int cull_views(rtx_ctx* c, const FrameArgs& F) {
    CullAnchors A{};
    const bool boxes = c->cull_boxes_pending;
    // after an upload every light's anchor; after an edit (rtx_edit.hip) the moved lights' alone
    const uint32_t lights = boxes ? ~0u : c->cull_lights_dirty;
    if (lights) {
        for (size_t l = 0; l < c->cull_lights.size(); ++l) {
            if (!((lights >> l) & 1u)) continue;
            for (int k = 0; k < 4; ++k) A.p[A.n][k] = c->cull_lights[l][k];
            A.bt[A.n] = A.p[A.n][3];
            A.idx[A.n] = static_cast<uint32_t>(kMaxViews + l);
            ++A.n;
        }
    }
    const uint32_t light_anchors = A.n;
    uint32_t valid = c->cull_view_valid;
    for (uint32_t v = 0; v < F.n_views && v < static_cast<uint32_t>(kMaxViews); ++v) {
        const float* o = F.cam[v].origin;
        if ((valid >> v) & 1u && std::memcmp(c->cull_view[v], o, 12) == 0) continue;
        valid |= 1u << v;
        for (int k = 0; k < 3; ++k) A.p[A.n][k] = o[k];
        A.p[A.n][3] = 0.f;
        A.bt[A.n] = F.cam[v].cull_bt;
        A.idx[A.n] = v;
        ++A.n;
    }
    if (A.n == 0 && !boxes) return RTX_OK;
    if (cull_launch(c, A, boxes) != RTX_OK) {   // (c->err says why)
        c->dev.cull = nullptr;
        c->dev.cull_T = nullptr;
        c->dev.cull_stride = 0;
        c->cull_boxes_pending = false;
        c->cull_lights_dirty = 0;
        c->cull_view_valid = 0;
        ++c->cull_failures;
        (void)hipGetLastError();
        return RTX_OK;
    }
    if (A.n > light_anchors) ++c->cull_updates;
    for (uint32_t j = 0; j < A.n; ++j)
        if (A.idx[j] < static_cast<uint32_t>(kMaxViews)) std::memcpy(c->cull_view[A.idx[j]], A.p[j], 12);
    c->cull_view_valid = valid;
    c->cull_boxes_pending = false;
    c->cull_lights_dirty = 0;
    return RTX_OK;
}

}  // namespace rtxh
