// rtx_sched.hip — the cost-ordered tile schedule: the kernels that turn a measured frame's per-tile
// costs into the next frames' dispatch order and heavy set, and the launches that queue them.
#include <algorithm>

#include "rtx_ctx.h"

using namespace rtxh;

// Next frames' dispatch order from this frame's per-tile cost: heaviest first, STABLE
// within a cost class so that tiles rendered together stay spatial neighbours (they walk
// the same BVH nodes: scalar-cache locality).  The order is (class, tile index): the same
// permutation a serial counting sort would give, computed by three launches over chunks of
// kSchedChunk tiles (one 256-thread workgroup each):
//   rtx_sched_count    per chunk: class histogram + cost sum (and the saved-cost fix-up)
//   rtx_sched_scan     one workgroup: exclusive prefix of the histograms in (class, chunk)
//                      order, the heavy threshold
//   rtx_sched_scatter  per chunk: every tile's slot = its (class, chunk) base + its rank
//                      among the chunk's tiles of that class; heavy flags / list; clears costs
// It also picks the heavy tiles for split rendering: cost > split_permille/1000 x (total cost /
// min(tiles, concurrent workgroup slots)), i.e. a tile that alone would outlast its share of
// the frame.  `split_slots` = 0 disables splitting, UINT32_MAX forces every tile heavy
// (tests).  Flags and list go to the staging set the host adopts at its next frame.
__device__ __forceinline__ uint32_t cost_class(uint32_t cst) {   // heavier -> smaller class
    const uint32_t lg = cst ? 32u - static_cast<uint32_t>(__builtin_clz(cst)) : 0u;   // 0..32
    const uint32_t half = (cst && lg >= 2) ? ((cst >> (lg - 2)) & 1u) : 0u;
    uint32_t k = 2u * lg + half;                                                     // 0..65
    k = k > 2u * 6u ? k - 2u * 6u : 0u;        // costs below 48 (x16 cycles) share the last class
    return (kCostBuckets - 1) - (k < kCostBuckets ? k : kCostBuckets - 1);
}

// A tile rendered split this frame has no fresh one-piece cost: it keeps the one it had
// when it was last rendered whole (kept in `saved`) — or, with `parts` (motion mode: the camera
// moves, so that cost goes stale), the sum of its split waves' durations for this frame's sort,
// which lets a tile that stopped being heavy leave the split set (`saved` is left as it was).
__global__ void __launch_bounds__(kReorderThreads) rtx_sched_count(uint32_t* __restrict__ cost, uint32_t n,
                                                                   const uint32_t* __restrict__ was_heavy,
                                                                   uint32_t* __restrict__ saved,
                                                                   uint32_t* __restrict__ hist,
                                                                   unsigned long long* __restrict__ csum,
                                                                   uint32_t nchunks, uint32_t parts,
                                                                   uint32_t* __restrict__ max_cost) {
    __shared__ uint32_t h[kCostBuckets];
    __shared__ unsigned long long tot;
    __shared__ uint32_t mx;
    const uint32_t tid = threadIdx.x, base = blockIdx.x * kSchedChunk;
    if (tid < kCostBuckets) h[tid] = 0;
    if (tid == 0) {
        tot = 0;
        mx = 0;
    }
    __syncthreads();
    unsigned long long my = 0;
    uint32_t my_max = 0;
    for (uint32_t k = 0; k < kSchedChunk / kReorderThreads; ++k) {
        const uint32_t t = base + k * kReorderThreads + tid;   // coalesced; counting ignores order
        if (t >= n) break;
        uint32_t c = cost[t];
        if (was_heavy && was_heavy[t]) {
            // split this frame: static frames sort it by the one-piece cost it had when last
            // rendered whole; motion mode by its part waves' sum (cost[t]), which stands in for this
            // frame only — the saved one-piece cost stays (a part sum leaves out each part wave's
            // fixed work, so it would cost the tile low once motion ends)
            if (!parts) {
                c = saved[t];
                cost[t] = c;
            }
        } else {
            saved[t] = c;
        }
        atomicAdd(&h[cost_class(c)], 1u);
        my += c;
        my_max = c > my_max ? c : my_max;
    }
    atomicAdd(&tot, my);
    atomicMax(&mx, my_max);
    __syncthreads();
    if (tid < kCostBuckets) hist[tid * nchunks + blockIdx.x] = h[tid];
    if (tid == 0) {
        csum[blockIdx.x] = tot;
        atomicMax(max_cost, mx);
    }
}

// Exclusive prefix of hist[class][chunk] in class-major order (in place), the total cost and
// the heavy threshold; zeroes the heavy counter the scatter appends to.
__global__ void __launch_bounds__(kScanThreads) rtx_sched_scan(uint32_t* __restrict__ hist, uint32_t nchunks,
                                                               const unsigned long long* __restrict__ csum, uint32_t n,
                                                               uint32_t split_slots, uint32_t split_permille,
                                                               uint32_t split_min, uint32_t wave_slots,
                                                               unsigned long long* __restrict__ thr_out,
                                                               uint32_t* __restrict__ heavy_n) {
    __shared__ uint32_t part[kScanThreads];
    __shared__ unsigned long long cpart[kScanThreads];
    const uint32_t tid = threadIdx.x;
    const uint32_t len = kCostBuckets * nchunks;
    const uint32_t per = (len + kScanThreads - 1) / kScanThreads;
    const uint32_t lo = tid * per, hi = (lo + per < len) ? lo + per : len;
    uint32_t s = 0;
    for (uint32_t i = lo; i < hi; ++i) s += hist[i];
    unsigned long long cs = 0;
    for (uint32_t i = tid; i < nchunks; i += kScanThreads) cs += csum[i];
    part[tid] = s;
    cpart[tid] = cs;
    __syncthreads();
    for (uint32_t o = 1; o < kScanThreads; o <<= 1) {   // inclusive Hillis-Steele scan
        const uint32_t v = tid >= o ? part[tid - o] : 0u;
        const unsigned long long w = tid >= o ? cpart[tid - o] : 0ull;
        __syncthreads();
        part[tid] += v;
        cpart[tid] += w;
        __syncthreads();
    }
    uint32_t acc = part[tid] - s;   // exclusive
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t v = hist[i];
        hist[i] = acc;
        acc += v;
    }
    if (tid == 0) {
        const unsigned long long total = cpart[kScanThreads - 1];
        const bool force = split_slots == 0xffffffffu;
        // (split_min: no tile below it is split, whatever its share of the frame)
        const unsigned long long thr =
            split_slots ? total * split_permille / (1000ull * (n < split_slots ? n : split_slots)) : ~0ull;
        *thr_out = force ? 0ull : (thr > split_min ? thr : static_cast<unsigned long long>(split_min));
        heavy_n[0] = 0;
        // the frame's heaviest tile (rtx_sched_count's maximum, zeroed for the next measurement) and
        // its cost per wave slot, for the in-flight choice (kInflightCritPermille)
        heavy_n[2] = heavy_n[1];
        heavy_n[1] = 0;
        const unsigned long long per = wave_slots ? total / (n < wave_slots ? n : wave_slots) : 0ull;
        heavy_n[3] = static_cast<uint32_t>(per < 0xffffffffull ? per : 0xffffffffull);
    }
}

__global__ void __launch_bounds__(kReorderThreads) rtx_sched_scatter(uint32_t* __restrict__ cost,
                                                                     uint32_t* __restrict__ order, uint32_t n,
                                                                     const uint32_t* __restrict__ hist,
                                                                     uint32_t nchunks,
                                                                     const unsigned long long* __restrict__ thr_in,
                                                                     uint32_t force, uint32_t* __restrict__ heavy_flag,
                                                                     uint32_t* __restrict__ heavy_list,
                                                                     uint32_t* __restrict__ heavy_n) {
    constexpr uint32_t kPer = kSchedChunk / kReorderThreads;   // consecutive tiles per thread
    constexpr uint32_t kSeg = kCostBuckets;   // (class, thread) entries scanned per thread: 32 x 256 / 256
    __shared__ uint32_t cnt[kCostBuckets][kReorderThreads];
    __shared__ uint32_t tsum[kReorderThreads];
    const uint32_t tid = threadIdx.x, base = blockIdx.x * kSchedChunk + tid * kPer;
    uint32_t cls[kPer], cst[kPer];
    for (uint32_t k = 0; k < kCostBuckets; ++k) cnt[k][tid] = 0;
    for (uint32_t k = 0; k < kPer; ++k) {
        const uint32_t t = base + k;
        cst[k] = t < n ? cost[t] : 0u;
        cls[k] = cost_class(cst[k]);
        if (t < n) cnt[cls[k]][tid]++;
    }
    __syncthreads();
    // exclusive scan of cnt flattened in (class, thread) order: thread j scans kSeg
    // consecutive entries, then the per-thread sums are scanned
    uint32_t* flat = &cnt[0][0];
    uint32_t s = 0;
    for (uint32_t i = 0; i < kSeg; ++i) s += flat[tid * kSeg + i];
    tsum[tid] = s;
    __syncthreads();
    for (uint32_t off = 1; off < kReorderThreads; off <<= 1) {
        const uint32_t v = tid >= off ? tsum[tid - off] : 0u;
        __syncthreads();
        tsum[tid] += v;
        __syncthreads();
    }
    uint32_t acc = tsum[tid] - s;
    for (uint32_t i = 0; i < kSeg; ++i) {
        const uint32_t v = flat[tid * kSeg + i];
        flat[tid * kSeg + i] = acc;
        acc += v;
    }
    __syncthreads();
    // slot = global (class, chunk) base + rank within the chunk's class (= flattened prefix
    // minus the prefix at the class's first thread) + rank within the thread
    const unsigned long long thr = *thr_in;
    uint32_t seen[kPer];
    for (uint32_t k = 0; k < kPer; ++k) {
        seen[k] = 0;
        for (uint32_t j = 0; j < k; ++j) seen[k] += cls[j] == cls[k];
    }
    for (uint32_t k = 0; k < kPer; ++k) {
        const uint32_t t = base + k;
        if (t >= n) break;
        const uint32_t c = cls[k];
        order[hist[c * nchunks + blockIdx.x] + (cnt[c][tid] - cnt[c][0]) + seen[k]] = t;
        uint32_t f = 0;
        if (force || cst[k] > thr) {
            const uint32_t h = atomicAdd(heavy_n, 1u);
            if (h < static_cast<uint32_t>(kMaxHeavyTiles)) { heavy_list[h] = t; f = 1; }
        }
        heavy_flag[t] = f;
        cost[t] = 0;
    }
}

// XCD-affine dispatch (RTX_XCD_ORDER=1, rtx_ctx::xcd_order): workgroups are dealt round robin over the 8
// XCDs (MI355X_MICROARCH.md, workgroup dispatch), so positions p and p + 8 of the dispatch order run on
// one XCD.  This pass re-deals the cost order so that position 8k + r holds the k-th tile, in cost order,
// of class r (each view cut into 8 x 8 blocks, block (i, j) in class (i + 3 j) mod 8): each XCD's L2 then
// serves eight blocks' BVH nodes, triangles and cull records instead of the whole screen's.  (One
// compact region per class, a 4 x 2 grid, measured 1.4-2x slower: the in-order round-robin dispatch
// then waits on the XCD of the heaviest region, profiles/r06/xcd_ab.txt.)  Regions hold unequal
// counts; once the smallest is exhausted the remaining tiles follow in cost order.  One workgroup, three
// passes over each thread's consecutive positions (counts, ranks, writes); a permutation, so no pixel
// changes.
#ifndef RTX_XCD_BLOCKS
#define RTX_XCD_BLOCKS 8   // the view cut into B x B blocks, dealt to the 8 classes as a Latin square
#endif
__device__ __forceinline__ uint32_t xcd_region(uint32_t tile, uint32_t tiles_x, uint32_t tiles_y) {
    const uint32_t per_view = tiles_x * tiles_y;
    const uint32_t rem = tile % per_view, bx = rem % tiles_x, gy = rem / tiles_x;
    const uint32_t i = bx * RTX_XCD_BLOCKS / tiles_x, j = gy * RTX_XCD_BLOCKS / tiles_y;
    // every row and column of blocks holds each class (RTX_XCD_BLOCKS = 8) or each class equally often:
    // a compact heavy area (the Bunny, the heightfield's grazing band) spreads over the classes
    return (i + 3u * j) % 8u;
}
__global__ void __launch_bounds__(kScanThreads) rtx_sched_xcd(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                              uint32_t n, uint32_t tiles_x, uint32_t tiles_y) {
    __shared__ uint32_t cnt[8][kScanThreads];
    __shared__ uint32_t ovf[kScanThreads];
    __shared__ uint32_t tot[8];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (n + kScanThreads - 1) / kScanThreads;
    const uint32_t lo = tid * per < n ? tid * per : n, hi = lo + per < n ? lo + per : n;
    uint32_t c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t p = lo; p < hi; ++p) ++c[xcd_region(in[p], tiles_x, tiles_y)];
    for (int r = 0; r < 8; ++r) cnt[r][tid] = c[r];
    __syncthreads();
    if (tid < 8) {   // exclusive scan of region tid's counts over the threads
        uint32_t acc = 0;
        for (uint32_t t = 0; t < kScanThreads; ++t) {
            const uint32_t v = cnt[tid][t];
            cnt[tid][t] = acc;
            acc += v;
        }
        tot[tid] = acc;
    }
    __syncthreads();
    uint32_t m = tot[0];
    for (int r = 1; r < 8; ++r) m = tot[r] < m ? tot[r] : m;
    uint32_t k[8], o = 0;
    for (int r = 0; r < 8; ++r) k[r] = cnt[r][tid];
    for (uint32_t p = lo; p < hi; ++p) o += k[xcd_region(in[p], tiles_x, tiles_y)]++ >= m ? 1u : 0u;
    ovf[tid] = o;
    __syncthreads();
    if (tid == 0) {   // exclusive scan of the overflow counts
        uint32_t acc = 0;
        for (uint32_t t = 0; t < kScanThreads; ++t) {
            const uint32_t v = ovf[t];
            ovf[t] = acc;
            acc += v;
        }
    }
    __syncthreads();
    for (int r = 0; r < 8; ++r) k[r] = cnt[r][tid];
    o = ovf[tid];
    for (uint32_t p = lo; p < hi; ++p) {
        const uint32_t t = in[p], r = xcd_region(t, tiles_x, tiles_y), kr = k[r]++;
        out[kr < m ? 8u * kr + r : 8u * m + o++] = t;
    }
}

namespace rtxh {

// The schedule's launches, the only place that queues them: count, scan, scatter and, with an
// `order_xcd`, the XCD re-deal, on stream `s`.  Nothing of a context is read: a frame's update
// (sched_update) and the diagnostics' run on given costs (rtx_schedule_run) both come through here.
hipError_t sched_launch(hipStream_t s, const SchedBufs& B, const SchedParams& P) {
    const uint32_t nch = (P.n_tiles + kSchedChunk - 1) / kSchedChunk;
    hipLaunchKernelGGL(rtx_sched_count, dim3(nch), dim3(kReorderThreads), 0, s, B.cost, P.n_tiles, B.was_heavy,
                       B.saved, B.hist, B.csum, nch, P.parts, B.heavy_n + 1);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(rtx_sched_scan, dim3(1), dim3(kScanThreads), 0, s, B.hist, nch, B.csum, P.n_tiles,
                       P.split_slots, P.permille, P.split_min, P.wave_slots, B.thr, B.heavy_n);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(rtx_sched_scatter, dim3(nch), dim3(kReorderThreads), 0, s, B.cost, B.order, P.n_tiles, B.hist,
                       nch, B.thr, P.split_slots == 0xffffffffu ? 1u : 0u, B.heavy_flag, B.heavy_list, B.heavy_n);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    if (B.order_xcd) {
        hipLaunchKernelGGL(rtx_sched_xcd, dim3(1), dim3(kScanThreads), 0, s, B.order, B.order_xcd, P.n_tiles,
                           P.tiles_x, P.tiles_y);
        if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

int sched_update(rtx_ctx* c, const FrameArgs& F) {
    const uint32_t slots = (c->split_mode == 0 || !c->facts.split_ok) ? 0u
                           : (c->split_mode == 2 ? 0xffffffffu : c->split_slots);
    const int stage = c->heavy.cur ^ 1;
    // (throughput mode: at least kThroughputPermille, see rtx_ctx::ev_frame)
    const uint32_t permille = c->concurrent ? std::max<uint32_t>(c->tuner.permille, kThroughputPermille)
                                            : c->tuner.permille;
    c->heavy.permille[stage] = permille;
    c->sched_stage = stage;
    c->sched_params = {F.n_tiles, F.tiles_x, F.tiles_y, F.part_cost, slots, permille, c->split_min, c->split_slots};
    const SchedBufs B = {F.cost, F.heavy_flag, c->d_saved_cost, c->d_hist, c->d_csum, c->d_thr, c->d_order,
                         c->xcd_order ? c->d_order_xcd.get() : nullptr, c->d_heavy_flag[stage], c->d_heavy_list[stage],
                         c->d_heavy_n};
    HIP_TRY(c, sched_launch(c->stream, B, c->sched_params));
    HIP_TRY(c, hipMemcpyAsync(c->h_heavy_n, c->d_heavy_n, 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipEventRecord(c->ev_heavy, c->stream));
    c->heavy.pending = true;
    c->sched_ready = true;
    return RTX_OK;
}

}  // namespace rtxh
