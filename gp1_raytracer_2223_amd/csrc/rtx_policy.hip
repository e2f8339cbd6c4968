// rtx_policy.hip — the frame policies of the render context (rtx_ctx.h): which tiles a frame splits
// and how (the split tuner, throughput mode and the in-flight one-piece choice), the frontier
// refinement, and when the split chain joins the frame stream.  Host code only; no pixel depends on
// any of it (every choice renders the reference's frame).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "rtx_ctx.h"

namespace rtxh {

namespace {
// The process's contexts that have queued a frame (rtx_ctx::ev_frame), for throughput mode.
std::mutex g_frames_m;
std::vector<rtx_ctx*> g_frames;

}  // namespace

// The other contexts on c's device with a frame still in flight (their ev_frame not reached).
uint32_t frames_concurrent(rtx_ctx* c) {
    std::lock_guard<std::mutex> l(g_frames_m);
    uint32_t n = 0;
    for (rtx_ctx* o : g_frames) {
        if (o == c || o->device != c->device) continue;
        const hipError_t q = hipEventQuery(o->ev_frame);
        if (q == hipErrorNotReady) {
            (void)hipGetLastError();   // (not-ready is no error for the caller's checks)
            ++n;
        }
    }
    return n;
}
void frames_note(rtx_ctx* c) {
    std::lock_guard<std::mutex> l(g_frames_m);
    if (std::find(g_frames.begin(), g_frames.end(), c) == g_frames.end()) g_frames.push_back(c);
}
void frames_forget(rtx_ctx* c) {
    std::lock_guard<std::mutex> l(g_frames_m);
    g_frames.erase(std::remove(g_frames.begin(), g_frames.end(), c), g_frames.end());
}

// Join the last frame's split chain into the frame stream (rtx_ctx::join) before anything
// that reads its pixels, reallocates or rewrites what it reads, or needs the frame complete.
int join_split(rtx_ctx* c) {
    if (!c->join.pending) return RTX_OK;
    c->join.pending = false;
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
    return RTX_OK;
}

// One round of the frontier refinement (kRefineRounds), once the measured frame has completed
// (rtx_ctx::ev_refine; not waited for): per part the longest closest-hit wave plus the longest
// shadow wave; the parts within kRefineTopPermille of the longest are replaced by their two
// children (inner nodes only; the order of the frontier kept), and the new frontier is copied into
// the image's parts section on the frame stream, behind every frame already queued.  The context's
// frontier (h_parts, dev.n_parts) changes only once the device holds the new one.
int refine_round(rtx_ctx* c) {
    rtxh::Refinement& R = c->refine;
    const hipError_t q = hipEventQuery(c->ev_refine);
    (void)hipGetLastError();   // (not-ready is no error for the caller's checks)
    if (q == hipErrorNotReady) return RTX_OK;
    HIP_TRY(c, q);
    HIP_TRY(c, hipMemcpy(c->h_part_max.data(), c->d_part_max, c->h_part_max.size() * sizeof(uint32_t),
                         hipMemcpyDeviceToHost));
    const size_t np = c->h_parts.size();
    std::vector<uint64_t> m(np, 0);
    uint64_t top = 0;
    for (size_t p = 0; p < np; ++p) {
        uint32_t a = 0, b = 0;
        for (int k = 0; k < kPartShards; ++k) {
            a = std::max(a, c->h_part_max[(0 * kMaxParts + p) * kPartShards + k]);
            b = std::max(b, c->h_part_max[(1 * kMaxParts + p) * kPartShards + k]);
        }
        m[p] = static_cast<uint64_t>(a) + b;
        top = std::max(top, m[p]);
    }
    ++R.round;
    // done: nothing measured, the last round gained under 10 %, or the rounds are spent
    const bool gained = R.prev_max == 0 || top * 10 < static_cast<uint64_t>(R.prev_max) * 9;
    R.prev_max = static_cast<uint32_t>(std::min<uint64_t>(top, 0xffffffffull));
    R.state = 2;
    if (top * kSplitMinUs < static_cast<uint64_t>(kRefineMinUs) * kSplitMinCost || !gained) return RTX_OK;
    // only a chain whose longest waves outlast the main kernel by kRefineOverMain: with less, the
    // frame is bound by its work (more parts only add waves; frames in flight lose throughput)
    const double top_ms = static_cast<double>(top) * kSplitMinUs / kSplitMinCost * 1e-3;
    if (c->tuner.main_ms > 0.f && top_ms * 1000.0 < static_cast<double>(kRefineOverMainPermille) * c->tuner.main_ms)
        return RTX_OK;
    std::vector<size_t> cand;
    for (size_t p = 0; p < np; ++p)
        if (c->h_parts[p].x >= 0 && m[p] * 1000 >= top * R.top && c->h_parts[p].w < 31) cand.push_back(p);
    std::sort(cand.begin(), cand.end(), [&](size_t x, size_t y) { return m[x] > m[y]; });
    if (cand.size() > R.splits) cand.resize(R.splits);
    std::vector<int> left(np, -1);   // per part that is cut: its left child's node slot
    size_t n_new = np;
    for (size_t p : cand) {
        // the part's node record (copy 0 of the node array): children only under an inner node
        float4 rec[2];
        HIP_TRY(c, hipMemcpy(rec, c->dev.nodes + 2ull * static_cast<uint32_t>(c->h_parts[p].y), sizeof rec,
                             hipMemcpyDeviceToHost));
        uint32_t link, ntri;
        std::memcpy(&link, &rec[1].z, 4);
        std::memcpy(&ntri, &rec[1].w, 4);
        if (ntri != 0 || n_new + 1 > static_cast<size_t>(kMaxParts)) continue;
        ++n_new;
        // (device layout: an inner node's link is its child pair's byte offset, 32 B a slot)
        left[p] = static_cast<int>(link / 32u);   // the right child is the next slot
    }
    if (n_new == np) return RTX_OK;
    std::vector<int4> fr;
    fr.reserve(n_new);
    for (size_t p = 0; p < np; ++p) {
        const int4 e = c->h_parts[p];
        if (left[p] < 0) {
            fr.push_back(e);
            continue;
        }
        fr.push_back(make_int4(e.x, left[p], e.z, e.w + 1));
        fr.push_back(make_int4(e.x, left[p] + 1, e.z | (1 << e.w), e.w + 1));
    }
    if (const int rc = join_split(c); rc != RTX_OK) return rc;   // (the chain may still read the parts)
    HIP_TRY(c, hipMemcpyAsync(c->parts_dev, fr.data(), fr.size() * sizeof(int4), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // (`fr` is pageable: the copy has read it)
    c->h_parts.swap(fr);
    c->dev.n_parts = static_cast<uint32_t>(c->h_parts.size());
    // a shorter chain: the split factor is balanced again from where it is, and frames in flight are
    // timed again (the window only with the tuner on)
    if (c->tuner.on) c->window.reset();
    c->tuner.restart_here();
    if (R.round < R.rounds) {
        R.state = 0;
        R.wait = 8;   // frames of the new frontier before it is measured
    }
    return RTX_OK;
}

// Whether a frame in flight (k frames of this device's contexts at once) renders one piece:
// InflightWindow::onepiece makes the choice; the window's end event is asked here, when it waits for it.
bool inflight_onepiece(rtx_ctx* c, uint32_t k) {
    const float r = inflight_ratio(c);
    bool ready = false;
    float ms = 0.f;
    if (c->window.wants_end(c->inflight_crit, r)) {
        ready = hipEventQuery(c->ev_win[1]) == hipSuccess;
        (void)hipGetLastError();   // (not-ready is no error for the caller's checks)
        if (ready) {
            if (hipEventElapsedTime(&ms, c->ev_win[0], c->ev_win[1]) != hipSuccess) ms = 0.f;
            (void)hipGetLastError();
        }
    }
    return c->window.onepiece(c->inflight_crit, r, k, c->tuner.best_span, ready, ms);
}
float inflight_ratio(const rtx_ctx* c) {
    if (c->max_cost_serial == 0 || c->tuner.best_span <= 0.f) return 0.f;
    const float tile_ms = static_cast<float>(c->max_cost_serial) * static_cast<float>(kSplitMinUs) /
                          static_cast<float>(kSplitMinCost) * 1e-3f;
    return tile_ms / c->tuner.best_span;
}

}  // namespace rtxh
