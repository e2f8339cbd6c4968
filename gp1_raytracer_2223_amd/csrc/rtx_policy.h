// rtx_policy.h — the state of the frame policies of the render context (rtx_ctx.h), one struct per
// policy: its defaults, its transitions and its resets.  Plain C++17 and no HIP: the transitions are
// functions of their inputs (rtx_policy.hip and rtx_frame.hip make the HIP calls and pass the results
// in), so tests/policy_harness.cpp drives them on the CPU.  No pixel depends on any of it.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "rtx.h"

namespace rtxd {

// 1.5 (v14 sweep, tools/split_sweep.sh): Synthetic100k 4.38 -> 3.51 ms, W4_Optional within
// noise of 2.0; below 1.25 the split overhead outgrows the tail it removes
constexpr int kSplitPermille = 1500;
// In flight (rtx_ctx::concurrent) a split frame's extra work (the chain's repeated path walks, its
// launches) can cost more than its shorter critical path saves, since the other contexts' frames fill
// the GPU beside a long tile (2 frames in flight, profiles/r06/inflight_split_ab.txt: Bunny + 8 lights
// 4K share of 8 0.067 split / 0.059 ms one piece, W4_Optional share of 8 0.110 / 0.088, Synthetic100k
// share of 8 0.405 / 0.622).  Two frames in flight hide a tile as long as about two frames' time: a
// frame in flight renders one piece when its heaviest tile's one-piece cost (measured serialized) is
// below kInflightCritPermille / 1000 x the split frame's serialized span (the tuner's best, main
// kernel or chain), which holds for the first two and not for Synthetic100k (profiles/r06/
// inflight_crit_ab.txt).  RTX_INFLIGHT_CRIT=f sets the factor (0: split as serialized frames do).
constexpr uint32_t kInflightCritPermille = 1600;
// ... or when split frames in flight do not overlap: k frames in flight at once, their interval on a
// context's stream at least k x the serialized span / kInflightOverlapMin (timed over kInflightWindow
// frames after kInflightWindowSkip; W4_Optional's shares: the chain's work fills the GPU)
constexpr float kInflightOverlapMin = 1.15f;
constexpr uint32_t kInflightWindow = 32;
constexpr uint32_t kInflightWindowSkip = 16;
// Frontier refinement (rtx_kernels.h): rounds, parts cut per round, the share of the longest part
// wave that makes a part a candidate, and the frames a new shape or upload waits first
constexpr uint32_t kRefineRounds = 3;
constexpr uint32_t kRefineSplits = 8;
constexpr uint32_t kRefineTopPermille = 600;
constexpr uint32_t kRefineQuiet = 32;
constexpr int kPolicyMaxViews = 8;   // = kMaxViews (rtx_kernels.h; rtx_ctx.h asserts it)

}  // namespace rtxd

namespace rtxh {
using namespace rtxd;

// Split-threshold tuner: the frame is max(main kernel, split chain), and the
// threshold that balances the two is the fastest (Synthetic100k: factor 2.0, W4_Optional 1.5).
// A measured frame with split tiles times both (ev_tune: fork, main kernel end, chain end); at
// its adoption the factor the timed set was selected with moves toward the balance, by steps
// that shrink when the direction flips, until the two are within 4 % or the step is < 1.5 %.
struct SplitTuner {
    uint32_t permille = kSplitPermille;   // the factor, RTX_SPLIT_FACTOR (fixes it: no tuner)
    bool on = true;                       // RTX_SPLIT_TUNE=0 / RTX_SPLIT_FACTOR: off
    bool done = false;
    bool rec = false;                     // the measured frame in flight recorded ev_tune
    uint32_t rec_permille = 0;            // ... and the factor its (current) heavy set was selected with
    uint32_t steps = 0;
    int dir = 0;
    float step_size = 1.15f;
    float main_ms = 0.f, chain_ms = 0.f;  // the last timed frame (rtx_split_tune_info)
    float best_span = 0.f;                // the fastest max(main, chain) seen, and its factor
    uint32_t best_permille = 0;

    // One step: the timed frame rendered the heavy set selected with factor `base`; main = its main
    // kernel, chain = the split launches (both from the fork).  The next factor is a step away from
    // THAT factor (a set selected with an older factor is not evidence about the current one: it is
    // ignored, as are non-positive times), toward the balance of the two, clamped to 1000..4000.
    // The frame span max(main, chain) of every factor tried is kept: a step that makes it 5 % worse
    // than the best seen returns to the best and stops (a GPU that cannot run the chain beside the main
    // kernel — a profiler serialising dispatches, another process — would otherwise drift the factor).
    // Also done: the two within 4 %, more than 16 steps, or a step (its square root at every
    // change of direction) below 1.015.
    void step(uint32_t base, float main, float chain) {
        main_ms = main;
        chain_ms = chain;
        if (!base || main <= 0.f || chain <= 0.f) return;
        if (base != permille) return;   // a set from before the last step: wait for the current one
        const float span = std::max(main, chain);
        if (best_permille == 0 || span < best_span) {
            best_span = span;
            best_permille = base;
        } else if (span > 1.05f * best_span) {
            permille = best_permille;
            done = true;
            return;
        }
        const float r = chain / main;
        const int d = r > 1.04f ? 1 : (r < 0.96f ? -1 : 0);
        if (d == 0 || ++steps > 16) {
            done = true;
            return;
        }
        if (dir != 0 && d != dir) step_size = std::sqrt(step_size);   // overshot
        if (step_size < 1.015f) {
            done = true;
            return;
        }
        dir = d;
        const double f = static_cast<double>(base) * (d > 0 ? step_size : 1.0 / step_size);
        permille = static_cast<uint32_t>(std::min(4000.0, std::max(1000.0, f)));
    }
    // The two restarts share search(): a tuner that is on searches again (the steps, the direction,
    // the step size and the best span start over).  They differ in two fields:
    //  - a new launch shape starts from the default factor and drops the timing in flight (`rec`,
    //    also when the tuner is off: the events were recorded for another shape);
    //  - a shorter chain after a refinement round is balanced again from the factor it has, and the
    //    measured frame in flight, if any, still counts.
    void restart_default() {
        if (on) permille = kSplitPermille;
        search();
        rec = false;
    }
    void restart_here() { search(); }

private:
    void search() {
        if (!on) return;
        done = false;
        steps = 0; dir = 0; step_size = 1.15f;
        best_span = 0.f; best_permille = 0;
    }
};

// The split frames' interval in flight on this context's stream (kInflightWindow): state 0 skipping
// kInflightWindowSkip frames, 2 timing kInflightWindow frames, 3 waiting for the end event, 4 done.
struct InflightWindow {
    uint32_t state = 0, frames = 0;
    int rec = -1;              // the ev_win slot this frame's end records (-1 none)
    float interval_ms = 0.f;

    void reset() { state = 0; frames = 0; interval_ms = 0.f; }   // (`rec` is each frame's own)

    // Whether onepiece() with this threshold and ratio will ask for the end event (queried only then).
    bool wants_end(uint32_t crit, float ratio) const { return crit != 0 && !below(crit, ratio) && state == 3; }

    // Whether a frame in flight (k frames of this device's contexts at once) renders one piece: its
    // heaviest tile is short next to the split frame's serialized span (ratio = tile / span, 0 until
    // known, below crit / 1000), or the split frames in flight were measured not to overlap (their
    // interval ~ k x the serialized span `best_span`: the chain's work fills the GPU, so the frames
    // only queue).  The slot is cleared first; crit 0 and a ratio below crit return without advancing
    // the window.  end_ready: the end event has completed, elapsed_ms from the start event (0: unknown).
    bool onepiece(uint32_t crit, float ratio, uint32_t k, float best_span, bool end_ready, float elapsed_ms) {
        rec = -1;
        if (crit == 0) return false;
        if (below(crit, ratio)) return true;
        if (state == 4)   // measured: overlap = k x span / interval
            return best_span > 0.f && interval_ms > 0.f &&
                   static_cast<float>(k) * best_span < kInflightOverlapMin * interval_ms;
        if (state == 0 && ++frames >= kInflightWindowSkip) {
            state = 2;
            frames = 0;
            rec = 0;
        } else if (state == 2 && ++frames == kInflightWindow) {
            state = 3;
            rec = 1;
        } else if (state == 3 && end_ready) {
            if (elapsed_ms > 0.f) interval_ms = elapsed_ms / static_cast<float>(kInflightWindow);
            state = 4;
        }
        return false;
    }

private:
    static bool below(uint32_t crit, float ratio) { return ratio > 0.f && ratio * 1000.f < static_cast<float>(crit); }
};

// Frontier refinement (kRefineRounds): the round and state (0 waiting for a split frame, 1 measured
// frame queued, 2 done), frames to wait, the last round's longest part wave.
struct Refinement {
    bool off = false;                                // RTX_REFINE=0
    // RTX_REFINE_ROUNDS / _SPLITS / _TOP (permille): the kRefine* constants (tuning)
    uint32_t rounds = kRefineRounds, splits = kRefineSplits, top = kRefineTopPermille;
    uint32_t round = 0;
    int state = 2;
    uint32_t wait = 0, prev_max = 0;
    uint32_t quiet = 0;                              // frames of this shape still to wait
    bool rec = false;                                // this frame measures its parts (ev_refine at its end)

    // A new launch shape of a refinable scene: from round 0, after kRefineQuiet frames of the shape,
    // and no measurement in flight.
    void reset_shape() {
        reset_upload(true);
        rec = false;
        quiet = kRefineQuiet;
    }
    // An upload: from round 0 (done at once when the scene is not refinable).  `rec` and `quiet` are
    // left as they are (the upload's own quiet time is rtx_ctx::renders_since_upload).
    void reset_upload(bool refinable) {
        round = 0; wait = 0; prev_max = 0;
        state = refinable ? 0 : 2;
    }
};

// Deferred join (rtx_policy.hip, join_split): the last frame's split chain has not been joined into
// the frame stream (`pending`); the next frame's main kernel may start beside it when it repeats the
// frame exactly (same parameters, cameras, scene image and heavy set: the two write disjoint tiles) —
// anything else joins first.  The other members: that frame's identity.
struct DeferredJoin {
    bool pending = false;
    bool off = false;                           // RTX_DEFER_JOIN=0
    rtx_render_params p{};
    rtx_camera cams[kPolicyMaxViews]{};
    int views = 0, sb = -1;
    uint64_t gen = 0;
    uint32_t ss = 0;
    const uint32_t* heavy = nullptr;
    uint32_t heavy_n = 0;

    bool same_frame(const rtx_render_params& q, const rtx_camera* c, int n, uint64_t g, int b, uint32_t s) const {
        return n == views && g == gen && b == sb && s == ss && std::memcmp(&q, &p, sizeof p) == 0 &&
               std::memcmp(c, cams, sizeof(rtx_camera) * static_cast<size_t>(n)) == 0;
    }
    void note(const rtx_render_params& q, const rtx_camera* c, int n, uint64_t g, int b, uint32_t s) {
        p = q;
        std::memcpy(cams, c, sizeof(rtx_camera) * static_cast<size_t>(n));
        views = n; gen = g; sb = b; ss = s;
    }
};

// Motion mode (kMotionFrames): frames left, and the previous frame's cameras it compares.
struct Motion {
    uint32_t left = 0;
    bool off = false;                           // RTX_MOTION=0: always the static schedule (A/B)
    // An upload in the animated pattern (the previous upload was rendered at most once too) moves the
    // geometry under a fixed tile schedule as a moving camera does: the next frame starts motion
    // mode when the scene has split tiles (prepare; RTX_MOTION=0 turns both off).
    bool upload_motion = false;
    int prev_views = 0;
    rtx_camera prev_cam[kPolicyMaxViews] = {};

    // Whether a camera differs from the previous frame's (any field; the view count too), and these
    // become the previous ones.
    bool moved(const rtx_camera* cams, int n) {
        bool m = prev_views != n;
        for (int v = 0; !m && v < n; ++v)
            m = std::memcmp(&cams[v], &prev_cam[v], offsetof(rtx_camera, fov)) || cams[v].fov != prev_cam[v].fov;
        std::memcpy(prev_cam, cams, sizeof(rtx_camera) * static_cast<size_t>(n));
        prev_views = n;
        return m;
    }
};

// The heavy tiles' double-buffered flag / list sets: the reorder kernel fills the staging set; the
// host adopts it (`cur`), with its count, at the next frame.
struct HeavySet {
    int cur = 0;
    uint32_t n = 0;
    bool pending = false;
    uint32_t permille[2] = {0, 0};              // per set: the factor the schedule selected it with
};

}  // namespace rtxh
