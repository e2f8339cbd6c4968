// rtx_frame.hip — a colour frame behind the C-ABI of include/rtx.h: its checks, buffers and schedule
// state (prepare), its launches (launch: the split chain, the main kernel, the schedule update), and
// the render, synchronise, download, gather and host-register entry points.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "rtx_ctx.h"
#include "rtx_launch.h"
#include "rtx_variants.h"

using namespace rtxh;

namespace rtxh {

// Index into kSpecVariants of the first variant the facts satisfy, -1 for none: every kind the
// scene references is compiled into the variant, and every other fact the variant assumes holds.
int spec_variant(int facts) {
    for (int i = 0; i < static_cast<int>(sizeof kSpecVariants / sizeof kSpecVariants[0]); ++i) {
        const int v = kSpecVariants[i], vk = v & kSpecKindAll, fk = facts & kSpecKindAll;
        if ((fk & ~vk) == 0 && ((v & ~kSpecKindAll) & ~facts) == 0) return i;
    }
    return -1;
}

// The launch record of a frame of `n_views` cameras: the cameras (with their cull bounds and room-plane
// numerators), the frame `sp` the kernel renders (the sample frame of a supersampled one, `p` otherwise),
// its owned wave tiles and the launch grid.  Everything a colour frame and the hit pass share; the
// outputs and the schedule are the caller's.
void frame_shape(rtx_ctx* c, const rtx_camera* cams, int n_views, const rtx_render_params* p,
                 const rtx_render_params& sp, uint32_t ss, FrameArgs& F, dim3& grid) {
    const bool striped = p->stripe_rows != 0 && p->stripe_step > 1;
    std::memset(&F, 0, sizeof F);
    for (int v = 0; v < n_views; ++v) {
        for (int k = 0; k < 3; ++k) {
            F.cam[v].origin[k] = cams[v].origin[k]; F.cam[v].right[k] = cams[v].right[k];
            F.cam[v].up[k] = cams[v].up[k]; F.cam[v].forward[k] = cams[v].forward[k];
        }
        F.cam[v].fov = cams[v].fov;
        // the camera anchor's t bound (CullRay::bt): 4x the farthest corner of the meshes' box + 1
        if (c->dev.cull_stride) {
            double R = 0.0;
            for (int k = 0; k < 8; ++k) {
                const double dx = cams[v].origin[0] - ((k & 1) ? c->cull_bmax[0] : c->cull_bmin[0]);
                const double dy = cams[v].origin[1] - ((k & 2) ? c->cull_bmax[1] : c->cull_bmin[1]);
                const double dz = cams[v].origin[2] - ((k & 4) ? c->cull_bmax[2] : c->cull_bmin[2]);
                R = std::fmax(R, std::sqrt(dx * dx + dy * dy + dz * dz));
            }
            const double bt = 4.0 * R + 1.0;
            F.cam[v].cull_bt = std::isfinite(bt) && bt < 0x1p60 ? static_cast<float>(bt) : 0.f;   // 0: no pruning
        }
        if (c->facts.spec & kSpecRoomPlanes) {   // the room planes' camera numerators (ViewCam)
            bool ok = true;
            for (int k = 0; k < 5; ++k) {
                const float a = c->facts.room_p0[k] - cams[v].origin[kRoomAxes[k]];
                const float aa = std::fabs(a);
                F.cam[v].room_a[k] = a;
                ok = ok && (a == 0.f || (aa >= 0x1p-60f && aa <= 0x1p60f));
            }
            F.cam[v].room_fast = ok ? 1u : 0u;
        }
    }
    F.n_views = static_cast<uint32_t>(n_views);
    F.aspect = static_cast<int>(sp.width) / static_cast<float>(static_cast<int>(sp.height));  // Renderer.cpp:30
    F.inv_width = 1.f / static_cast<float>(static_cast<int>(sp.width));
    F.inv_height = 1.f / static_cast<float>(static_cast<int>(sp.height));
    F.width = sp.width; F.height = sp.height;
    F.ss_log2 = ss; F.out_width = p->width; F.out_height = p->height;
    F.mode = p->lighting_mode; F.shadows = p->shadows_enabled ? 1 : 0;
    F.rshift = p->format.rshift; F.gshift = p->format.gshift; F.bshift = p->format.bshift; F.amask = p->format.amask;
    const uint32_t groups = (sp.height + kWaveTile - 1) / kWaveTile;
    uint32_t gy = groups;
    if (striped) {
        // every view owns the same number of stripes only if the stripe count divides
        // evenly; size the grid for the largest owner and let the kernel skip the rest
        const uint32_t gps = sp.stripe_rows / kWaveTile;
        const uint32_t nstripes = (groups + gps - 1) / gps;
        const uint32_t owned = (nstripes + p->stripe_step - 1) / p->stripe_step;
        F.groups_per_stripe = gps; F.stripe_first = p->stripe_first; F.stripe_step = p->stripe_step;
        gy = owned * gps;
    }
    F.tiles_x = (sp.width + kWaveTile - 1) / kWaveTile;
    F.tiles_y = gy;
    const uint32_t ntiles = F.tiles_x * gy * static_cast<uint32_t>(n_views);
    F.n_tiles = ntiles;
    const uint32_t nblocks = (ntiles + kWavesPerBlock - 1) / kWavesPerBlock;
    grid = dim3(nblocks, 1, 1);
}

// The head of a launch shape's key (rtx_ctx::sched_key): the launches that share it have the same wave
// tiles, so one's dispatch order is a permutation of the other's.
std::string tiles_key(uint32_t width, uint32_t height, int n_views, uint32_t stripe_rows, uint32_t stripe_first,
                      uint32_t stripe_step) {
    return std::to_string(width) + "x" + std::to_string(height) + "v" + std::to_string(n_views) + "s" +
           std::to_string(stripe_rows) + "/" + std::to_string(stripe_first) + "/" + std::to_string(stripe_step) + "g";
}

// ---- prepare's steps, in its order --------------------------------------------------------------
// (the first one is an adaptive frame's too, rtx_adaptive.hip)
int check_params(rtx_ctx* c, const rtx_camera* cams, int n_views, const rtx_render_params* p) {
    if (!c || !cams || !p) return RTX_E_INVALID;
    if (n_views < 1 || n_views > kMaxViews) return fail(c, RTX_E_INVALID, "n_views must be 1..8");
    if (!c->has_scene) return fail(c, RTX_E_STATE, "no scene uploaded");
    if (p->width == 0 || p->height == 0 || p->width > 65536 || p->height > 65536)
        return fail(c, RTX_E_INVALID, "bad image size");
    if (p->lighting_mode < 0 || p->lighting_mode >= RTX_MODE_COUNT) return fail(c, RTX_E_INVALID, "bad lighting mode");
    if (p->format.rshift > 24 || p->format.gshift > 24 || p->format.bshift > 24)
        return fail(c, RTX_E_INVALID, "bad pixel format");
    const bool striped = p->stripe_rows != 0 && p->stripe_step > 1;
    if (striped && (p->stripe_rows % 16 != 0 || p->stripe_first >= p->stripe_step))
        return fail(c, RTX_E_INVALID, "stripe_rows must be a multiple of 16 and stripe_first < stripe_step");
    // the sample frame's sides stay inside div_rn's divisor domain like a plain frame's
    const uint32_t ss = c->ss_log2;
    if ((static_cast<uint64_t>(p->width) << ss) > 65536 || (static_cast<uint64_t>(p->height) << ss) > 65536)
        return fail(c, RTX_E_INVALID, "bad image size: supersampled " + std::to_string(1u << ss) + "x" +
                                          std::to_string(1u << ss) + ", the sample frame exceeds 65536 per side");
    return RTX_OK;
}

// The frame buffer (and the colour plane when asked for) of npx pixels.
int frame_buffers(rtx_ctx* c, size_t npx, bool want_rgb) {
    if (npx > c->d_px.cap) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (const int rc = c->d_px.grow(c, npx); rc != RTX_OK) return rc;
    }
    if (want_rgb && npx > c->d_rgb.cap) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (const int rc = c->d_rgb.grow(c, npx, 12); rc != RTX_OK) return rc;
    }
    return RTX_OK;
}

namespace {

// Cost-ordered dispatch (see the kernel): one order/cost pair per launch shape, for ntiles tiles.
int sched_buffers(rtx_ctx* c, uint32_t ntiles) {
    if (ntiles <= c->sched_cap) return RTX_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->sched_cap = 0;
    const size_t nch = (ntiles + kSchedChunk - 1) / kSchedChunk;
    int rc = c->d_order.grow(c, ntiles);
    c->d_order_xcd.free();
    if (rc == RTX_OK && c->xcd_order) rc = c->d_order_xcd.grow(c, ntiles);
    if (rc == RTX_OK) rc = c->d_cost.grow(c, ntiles);
    for (auto& f : c->d_heavy_flag)
        if (rc == RTX_OK) rc = f.grow(c, ntiles);
    if (rc == RTX_OK) rc = c->d_saved_cost.grow(c, ntiles);
    if (rc == RTX_OK) rc = c->d_hist.grow(c, nch * kCostBuckets);
    if (rc == RTX_OK) rc = c->d_csum.grow(c, nch);
    if (rc != RTX_OK) return rc;
    c->sched_cap = ntiles;
    c->sched_key.clear();
    return RTX_OK;
}

// A new launch shape or scene: identity order, fresh costs, no split, and every policy from its start.
int new_shape(rtx_ctx* c, const std::string& key, uint32_t ntiles) {
    if (c->heavy.pending) HIP_TRY(c, hipEventSynchronize(c->ev_heavy));
    c->heavy.pending = false;
    c->heavy.n = 0;
    c->sched_key = key;
    c->sched_ready = false;
    c->sched_frame = 0;
    c->motion.left = 0;
    c->max_cost_serial = 0;
    if (c->refinable) {   // a new shape refines from the upload's frontier
        if (c->h_parts.size() != c->h_parts_base.size()) {
            if (const int rc = join_split(c); rc != RTX_OK) return rc;
            c->h_parts = c->h_parts_base;
            HIP_TRY(c, hipMemcpyAsync(c->parts_dev, c->h_parts.data(), c->h_parts.size() * sizeof(int4),
                                      hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            c->dev.n_parts = static_cast<uint32_t>(c->h_parts.size());
        }
        c->refine.reset_shape();
    }
    c->window.reset();
    c->tuner.restart_default();   // tune again from the default
    HIP_TRY(c, hipMemsetAsync(c->d_cost, 0, ntiles * 4, c->stream));
    return RTX_OK;
}

// Adopt the heavy set the last measured frame selected, and step the tuner with that frame's timings.
int adopt_heavy(rtx_ctx* c, bool motion) {
    if (!c->heavy.pending) return RTX_OK;
    if (motion) {   // no host wait: adopt only a measurement that has completed
        const hipError_t q = hipEventQuery(c->ev_heavy);
        (void)hipGetLastError();   // (a not-ready query is no error for the launches' checks)
        if (q != hipSuccess && q != hipErrorNotReady) HIP_TRY(c, q);
        if (q != hipSuccess) return RTX_OK;
    } else {
        HIP_TRY(c, hipEventSynchronize(c->ev_heavy));   // (one sync per measurement)
    }
    c->heavy.pending = false;
    c->heavy.n = std::min<uint32_t>(c->h_heavy_n[0], kMaxHeavyTiles);
    if (!c->concurrent) c->max_cost_serial = c->h_heavy_n[2];
    c->heavy.cur ^= 1;
    // nothing to balance while no tile is heavy at the default factor (the tuner only
    // raises the factor from there when the split chain is the longer)
    if (c->heavy.n == 0 && c->tuner.permille == kSplitPermille && c->heavy.permille[c->heavy.cur] == kSplitPermille)
        c->tuner.done = true;
    if (c->tuner.rec) {   // the measured frame's timings: complete (they precede ev_heavy)
        c->tuner.rec = false;
        float mm = 0.f, ch = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&mm, c->ev_tune[0], c->ev_tune[1]));
        HIP_TRY(c, hipEventElapsedTime(&ch, c->ev_tune[0], c->ev_tune[2]));
        c->tuner.step(c->tuner.rec_permille, mm, ch);
    }
    return RTX_OK;
}

// Whether the frame renders its heavy tiles split: throughput mode and the in-flight one-piece rule.
bool choose_split(rtx_ctx* c) {
    // throughput mode: other contexts' frames in flight on this device (rtx_ctx::ev_frame; asked only
    // where a tile can be split: the other contexts' event queries are not free in a GPU-bound loop)
    const uint32_t others = (!c->throughput_off && c->tuner.on && c->facts.split_ok && (c->heavy.n > 0 || !c->tuner.done))
                                ? frames_concurrent(c) : 0u;
    c->concurrent = others > 0;
    // in flight: one piece while the heaviest tile is short next to the split frame (kInflightCritPermille)
    c->frame_onepiece = c->concurrent && c->heavy.n > 0 && inflight_onepiece(c, others + 1);
    return c->split_mode != 0 && c->facts.split_ok && c->sched_enabled && c->heavy.n > 0 && !c->frame_onepiece;
}

// The frontier refinement: a completed measurement's round, then whether this frame measures its parts.
int arm_refinement(rtx_ctx* c, FrameArgs& F, bool split, bool motion) {
    rtxh::Refinement& R = c->refine;
    if (R.state == 1)
        if (const int rc = refine_round(c); rc != RTX_OK) return rc;
    if (R.quiet) --R.quiet;
    if (split && R.state == 0 && !motion && c->renders_since_upload >= kRefineQuiet && R.quiet == 0 &&
        (R.wait == 0 || --R.wait == 0)) {
        constexpr size_t kWords = 2ull * kMaxParts * kPartShards;
        if (!c->d_part_max) {
            if (const int rc = c->d_part_max.grow(c, kWords); rc != RTX_OK) return rc;
            c->h_part_max.resize(kWords);
        }
        HIP_TRY(c, hipMemsetAsync(c->d_part_max, 0, kWords * sizeof(uint32_t), c->stream));
        F.part_max = c->d_part_max;
        R.rec = true;
    }
    return RTX_OK;
}

// light-major (FrameArgs::lm_*): a launch small enough that its slowest tiles, not its work, set
// its time (a few tiles per resident wave slot: a stripe share of a frame), with shadows and 2+
// lights; the deep-stack variants render one piece
int choose_light_major(rtx_ctx* c, FrameArgs& F) {
    const uint32_t nl = c->dev.n_lights, ntiles = F.n_tiles;
    c->frame_lm = F.shadows && nl >= 2 && nl <= kMaxLmLights && !c->facts.deep_stack && !c->facts.hbm_stack &&
                  (c->lm_mode == 2 || (c->lm_mode == 1 && ntiles <= c->lm_tiles));
    if (!c->frame_lm) return RTX_OK;
    if (ntiles > c->d_lm_rec.cap) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (const int rc = c->d_lm_rec.grow(c, ntiles, 64 * 2 * sizeof(float4)); rc != RTX_OK) return rc;
    }
    if (static_cast<size_t>(ntiles) * nl > c->d_lm_mask.cap) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (const int rc = c->d_lm_mask.grow(c, static_cast<size_t>(ntiles) * nl); rc != RTX_OK) return rc;
    }
    F.lm_lights = nl;
    F.lm_rec = c->d_lm_rec;
    F.lm_mask = c->d_lm_mask;
    return RTX_OK;
}

// Measure tile costs on the first frame of a shape and then every kSchedPeriod frames;
// the frames in between reuse the last order and pay nothing for scheduling.
// while the split threshold is being tuned (a scene with split tiles), every other frame is measured
void choose_measure(rtx_ctx* c, FrameArgs& F, bool motion) {
    const bool tuning = c->tuner.on && !c->tuner.done && c->heavy.n > 0 && c->split_mode == 1 && c->facts.split_ok && !motion &&
                        !c->concurrent;
    const bool measure = c->sched_enabled && !c->heavy.pending &&
                         (!c->sched_ready || motion || c->sched_frame % (tuning ? 2u : c->sched_period) == 0);
    ++c->sched_frame;
    F.order = (c->sched_enabled && c->sched_ready) ? (c->xcd_order ? c->d_order_xcd : c->d_order).get() : nullptr;
    F.cost = measure ? c->d_cost.get() : nullptr;
    F.part_cost = (measure && motion) ? 1u : 0u;
}

}  // namespace

int prepare(rtx_ctx* c, const rtx_camera* cams, int n_views, const rtx_render_params* p, bool want_rgb, FrameArgs& F,
            dim3& grid) {
    if (const int rc = check_params(c, cams, n_views, p); rc != RTX_OK) return rc;
    // Supersampling (rtx_set_supersample): the launch renders the k*width x k*height sample frame `sp`
    // (the reference's frame of that size; stripes stay output rows, k*stripe_rows sample rows: whole
    // wave-tile rows) and resolves it into the width x height frame buffer.
    const uint32_t ss = c->ss_log2;
    rtx_render_params sp = *p;
    sp.width <<= ss; sp.height <<= ss; sp.stripe_rows <<= ss;
    const size_t npx = static_cast<size_t>(p->width) * p->height * static_cast<size_t>(n_views);
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->join.pending && !c->join.same_frame(*p, cams, n_views, c->scene_gen, c->sb_cur, ss))
        if (const int rc = join_split(c); rc != RTX_OK) return rc;
    c->join.note(*p, cams, n_views, c->scene_gen, c->sb_cur, ss);   // this frame's identity, for the next frame's test
    if (const int rc = frame_buffers(c, npx, want_rgb); rc != RTX_OK) return rc;
    frame_shape(c, cams, n_views, p, sp, ss, F, grid);
    F.out_px = c->d_px;
    F.out_rgb = want_rgb ? c->d_rgb.get() : nullptr;
    F.counters = c->d_counters;
    if (const int rc = sched_buffers(c, F.n_tiles); rc != RTX_OK) return rc;
    const std::string key = tiles_key(sp.width, sp.height, n_views, sp.stripe_rows, p->stripe_first, p->stripe_step) +
                            c->facts.sig + "m" + std::to_string(p->lighting_mode) + std::to_string(p->shadows_enabled) +
                            "k" + std::to_string(ss);
    // Motion mode: a camera differs from the previous frame's (any field), so the tile costs go
    // stale quickly.  For kMotionFrames frames from then on, every frame is measured whose previous
    // measurement has completed (adopted without waiting), and split tiles are costed by their
    // split waves (FrameArgs::part_cost).  Otherwise: one measurement every sched_period frames,
    // adopted at the next frame (one host wait per measurement).
    // Animated geometry (Motion::upload_motion) counts where a stale schedule costs: a scene with split
    // tiles (W4_Optional's F6 loop: GPU wait 0.51 -> 0.43 ms).  Without them the per-frame
    // measurement is the larger cost (W4_Bunny's loop 7-10 % slower, W4_Reference's serial 11 %).
    const bool moved = c->motion.moved(cams, n_views) || (c->motion.upload_motion && c->heavy.n > 0);
    c->motion.upload_motion = false;
    if (key != c->sched_key) {
        if (const int rc = new_shape(c, key, F.n_tiles); rc != RTX_OK) return rc;
    } else if (moved && !c->motion.off) {
        c->motion.left = kMotionFrames;
    }
    const bool motion = c->motion.left > 0;
    if (motion) --c->motion.left;
    c->frame_motion = motion;
    if (const int rc = adopt_heavy(c, motion); rc != RTX_OK) return rc;
    const bool split = choose_split(c);
    F.heavy_flag = split ? c->d_heavy_flag[c->heavy.cur].get() : nullptr;
    F.part_max = nullptr;
    if (const int rc = arm_refinement(c, F, split, motion); rc != RTX_OK) return rc;
    F.heavy_list = c->d_heavy_list[c->heavy.cur];
    F.heavy_n = split ? c->heavy.n : 0u;
    F.hit_key = c->d_hit_key;
    F.occ_bits = c->d_occ;
    if (const int rc = choose_light_major(c, F); rc != RTX_OK) return rc;
    choose_measure(c, F, motion);
    return RTX_OK;
}

// The HBM stacks of the HSTK variant: max_depth + 1 entries for each wave of a launch of
// `groups` workgroups (sized per launch: a wave's index in it selects its stack).
int ensure_hbm_stacks(rtx_ctx* c, uint32_t groups) {
    const size_t depth = static_cast<size_t>(c->facts.max_depth) + 1u;
    const size_t need = static_cast<size_t>(groups) * kWavesPerBlock * depth;
    constexpr size_t kEntryBytes = sizeof(uint4) + sizeof(unsigned long long);
    if (need * kEntryBytes > (size_t(64) << 30))
        return fail(c, RTX_E_UNSUPPORTED, "DFS stacks of a " + std::to_string(c->facts.max_depth) + "-level BVH for this frame exceed 64 GB");
    if (need > c->d_hstkT.cap) {   // (the one grown last: both hold `need` or this runs again)
        c->d_hstkT.free();
        if (const int rc = c->d_hstk.grow(c, need); rc != RTX_OK) return rc;
        if (const int rc = c->d_hstkT.grow(c, need); rc != RTX_OK) return rc;
    }
    c->dev.hstk = c->d_hstk;
    c->dev.hstkT = c->d_hstkT;
    c->dev.hstk_depth = static_cast<uint32_t>(depth);
    return RTX_OK;
}

namespace {

// ---- launch's steps -----------------------------------------------------------------------------
// The heavy tiles, one BVH frontier part per workgroup (see the kernel), on a high-priority stream
// forked from the frame stream: they share no pixels with the main kernel, so the two run side by
// side and the join closes the frame.
int launch_chain(rtx_ctx* c, const FrameArgs& F, int v) {
    const uint32_t nh = (c->heavy.n + kWavesPerBlock - 1) / kWavesPerBlock, np = c->dev.n_parts;   // heavy wave tiles per workgroup
    hipStream_t s2 = c->split_stream;
    // the tuner's timings: static cameras only (a moving one changes the frame under the measurement)
    const bool timed = F.cost && c->tuner.on && !c->tuner.done && c->split_mode == 1 && !c->frame_motion && !c->concurrent;
    if (timed) HIP_TRY(c, hipEventRecord(c->ev_tune[0], c->stream));
    HIP_TRY(c, hipEventRecord(c->ev_fork, c->stream));
    HIP_TRY(c, hipStreamWaitEvent(s2, c->ev_fork, 0));
    if (!RTX_ABL_CHAIN) {
        launch_render_phase(1, v, dim3(nh, np, 1), s2, c->dev, F);
        HIP_TRY(c, hipGetLastError());
        if (F.shadows && c->dev.n_lights) {
            launch_render_phase(2, v, dim3(nh, np, c->dev.n_lights), s2, c->dev, F);
            HIP_TRY(c, hipGetLastError());
        }
        launch_render_phase(3, v, dim3(nh, 1, 1), s2, c->dev, F);
        HIP_TRY(c, hipGetLastError());
    }
    if (timed) {   // (before ev_join: the frame's completion then implies this event's)
        HIP_TRY(c, hipEventRecord(c->ev_tune[2], s2));
        c->tuner.rec = true;
        c->tuner.rec_permille = c->heavy.permille[c->heavy.cur];
    }
    HIP_TRY(c, hipEventRecord(c->ev_join, s2));
    return RTX_OK;
}

// The frame's own launch on the frame stream: one kernel, or the light-major three.
int launch_main(rtx_ctx* c, const FrameArgs& F, dim3 grid, int v) {
    if (c->facts.deep_stack)   // (the deep variants walk without the cull; hbm_stack is a deep stack too)
        launch_render_one(false, true, c->facts.hbm_stack, false, grid, c->stream, c->dev, F);
    else if (F.lm_lights) {   // light-major: hit records, then the (tile, light) waves
        launch_render_phase(4, v, grid, c->stream, c->dev, F);
        HIP_TRY(c, hipGetLastError());
        // persistent light waves: one per resident wave slot (at most one per item)
        const uint32_t items = F.n_tiles * F.lm_lights, waves = std::min(items, c->lm_waves);
        launch_render_phase(5, v, dim3((waves + kWavesPerBlock - 1) / kWavesPerBlock), c->stream, c->dev, F);
        HIP_TRY(c, hipGetLastError());
        launch_render_phase(6, v, grid, c->stream, c->dev, F);
    } else if (!(RTX_ABL_MAIN && F.heavy_flag && !F.cost))
        launch_render_phase(0, v, grid, c->stream, c->dev, F);
    HIP_TRY(c, hipGetLastError());
    return RTX_OK;
}

// The instrumented variants (count: 1 = the reference's traversal counted, 2 = the culled walk's
// executed tests, rtx_count_work_culled; the plain one without records).
int launch_counting(rtx_ctx* c, const FrameArgs& F, dim3 grid, int count) {
    FrameArgs G = F;   // the instrumented variant neither reads nor feeds the schedule
    G.order = nullptr;
    G.cost = nullptr;
    G.heavy_flag = nullptr;
    const bool culled = count == 2 && c->dev.cull_stride && !c->facts.deep_stack;   // (hbm_stack is a deep stack too)
    if (culled)   // the views' camera records, as a frame would
        if (const int rc = cull_views(c, F); rc != RTX_OK) return rc;
    launch_render_one(true, c->facts.deep_stack, c->facts.hbm_stack, culled, grid, c->stream, c->dev, G);
    HIP_TRY(c, hipGetLastError());
    return RTX_OK;
}

// The events at the frame's end: the in-flight window's, the refinement's, and the frame's own.
int end_frame(rtx_ctx* c) {
    // the frame's end, for other contexts' throughput mode (prepare).  Only a context whose tiles can
    // be split records it: one that has nothing to split (no frontier, or no heavy tile at a converged
    // factor: W4_Bunny) skips the event and the registry's lock on every frame.
    const bool tracked = c->facts.split_ok && c->split_mode != 0 && !(c->heavy.n == 0 && c->tuner.done);
    if (c->window.rec >= 0) HIP_TRY(c, hipEventRecord(c->ev_win[c->window.rec], c->stream));
    if (c->refine.rec) {   // the measured frame's end (its chain joined): its part statistics are complete
        HIP_TRY(c, hipEventRecord(c->ev_refine, c->stream));
        c->refine.rec = false;
        c->refine.state = 1;
    }
    if (tracked) {
        HIP_TRY(c, hipEventRecord(c->ev_frame, c->stream));
        if (!c->in_registry) {
            frames_note(c);
            c->in_registry = true;
        }
    } else if (c->in_registry) {
        frames_forget(c);
        c->in_registry = false;
    }
    return RTX_OK;
}

}  // namespace

// count: 0 a frame, 1 / 2 the instrumented kernels (launch_counting)
int launch(rtx_ctx* c, const FrameArgs& F, dim3 grid, int count) {
    if (grid.x == 0 || grid.y == 0) return RTX_OK;
    // (prepare joined already unless this frame repeats the last one's parameters and cameras)
    const bool inflight_join = c->concurrent && (!c->defer_inflight || c->window.state == 2 || c->window.state == 3);
    if (c->join.pending && (count || F.cost || F.part_max || F.lm_lights || inflight_join || c->facts.hbm_stack ||
                            c->facts.deep_stack || F.heavy_flag != c->join.heavy || F.heavy_n != c->join.heavy_n))
        if (const int rc = join_split(c); rc != RTX_OK) return rc;
    if (c->facts.hbm_stack)
        if (const int rc = ensure_hbm_stacks(c, grid.x); rc != RTX_OK) return rc;
    if (count) return launch_counting(c, F, grid, count);
    ++c->renders_since_upload;
    if (c->dev.cull_stride)   // the views' camera-anchor cull records, when a camera moved
        if (const int rc = cull_views(c, F); rc != RTX_OK) return rc;
    // the first specialised variant whose facts the scene and frame satisfy (kSpecVariants;
    // RTX_NO_SPEC=1 forces the generic kernel); the split launches take it too
    const int facts = c->facts.spec | ((F.mode == RTX_MODE_COMBINED && F.shadows) ? kSpecCombShadows : 0);
    const int v = (c->no_spec || c->facts.deep_stack) ? -1 : spec_variant(facts);
    c->last_facts = facts;
    c->last_variant = v;
    if (F.heavy_flag)
        if (const int rc = launch_chain(c, F, v); rc != RTX_OK) return rc;
    if (const int rc = launch_main(c, F, grid, v); rc != RTX_OK) return rc;
    if (F.heavy_flag && c->tuner.rec && F.cost) HIP_TRY(c, hipEventRecord(c->ev_tune[1], c->stream));
    if (F.heavy_flag) {
        // a plain repeat of the frame defers the join to the next frame or reader (rtx_ctx::join);
        // a measured, tuned, refined or in-flight one joins now
        if (F.cost || F.part_max || inflight_join || c->join.off || c->tuner.rec || c->refine.rec) {
            HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_join, 0));
        } else {
            c->join.pending = true;
            c->join.heavy = F.heavy_flag;
            c->join.heavy_n = F.heavy_n;
        }
    }
    if (F.cost)   // the next frames' order and heavy set (rtx_sched.hip)
        if (const int rc = sched_update(c, F); rc != RTX_OK) return rc;
    return end_frame(c);
}

void remember(rtx_ctx* c, const rtx_render_params* p, int n_views, bool rgb) {
    c->last = *p;
    c->last_views = n_views;
    c->last_valid = true;
    c->last_rgb = rgb;
}

// Queue the D2H copy of the rows a render of `p` with `n_views` views owns into the caller's
// full-frame host buffers, on the context stream, for every plane with a destination.  A striped
// frame is one hipMemcpy2DAsync per view and plane: `stripe_rows` rows every `stripe_step` stripes
// (row pitch of the 2-D copy = stripe_step stripes), plus the trailing partial stripe.
int queue_rows(rtx_ctx* c, const rtx_render_params& p, int n_views, const CopyPlane* planes, int n_planes) {
    const size_t W = p.width, H = p.height;
    const bool striped = p.stripe_rows != 0 && p.stripe_step > 1;
    for (int v = 0; v < n_views; ++v) {
        const size_t base = static_cast<size_t>(v) * W * H;
        const size_t rows = striped ? p.stripe_rows : H, step = striped ? p.stripe_step : 1;
        const size_t first = striped ? (p.stripe_first + step - static_cast<uint32_t>(v) % step) % step : 0;
        // owned stripes s = first + k*step; the full ones end at or before row H
        size_t n_full = 0;
        if ((first + 1) * rows <= H) n_full = ((H / rows) - 1 - first) / step + 1;
        const size_t last = first + n_full * step;   // next owned stripe (maybe partial or past H)
        for (int k = 0; k < n_planes; ++k) {
            const CopyPlane& pl = planes[k];
            if (!pl.dst) continue;
            if (!striped) {
                HIP_TRY(c, hipMemcpyAsync(pl.dst + base * pl.elem, pl.src + base * pl.elem, W * H * pl.elem,
                                          hipMemcpyDeviceToHost, c->stream));
                continue;
            }
            const size_t row_b = W * pl.elem, off = (base + first * rows * W) * pl.elem;
            if (n_full)
                HIP_TRY(c, hipMemcpy2DAsync(pl.dst + off, step * rows * row_b, pl.src + off, step * rows * row_b,
                                            rows * row_b, n_full, hipMemcpyDeviceToHost, c->stream));
            if (last * rows < H) {
                const size_t o2 = (base + last * rows * W) * pl.elem;
                HIP_TRY(c, hipMemcpyAsync(pl.dst + o2, pl.src + o2, (H - last * rows) * row_b, hipMemcpyDeviceToHost,
                                          c->stream));
            }
        }
    }
    return RTX_OK;
}

}  // namespace rtxh

namespace {

// ... of the last colour frame
int queue_owned_copy(rtx_ctx* c, uint32_t* out_px, float* out_rgb) {
    if (!c || !out_px) return RTX_E_INVALID;
    if (!c->last_valid) return fail(c, RTX_E_STATE, "nothing rendered yet");
    if (out_rgb && !c->last_rgb) return fail(c, RTX_E_STATE, "last render did not produce colours");
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = join_split(c); rc != RTX_OK) return rc;
    const CopyPlane planes[2] = {{reinterpret_cast<char*>(out_px), reinterpret_cast<const char*>(c->d_px.get()), 4},
                                 {reinterpret_cast<char*>(out_rgb), reinterpret_cast<const char*>(c->d_rgb.get()), 12}};
    return queue_rows(c, c->last, c->last_views, planes, 2);
}

}  // namespace

extern "C" int rtx_set_supersample(rtx_ctx* c, uint32_t k) {
    if (!c) return RTX_E_INVALID;
    if (k != 1 && k != 2 && k != 4 && k != 8)
        return fail(c, RTX_E_INVALID, "supersample factor must be 1, 2, 4 or 8 (got " + std::to_string(k) + ")");
    c->ss_log2 = k == 8 ? 3u : (k == 4 ? 2u : (k == 2 ? 1u : 0u));
    return RTX_OK;
}

extern "C" int rtx_render_views_async(rtx_ctx* c, const rtx_camera* cams, int n_views, const rtx_render_params* p,
                                      int want_rgb) {
    FrameArgs F;
    dim3 grid;
    int rc = prepare(c, cams, n_views, p, want_rgb != 0, F, grid);
    if (rc != RTX_OK) return rc;
    rc = launch(c, F, grid, 0);
    if (rc != RTX_OK) return rc;
    remember(c, p, n_views, want_rgb != 0);
    return RTX_OK;
}

extern "C" int rtx_render_async(rtx_ctx* c, const rtx_camera* cam, const rtx_render_params* p, int want_rgb) {
    return rtx_render_views_async(c, cam, 1, p, want_rgb);
}

extern "C" int rtx_synchronize(rtx_ctx* c) {
    if (!c) return RTX_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    if (const int rc = join_split(c); rc != RTX_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}

extern "C" int rtx_download(rtx_ctx* c, uint32_t* out_px, float* out_rgb) {
    const int rc = queue_owned_copy(c, out_px, out_rgb);
    if (rc != RTX_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}

extern "C" int rtx_gather_async(rtx_ctx* c, uint32_t* out_px, float* out_rgb) {
    return queue_owned_copy(c, out_px, out_rgb);
}

extern "C" int rtx_host_register(rtx_ctx* c, void* p, size_t bytes) {
    if (!c || !p || !bytes) return RTX_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipHostRegister(p, bytes, hipHostRegisterPortable));
    return RTX_OK;
}

extern "C" int rtx_host_unregister(rtx_ctx* c, void* p) {
    if (!c || !p) return RTX_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipHostUnregister(p));
    return RTX_OK;
}

extern "C" int rtx_render(rtx_ctx* c, const rtx_camera* cam, const rtx_render_params* p, uint32_t* out_px,
                          float* out_rgb) {
    if (!out_px) return RTX_E_INVALID;
    int rc = rtx_render_async(c, cam, p, out_rgb != nullptr);
    if (rc != RTX_OK) return rc;
    return rtx_download(c, out_px, out_rgb);
}

extern "C" int rtx_device_buffers(rtx_ctx* c, void** d_px, void** d_rgb) {
    if (!c) return RTX_E_INVALID;
    if (const int rc = join_split(c); rc != RTX_OK) return rc;   // (the caller orders its work after the stream)
    if (d_px) *d_px = c->d_px;
    if (d_rgb) *d_rgb = c->d_rgb;
    return RTX_OK;
}
