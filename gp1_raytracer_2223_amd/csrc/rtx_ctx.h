// rtx_ctx.h — the render context (rtx_ctx, the opaque handle of include/rtx.h) and what the host
// units of librtx_hip.so call across each other (namespace rtxh): the frame policies (their state
// and pure transitions are rtx_policy.h's structs, one per policy; rtx_policy.hip makes their HIP
// calls: the split tuner, the throughput / in-flight choice, the frontier refinement and the
// deferred join of the split chain), the context's device buffers (DevBuf), the upload
// (rtx_upload.hip, committing what the HIP-free rtx_pack.h packs), the cull records
// (rtx_cull_records.hip), the in-place edits (rtx_edit.hip), the tile schedule (rtx_sched.hip), the frame (rtx_frame.hip) and what the stored hit pass's consumers share (rtx_pass.hip).  The render
// kernel's launches are rtx_launch.h's.  Internal to librtx_hip.so.
#pragma once

#include <hip/hip_runtime.h>

#include <array>
#include <cstdint>
#include <string>
#include <vector>

#include "rtx.h"
#include "rtx_diag.h"
#include "rtx_cull.h"
#include "rtx_kernels.h"
#include "rtx_pack.h"
#include "rtx_policy.h"

using namespace rtxd;

// The two kinds of cull-record tree values (rtx_cull_tris / rtx_cull_nodes in rtx_cull_records.hip): margin +
// dt per triangle, a box per node slot.  Margins and dt are >= 0 or +inf (never NaN), box bounds never
// NaN either, so the trees' min / max folds are exact in any order.
struct alignas(8) CullMD {
    float m, dt;
};
struct alignas(16) CullBox {
    float lo[3], pad0, hi[3], pad1;
};

static_assert(kPolicyMaxViews == kMaxViews, "rtx_policy.h's cameras per frame");

namespace rtxh {
// What the tile schedule's launches (sched_launch, rtx_sched.hip) work on: device buffers for n_tiles tiles
// (hist: kCostBuckets per chunk of kSchedChunk tiles, csum: one per chunk, heavy_list: kMaxHeavyTiles,
// heavy_n: 4 words, zero before the first run), and the scalars of one run.
struct SchedBufs {
    uint32_t* cost;              // the measured costs; zero afterwards
    const uint32_t* was_heavy;   // the flags the measured frame was split by, or null: no tile was
    uint32_t* saved;             // last one-piece cost per tile
    uint32_t* hist;
    unsigned long long* csum;
    unsigned long long* thr;     // the heavy threshold
    uint32_t* order;
    uint32_t* order_xcd;         // the XCD re-deal of `order`, or null: none
    uint32_t* heavy_flag;
    uint32_t* heavy_list;
    uint32_t* heavy_n;
};
struct SchedParams {
    uint32_t n_tiles, tiles_x, tiles_y;
    uint32_t parts;         // motion mode: split tiles are costed by their part waves' sum
    uint32_t split_slots;   // effective: 0 no tile is heavy, 0xffffffff every tile is
    uint32_t permille, split_min, wave_slots;
};
}  // namespace rtxh

// A device buffer: its pointer and the units (elements, unless grow is told another size) it holds.
// One constructed with rtx_ctx::bufs is the context's: rtx_destroy frees every one of those.  Explicit
// lifetime, no destructor: a free needs the context's device current.
struct DevMem {
    void* p = nullptr;
    size_t cap = 0;
    void free() { (void)hipFree(p); p = nullptr; cap = 0; }
};
template <class T>
struct DevBuf : DevMem {
    DevBuf() = default;   // (a scene image's own: rtx_ctx::SceneBuf)
    explicit DevBuf(std::vector<DevMem*>& owner) { owner.push_back(this); }
    DevBuf(const DevBuf&) = delete;
    T* get() const { return static_cast<T*>(p); }
    operator T*() const { return get(); }
    // Free the buffer and allocate it again for `need` units of `elem` bytes (cap 0 when the allocation
    // fails).  No synchronisation: the caller has made sure that nothing queued still reads the old one.
    int grow(rtx_ctx* c, size_t need, size_t elem = sizeof(T));
    hipError_t alloc(size_t need, size_t elem = sizeof(T)) {   // ... with HIP's own error (for rtx_create's report)
        free();
        const hipError_t e = hipMalloc(&p, need * elem);
        if (e == hipSuccess) cap = need;
        return e;
    }
};

struct rtx_ctx {
    std::vector<DevMem*> bufs;   // every DevBuf below (first: they register as they are constructed)
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::string err;
    // scene image in HBM (one allocation, 256-B aligned sections)
    // Two scene images (device + pinned staging), alternated by uploads: an upload packs
    // into the image no queued frame reads and copies it asynchronously, so the host can
    // prepare the next animated frame while the GPU renders this one.
    struct SceneBuf {
        char* d = nullptr;
        char* h = nullptr;
        size_t cap = 0;
        hipEvent_t done = nullptr;   // recorded after the last frame that reads this image
        bool pending = false;
        DevBuf<float4> cull;         // the image's cull records (DevScene::cull), device only; cap in bytes
        void free() {                // (the image and its staging: explicit, like DevBuf's)
            (void)hipFree(d);
            if (h) (void)hipHostFree(h);
            d = h = nullptr;
            cap = 0;
        }
        hipError_t grow(size_t total) {
            free();
            hipError_t e = hipMalloc(&d, total);
            if (e == hipSuccess) e = hipHostMalloc(&h, total);
            if (e == hipSuccess) cap = total;
            return e;
        }
    };
    SceneBuf sb[2];
    int sb_cur = -1;
    size_t scene_bytes = 0;
    rtxh::SceneFacts facts;  // of the uploaded scene (rtx_pack.h)
    // In-place edits (rtx_edit_*, rtx_edit.hip): what the values derived from lights and materials need of
    // the uploaded scene, kept in step by every edit; edit_ok: the current image is a host upload's (a
    // device Update's registration and its images are not edited)
    rtxh::EditInputs edit;
    bool edit_ok = false;
    DevScene dev{};
    bool has_scene = false;
    // frame buffer in HBM
    DevBuf<uint32_t> d_px{bufs};
    DevBuf<float> d_rgb{bufs};   // 3 floats a pixel
    // supersampling (rtx_set_supersample): log2 of the k x k samples per pixel of every later frame;
    // the frame buffer stays width x height per view (FrameArgs::ss_log2)
    uint32_t ss_log2 = 0;
    DevBuf<unsigned long long> d_counters{bufs};
    // last render
    // cost-ordered tile dispatch
    DevBuf<uint32_t> d_order{bufs};
    DevBuf<uint32_t> d_order_xcd{bufs};   // the XCD-affine re-deal of d_order (rtx_sched_xcd)
    bool xcd_order = false;               // RTX_XCD_ORDER=1
    DevBuf<uint32_t> d_cost{bufs};
    DevBuf<uint32_t> d_saved_cost{bufs};  // last one-piece cost per tile
    DevBuf<uint32_t> d_hist{bufs};        // per (class, chunk) tile counts -> slot bases (rtx_sched_*)
    DevBuf<unsigned long long> d_csum{bufs};   // per chunk cost sums
    DevBuf<unsigned long long> d_thr{bufs};    // heavy threshold of the measured frame
    uint32_t sched_cap = 0;               // tiles the schedule arrays and d_heavy_flag hold (set once all have grown)
    std::string sched_key;
    bool sched_ready = false;
    bool sched_enabled = true;
    rtxh::SchedParams sched_params{};     // of the last measured frame's update, and the heavy set it
    int sched_stage = 0;                  // staged (rtx_schedule_heavy)
    uint64_t sched_frame = 0;
    uint64_t scene_gen = 0;
    // split rendering of heavy tiles: double-buffered flag/list sets (HeavySet)
    DevBuf<uint32_t> d_heavy_flag[2] = {DevBuf<uint32_t>{bufs}, DevBuf<uint32_t>{bufs}};
    DevBuf<uint32_t> d_heavy_list[2] = {DevBuf<uint32_t>{bufs}, DevBuf<uint32_t>{bufs}};
    DevBuf<uint32_t> d_heavy_n{bufs};
    rtxh::HeavySet heavy;
    uint32_t* h_heavy_n = nullptr;   // pinned
    hipEvent_t ev_heavy = nullptr;
    hipStream_t split_stream = nullptr;   // split launches run beside the main kernel
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // Throughput mode (prepare): another context of this process on the same device still had a frame
    // in flight when this one was queued (ev_frame, the end of each queued frame; g_frames).  The
    // GPU then interleaves the contexts' frames and a tile's critical path is hidden by the other
    // frames, so the split launches only add work: the measured frames select heavy tiles with at
    // least kThroughputPermille and the tuner (whose timings the other frames distort) waits.
    hipEvent_t ev_frame = nullptr;
    bool in_registry = false;                   // listed in g_frames (its ev_frame is recorded per frame)
    bool concurrent = false;
    bool throughput_off = false;                // RTX_THROUGHPUT=0
    // in flight (kInflightCritPermille): the heaviest tile's one-piece cost measured in the last
    // serialized measurement (cost units), the threshold (RTX_INFLIGHT_CRIT), and whether the last
    // frame rendered one piece because of it
    uint32_t max_cost_serial = 0;
    rtxh::DeferredJoin join;                    // the deferred join of the last frame's split chain (join_split)
    // frames in flight defer too, except while the in-flight overlap window is timed (RTX_DEFER_INFLIGHT=0: never)
    bool defer_inflight = true;
    rtxh::InflightWindow window;                // the split frames' interval in flight (inflight_onepiece)
    hipEvent_t ev_win[2] = {};
    uint32_t inflight_crit = kInflightCritPermille;
    bool frame_onepiece = false;
    uint32_t split_mode = 1;         // 0 off, 1 auto, 2 force (RTX_SPLIT=0 / unset / force)
    uint32_t split_slots = 0;        // concurrent render waves on this device
    uint32_t split_min = kSplitMinCost;         // RTX_SPLIT_MIN_US: the least cost (16-cycle units) a split tile has
    rtxh::SplitTuner tuner;                     // the split factor and its tuner
    hipEvent_t ev_tune[3] = {nullptr, nullptr, nullptr};
    uint32_t sched_period = kSchedPeriod;       // RTX_SCHED_PERIOD (tuning)
    rtxh::Motion motion;                        // motion mode (kMotionFrames)
    bool frame_motion = false;                  // the frame being prepared / launched is in motion mode
    uint32_t split_parts = kPartsPerMesh;            // RTX_SPLIT_PARTS (tuning)
    // frontier refinement (kRefineRounds): the current image's parts (host copy of the real entries;
    // the image reserves kMaxParts), its parts section, and the rounds' state
    bool refinable = false;
    rtxh::Refinement refine;
    std::vector<int4> h_parts;
    std::vector<int4> h_parts_base;                  // the upload's frontier (each launch shape starts from it)
    int4* parts_dev = nullptr;
    hipEvent_t ev_refine = nullptr;
    DevBuf<uint32_t> d_part_max{bufs};
    std::vector<uint32_t> h_part_max;
    DevBuf<uint4> d_hstk{bufs};      // the HBM stacks (and the instrumented variant's masks), grown on demand
    DevBuf<unsigned long long> d_hstkT{bufs};
    bool room_skip_off = false;      // RTX_ROOM_SKIP=0 (SceneFacts::room_fact)
    bool no_spec = false;            // RTX_NO_SPEC=1: always the generic kernel (tests)
    int last_facts = 0;              // rtx_spec_info: the facts and the kSpecVariants index (-1: the
    int last_variant = -1;           // generic kernel) of the last frame launched
    DevBuf<unsigned long long> d_hit_key{bufs};
    DevBuf<uint32_t> d_occ{bufs};
    // Light-major frames (FrameArgs::lm_*, DESIGN.md §6, opt-in): lm_mode 0 never (default), 1 auto
    // (RTX_LIGHT_MAJOR=auto: a launch of at most lm_tiles wave tiles, kLmSlotsPercent of the resident
    // wave slots, RTX_LIGHT_MAJOR_TILES), 2 always (RTX_LIGHT_MAJOR=1)
    uint32_t lm_mode = 0;
    uint32_t lm_tiles = 0;
    uint32_t lm_waves = 0;                      // PHASE 5's persistent waves: every resident slot (32 per CU)
    DevBuf<float4> d_lm_rec{bufs};              // 2 float4 per tile pixel; cap in tiles
    DevBuf<unsigned long long> d_lm_mask{bufs}; // per (tile, light)
    bool frame_lm = false;                      // the frame being launched is light-major
    // exact cull (DevScene::cull): on for host uploads (RTX_NO_CULL=1: off); the
    // scratch of its record launches (the segment trees of the per-triangle boxes and of each
    // anchor's margins, the slots' boxes, the trees' arrival counters) and the node-slot ranges
    // in the current image
    bool no_cull = false;
    float cull_ratio = 1.5f;              // CullParams (RTX_CULL_RATIO, RTX_CULL_LEAVES: tuning)
    double cull_min_sa = 1.5;             // upload_scene's worth test (RTX_CULL_MIN_SA)
    bool cull_leaves = false;
    // Animated loops re-upload every frame and render it once, so the records are rebuilt per
    // frame.  Round 4's records cost more than a frame and were skipped after two such uploads;
    // the segment-tree records (tens of us) are built for every upload.  RTX_CULL_ANIMATED=0
    // restores the skip (after two consecutive uploads rendered at most once each, until an
    // upload is rendered twice).
    bool cull_animated = true;
    uint32_t renders_since_upload = 0;
    uint32_t short_uploads = 0;
    // The cull's worth estimate (upload_scene: the surface areas of every node's reference box and
    // tight box, tens of us of host time per upload) is reused by the uploads of such a loop for
    // kCullWorthReuse uploads while the scene's counts stay the same: the decision only picks the
    // faster of two exact walks.
    int cull_worth = -1;
    uint32_t cull_worth_age = 0;
    std::string cull_worth_sig;
    DevBuf<CullBox> d_cull_btree{bufs};   // 2n entries; cap = the leaves n it holds
    DevBuf<CullMD> d_cull_mtree{bufs};    // 2n entries per anchor of one launch
    uint32_t cull_failures = 0;           // record builds that failed (the image then renders unculled)
    uint32_t cull_fail_at = 0, cull_launches = 0;   // RTX_CULL_FAIL=k: the k-th record build fails (tests)
    DevBuf<CullBox> d_cull_nbox{bufs};    // per node slot of the current image
    DevBuf<uint32_t> d_cull_arrive{bufs}; // per tree (kCullMaxAnchors margin trees, then the box tree)
    uint32_t cull_top_lds = kCullTopLds;  // RTX_CULL_TOP_LDS (tests: the global-memory top levels)
    const uint2* cull_rng = nullptr;
    uint32_t cull_nslots = 0, cull_ntris = 0, cull_n = 0;
    float cull_view[kMaxViews][3] = {};   // camera origin each view's records of the current image were made for
    uint32_t cull_view_valid = 0;         // bit v: view v's records are current
    double cull_bmin[3] = {}, cull_bmax[3] = {};   // the meshes' box (a camera anchor's t bound, cull_bt)
    uint64_t cull_updates = 0;            // camera-anchor record launches so far (rtx_cull_info)
    float cull_anchor[kMaxViews + kMaxCullLights][5] = {};   // per record copy: anchor xyz, w, bt (rtx_cull_dump)
    std::vector<std::array<float, 4>> cull_lights;   // the uploaded lights' anchors {origin, T}
    bool cull_boxes_pending = false;      // an upload's boxes and light records wait for its first frame
    uint32_t cull_lights_dirty = 0;       // bit l: an edit moved light l, whose records alone wait (rtx_edit.hip)
    rtx_render_params last{};
    int last_views = 1;
    bool last_valid = false, last_rgb = false;
    // Hit pass (rtx_render_aov*): the planes in HBM (each allocated when a mask first asks for it;
    // aov_cap = the elements each allocated one holds) and the last pass's own record beside the
    // colour frame's `last`, so a colour gather after a pass still copies the colour frame's rows
    DevBuf<float> d_aov_depth{bufs}, d_aov_normal{bufs};
    DevBuf<uint32_t> d_aov_material{bufs}, d_aov_primitive{bufs};
    size_t aov_cap = 0;
    rtx_render_params aov_last{};
    int aov_last_views = 1;
    uint32_t aov_last_mask = 0;   // 0: no pass yet
    // ... and, for deferred shading (rtx_shade_aov*, rtx_deferred.hip), the pass's cameras and the
    // number of materials of the scene it traced (its material plane's indices lie below it)
    rtx_camera aov_last_cams[kMaxViews] = {};
    uint32_t aov_last_materials = 0;
    // Relighting (rtx_render_shadows_async, rtx_relight*: rtx_relight.hip).  The shadow plane in HBM, one
    // word per pixel of the hit pass (bit l: light l occluded), and its validity record: the hit pass it
    // belongs to, by the serial every hit pass bumps (0: no shadow pass yet), and the lights it was traced
    // for, each as its origin's and type's bits.  light_keys is the same of the scene uploaded last.
    uint64_t aov_serial = 0;
    DevBuf<uint32_t> d_shadow{bufs};
    uint64_t shadow_serial = 0;
    std::vector<std::array<uint32_t, 4>> shadow_lights;
    std::vector<std::array<uint32_t, 4>> light_keys;
    // Ray queries and shaded rays (rtx_trace_rays, rtx_occluded, rtx_shade_rays: rtx_query.hip): the host
    // variants' staging buffer in HBM, the rays and then every result array of one call; its cap = the
    // rays it holds
    DevBuf<char> d_query{bufs};
    // Adaptive supersampling (rtx_render_adaptive*: rtx_adaptive.hip): the list of the pixels to refine
    // (width * height entries, grown on demand) and its length on the device, which an adaptive frame
    // never reads on the host; adapt_waves = the refinement's persistent waves (every wave slot at the
    // render kernel's occupancy, RTX_ADAPTIVE_WAVES caps it), adapt_valid = an adaptive frame was queued
    DevBuf<uint32_t> d_adapt_list{bufs};
    DevBuf<uint32_t> d_adapt_count{bufs};
    uint32_t adapt_waves = 0;
    bool adapt_valid = false;
};

namespace rtxh {

inline int fail(rtx_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

#define HIP_TRY(ctx, call)                                                                  \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess)                                                               \
            return rtxh::fail((ctx), RTX_E_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

// The other contexts on c's device with a frame still in flight, and the registry of contexts
// whose frames can be (rtx_ctx::ev_frame, throughput mode).
uint32_t frames_concurrent(rtx_ctx* c);
void frames_note(rtx_ctx* c);
void frames_forget(rtx_ctx* c);
// rtx_upload.hip.  Pack a scene (rtx_pack.h) and commit it to the context's next image; `reserve`
// (per mesh, or empty) and `P`, the packed scene, serve the device Update's registration.
int upload_scene(rtx_ctx* c, const rtx_scene* s, const std::vector<uint8_t>& reserve, PackedScene& P);
// The image a new scene of `total` bytes goes into: the one no queued frame reads, once the frames of
// two uploads ago are done with it, grown to hold it.  And its adoption once the copies are queued:
// every frame queued so far reads the previous image.
int next_image(rtx_ctx* c, size_t total, int& k);
int adopt_image(rtx_ctx* c, int k, size_t total);

// rtx_cull_records.hip: at upload, the light anchors (tmax bound T[l]) of the image's cull records;
// before a frame, the record launches its views still need; and the device's octant copies 1..7 of
// an uploaded node array (`n2` node records per copy, copies `stride` float4 apart).
void cull_records(rtx_ctx* c, const std::vector<float>& T, const rtx_light* lights, uint32_t n_lights);
int cull_views(rtx_ctx* c, const FrameArgs& F);
// whether record launches that need no view wait (an upload's, or an edit's moved lights)
inline bool cull_lights_due(const rtx_ctx* c) { return c->cull_boxes_pending || c->cull_lights_dirty != 0; }
void octant_expand(float4* nodes, uint32_t n2, uint32_t stride, hipStream_t s);

// rtx_sched.hip: queue the next frames' dispatch order and heavy set from measured frame F's tile costs;
// and the launches themselves, on buffers and scalars of the caller's (HIP's error, nothing of a context).
int sched_update(rtx_ctx* c, const FrameArgs& F);
hipError_t sched_launch(hipStream_t s, const SchedBufs& B, const SchedParams& P);

// rtx_frame.hip: the launch record shared by a colour frame and the hit pass; a colour frame's
// checks, buffers and schedule; the HSTK variant's stacks; the frame's launches (count: 0 a frame,
// 1 / 2 the instrumented kernels); the record of the last frame; and the D2H copy of a frame's
// owned rows, plane by plane.
void frame_shape(rtx_ctx* c, const rtx_camera* cams, int n_views, const rtx_render_params* p,
                 const rtx_render_params& sp, uint32_t ss, FrameArgs& F, dim3& grid);
int prepare(rtx_ctx* c, const rtx_camera* cams, int n_views, const rtx_render_params* p, bool want_rgb, FrameArgs& F,
            dim3& grid);
// prepare's first step: what rtx_render* rejects of a frame's arguments, before anything is queued
int check_params(rtx_ctx* c, const rtx_camera* cams, int n_views, const rtx_render_params* p);
// The head of a launch shape's schedule key: the tile set (size, views, stripes), before the scene and mode
std::string tiles_key(uint32_t width, uint32_t height, int n_views, uint32_t stripe_rows, uint32_t stripe_first,
                      uint32_t stripe_step);
// ... its buffer step: the frame buffer (and the colour plane when asked for) of npx pixels
int frame_buffers(rtx_ctx* c, size_t npx, bool want_rgb);
// The kSpecVariants index of the first variant the facts satisfy (-1: none, the generic kernel).
int spec_variant(int facts);
int ensure_hbm_stacks(rtx_ctx* c, uint32_t groups);
int launch(rtx_ctx* c, const FrameArgs& F, dim3 grid, int count);
void remember(rtx_ctx* c, const rtx_render_params* p, int n_views, bool rgb);
struct CopyPlane { char* dst; const char* src; size_t elem; };
int queue_rows(rtx_ctx* c, const rtx_render_params& p, int n_views, const CopyPlane* planes, int n_planes);

// rtx_pass.hip: what a consumer of the stored hit pass (rtx_ctx::aov_last*) starts from.  Its checks, which
// change nothing; each entry point calls them in its contract's order (rtx.h's error tables):
// a shade's lighting mode and pixel format, as rtx_render checks them;
int shade_param_checks(rtx_ctx* c, const rtx_render_params* p);
// a scene, no supersampling, and a last hit pass with all four planes (`what` names the consumer);
int pass_checks(rtx_ctx* c, const char* what);
// and a scene with at least the materials the pass was traced with, and one at all.
int material_checks(rtx_ctx* c);
// The pass's shape with the call's mode, shadows and format: what the frame would be rendered with.
rtx_render_params pass_shape(const rtx_ctx* c, const rtx_render_params* p);
// The launch record of a kernel over the pass in `shape`, after the checks, join_split and any growth: the
// pass's cameras and tiles (frame_shape), the last colour frames' dispatch order when they had this tile
// set, the four planes, and the light anchors' cull records when they are due.  Nothing of the colour
// frames' state is written; the outputs are the caller's.
int pass_frame(rtx_ctx* c, const rtx_render_params& shape, FrameArgs& F, dim3& grid);
// The context's four device planes (NULL: not allocated yet), and the same bound into a launch record.
rtx_aov_planes device_planes(const rtx_ctx* c);
void bind_planes(const rtx_ctx* c, FrameArgs& F, uint32_t mask);
// The RTX_AOV_* bits of the planes of `o` that are not NULL.
uint32_t planes_mask(const rtx_aov_planes& o);

// Join the last frame's deferred split chain into the frame stream (rtx_ctx::join).
int join_split(rtx_ctx* c);
// One round of the frontier refinement once its measured frame has completed (rtx_ctx::refine).
int refine_round(rtx_ctx* c);
// The heaviest tile's serialized one-piece time over the split frame's serialized span (0 until known).
float inflight_ratio(const rtx_ctx* c);
// Whether a frame in flight, with k frames of this device's contexts at once, renders one piece.
bool inflight_onepiece(rtx_ctx* c, uint32_t k);

// The timed loop of every rtx_time_* entry point, after its checks and whatever it keeps outside the timing:
// once(i) for i = 0 .. iters-1 between ev0 and ev1 on the context stream, and their mean in *mean_ms.  The
// first code that is not RTX_OK is returned unchanged, *mean_ms untouched.
template <class Once>
int timed_loop(rtx_ctx* c, int iters, float* mean_ms, Once once) {
    HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
    for (int i = 0; i < iters; ++i)
        if (const int rc = once(i); rc != RTX_OK) return rc;
    HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
    HIP_TRY(c, hipEventSynchronize(c->ev1));
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *mean_ms = ms / static_cast<float>(iters);
    return RTX_OK;
}

}  // namespace rtxh

template <class T>
int DevBuf<T>::grow(rtx_ctx* c, size_t need, size_t elem) {
    HIP_TRY(c, alloc(need, elem));
    return RTX_OK;
}
