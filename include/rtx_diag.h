/*
 * rtx_diag.h — diagnostics of librtx_hip.so beside the product boundary (rtx.h): timing, the
 * instrumented work counters of the SURVEY §8(d) FLOP model, and the internals of the scheduling
 * and pruning machinery (cost-ordered dispatch, split rendering and its tuner, light-major frames,
 * the exact cull, the device Update's phase stamps).  None of these has a counterpart in the
 * reference's Renderer (source/Renderer.h:17-61); the benchmark (bench.py), the tools and the tests
 * use them.  Same conventions as rtx.h: RTX_OK or a negative RTX_E_* code, nothing throws.
 * (Implemented in csrc/rtx_diag.hip; the hit pass's timing in rtx_aov.hip, deferred shading's in rtx_deferred.hip, relighting's in rtx_relight.hip, the device Update's
 * stamps in rtx_anim_host.hip.)
 */
#ifndef RTX_DIAG_H_
#define RTX_DIAG_H_

#include "rtx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Time `iters` back-to-back launches of the render kernel(s) with HIP events recorded
 * on the context stream; writes the mean per-frame device time in ms. */
int rtx_time_frames(rtx_ctx* ctx, const rtx_camera* cam, const rtx_render_params* params,
                    int iters, float* mean_ms);
int rtx_time_views(rtx_ctx* ctx, const rtx_camera* cams, int n_views, const rtx_render_params* params,
                   int iters, float* mean_ms);
/* The same for the hit pass (rtx_render_aov_async with one camera and `mask`): `iters` back-to-back
 * passes, the mean device time of one in ms.  The planes then hold the pass, as after rtx_render_aov_async. */
int rtx_time_aov_frames(rtx_ctx* ctx, const rtx_camera* cam, const rtx_render_params* params, uint32_t mask,
                        int iters, float* mean_ms);
/* The same for deferred shading (rtx_shade_aov_async(params, want_rgb), rtx.h): `iters` back-to-back
 * shades of the last hit pass, the mean device time of one in ms.  The frame buffer then holds the
 * shaded pass, as after rtx_shade_aov_async. */
int rtx_time_shade_aov(rtx_ctx* ctx, const rtx_render_params* params, int want_rgb, int iters, float* mean_ms);
/* The same for relighting (rtx.h): `iters` back-to-back shadow passes (rtx_render_shadows_async) or relights
 * (rtx_relight_async(params, want_rgb)) of the last hit pass, the mean device time of one in ms.  The
 * shadow plane or the frame buffer then holds the result, as after the call timed. */
int rtx_time_shadows(rtx_ctx* ctx, int iters, float* mean_ms);
int rtx_time_relight(rtx_ctx* ctx, const rtx_render_params* params, int want_rgb, int iters, float* mean_ms);
/* The same for the resolved relight (rtx_relight_resolve_async(params, k, want_rgb), rtx.h): `iters`
 * back-to-back launches under its checks, the mean device time of one in ms.  The frame buffer and the
 * last-frame record are then as after one call.  iters <= 0 or a NULL mean_ms: RTX_E_INVALID. */
int rtx_time_relight_resolve(rtx_ctx* ctx, const rtx_render_params* params, uint32_t k, int want_rgb, int iters,
                             float* mean_ms);
/* The same for the incremental shadow pass: `iters` back-to-back launches of rtx_update_shadows_async(lights)
 * under its checks, the mean device time of one in ms.  Re-tracing is idempotent, so the plane and its
 * record are then as after one call.  iters <= 0 or a NULL mean_ms: RTX_E_INVALID. */
int rtx_time_shadows_update(rtx_ctx* ctx, uint32_t lights, int iters, float* mean_ms);
/* The same for a ray query on device pointers (rtx.h): `iters` back-to-back queries of the same n rays,
 * the mean device time of one in ms.  what 0: rtx_trace_rays_device(d_rays, n, mask, d_out); 1:
 * rtx_occluded_device(d_rays, n, d_occ); 2: the yardstick, a device-to-device copy of the n rays (32 n
 * bytes) into the context's staging buffer. */
int rtx_time_ray_queries(rtx_ctx* ctx, const rtx_ray* d_rays, uint32_t n, int what, uint32_t mask,
                         const rtx_aov_planes* d_out, uint8_t* d_occ, int iters, float* mean_ms);
/* The same for rtx_shade_rays_device(d_rays, n, params, d_pixels, d_rgb): `iters` back-to-back calls, the
 * mean device time of one in ms. */
int rtx_time_shade_rays(rtx_ctx* ctx, const rtx_ray* d_rays, uint32_t n, const rtx_render_params* params,
                        uint32_t* d_pixels, float* d_rgb, int iters, float* mean_ms);
/* The same for rtx_render_adaptive_async(cam, params, 0, k, threshold) (rtx.h): `iters` back-to-back
 * adaptive frames (plain frame, classification, refinement; no colour plane, as rtx_time_frames), the
 * mean device time of one in ms. */
int rtx_time_adaptive_frames(rtx_ctx* ctx, const rtx_camera* cam, const rtx_render_params* params, uint32_t k,
                             uint32_t threshold, int iters, float* mean_ms);
/* Bytes of HBM the uploaded scene image occupies. */
int rtx_scene_bytes(const rtx_ctx* ctx, uint64_t* bytes);
/* Diagnostics: copy the context's current scene image (DESIGN.md §2 layout) after its queued
 * work; `bytes` gets the image size (out may be NULL to query it). */
int rtx_scene_image(rtx_ctx* ctx, void* out, size_t capacity, size_t* bytes);
/* Instrumented render: the same traversal with per-ray work counters (12 x uint64, in
 * the order pixels, sphere, plane, slab, tri, hit, shadow, occluded, shade_base,
 * shade_lambert, shade_phong, shade_ct — the SURVEY §8(d) FLOP model).  Not timed. */
int rtx_count_work(rtx_ctx* ctx, const rtx_camera* cam, const rtx_render_params* params,
                   uint64_t* counts12);
/* Same, plus diagnostics appended after the 12 model counters: [12] node-pair tests and
 * [13] triangle tests executed per WAVE (packet work, one count per wave per step). */
int rtx_count_work_ex(rtx_ctx* ctx, const rtx_camera* cam, const rtx_render_params* params,
                      uint64_t* counts, int n_counts);
/* The same counters for the walk the product executes when the scene has exact-cull records
 * (otherwise identical to rtx_count_work_ex): slab [3] and triangle [4] tests the
 * culled, ordered walk performs per lane (a lane in a node's mask is tested against both
 * children), [12]/[13] per-wave steps, and [14] the exact-cull box tests.  One-piece frame (the
 * split launches' extra path tests not included).  Not timed. */
int rtx_count_work_culled(rtx_ctx* ctx, const rtx_camera* cam, const rtx_render_params* params,
                          uint64_t* counts, int n_counts);
/* Split rendering of heavy tiles (no reference counterpart: a scheduling detail of this
 * path).  Tiles whose measured cost exceeds their share of the frame are re-rendered with
 * their BVH traversals cut into `parts` subtree pieces run by separate workgroups; the
 * pixels are identical either way.  Reports the heavy-tile count the next frame will use
 * and the frontier size of the uploaded scene (0 = the scene is rendered unsplit).
 * Environment: RTX_SPLIT=0 disables, RTX_SPLIT=force splits every tile (tests). */
int rtx_split_info(rtx_ctx* ctx, uint32_t* heavy_tiles, uint32_t* parts);
/* Light-major frames (no reference counterpart: a decomposition of the frame's work that never
 * changes a pixel; opt-in, measured slower than one piece): one wave per tile for the
 * primary hits, persistent waves over the (tile, light) shadow rays, one wave per tile shading every
 * light in the reference's order.  Reports whether the last prepared frame was light-major and the
 * largest launch (wave tiles) that is: 0 never (the default), 0xffffffff always (RTX_LIGHT_MAJOR=1),
 * else the threshold of RTX_LIGHT_MAJOR=auto (RTX_LIGHT_MAJOR_TILES). */
int rtx_light_major_info(rtx_ctx* ctx, uint32_t* last_frame, uint32_t* max_tiles);
/* The split threshold's tuner: the current factor (a tile is split when its cost
 * exceeds factor x its share of the frame), the last timed frame's main kernel and split chain
 * (ms, from the fork), and the tuner's state (0 tuning, 1 converged, 2 off: RTX_SPLIT_TUNE=0 or a
 * fixed RTX_SPLIT_FACTOR).  Re-tuned for every new launch shape. */
int rtx_split_tune_info(rtx_ctx* ctx, float* factor, float* main_ms, float* chain_ms, uint32_t* done);
/* Frames in flight: while another context's frame is in flight on the device, a frame
 * whose tiles would split renders one piece when its heaviest tile's serialized one-piece time is
 * below crit_threshold x the split frame's serialized span (the split tuner's best; RTX_INFLIGHT_CRIT,
 * 0: always split as serialized frames do), or when split frames in flight, timed on this context's
 * stream, were found not to overlap.  Reports whether the last prepared frame saw another context's
 * frame in flight, whether it rendered one piece for that, the ratio (heaviest tile / split span; 0
 * until both are measured), the threshold and the split frames' interval in flight (ms, 0 before). */
int rtx_inflight_info(rtx_ctx* ctx, uint32_t* concurrent, uint32_t* onepiece, float* crit, float* crit_threshold,
                      float* split_interval_ms);
/* Exact cull (no reference counterpart: a pruning of the reference's own BVH walk that never
 * changes a pixel).  Reports whether the uploaded scene renders with it (on for
 * host uploads whose reference boxes are inflated enough to pay, see upload_scene) and how
 * many times a camera's records were (re)built.  Environment: RTX_NO_CULL=1 disables;
 * RTX_CULL_MIN_SA, RTX_CULL_RATIO tune the enabling test and the per-node flag (tests). */
int rtx_cull_info(rtx_ctx* ctx, uint32_t* enabled, uint64_t* camera_updates);
/* Kernel specialisation (no reference counterpart: variants of the render kernel with uniform facts
 * of the scene and frame compiled in; the same operations, so the same pixels).
 * Reports the facts (kSpec* bits, csrc/rtx_kernels.h) of the last frame launched and the variant it
 * took: an index into kSpecVariants, or -1 for the generic kernel (no variant's facts hold, a deep
 * BVH, RTX_NO_SPEC=1).  After an upload and before the next frame: the scene's facts and -1.  Host
 * bookkeeping at the launch site only. */
int rtx_spec_info(rtx_ctx* ctx, uint32_t* facts, int32_t* last_variant);
/* Room skip (no reference counterpart: shadow-ray room-plane tests the reference's own binary32
 * arithmetic provably fails are not executed).  Reports the uploaded scene's fact (the
 * five planes are the room, every light is a point light strictly inside it, and the light margins
 * span at most 2^100) and room_M = RD(2^20 x the smallest light margin): a wave skips the tests when
 * every shadow origin in it lies strictly inside the room within room_M of every plane.  Fact 0 and
 * room_M 0 when it does not hold or RTX_ROOM_SKIP=0 (read at rtx_create) turned the skip off. */
int rtx_room_info(rtx_ctx* ctx, uint32_t* fact, float* room_M);
/* Diagnostics of the exact cull (tests): waits for the context stream, then copies the current
 * image's records of record copy `anchor` (view v < 8: its camera; 8 + l: light l) — n_slots x
 * 8 floats, {c, E.x}, {E.y, E.z, dt, flag bits} — and their inputs: per slot the triangle range
 * [first, end) (2 x u32), node copy 0 (8 floats per slot), the triangle records (16 floats
 * each: {v0, n.x}, {E1, n.y}, {E2, n.z}, {mat}), and the anchor the copy was last built for
 * (x, y, z, w = 0 camera / tmax bound of a light, bt).  Null pointers are skipped; sizes via
 * *n_slots / *n_tris.  RTX_E_INVALID when the scene has no records. */
int rtx_cull_dump(rtx_ctx* ctx, uint32_t anchor, uint32_t* n_slots, uint32_t* n_tris, float* anchor_p,
                  float* records, uint32_t* ranges, float* nodes, float* tris);
/* Diagnostics of the cost-ordered dispatch (tests): after a measured frame, the dispatch
 * permutation of the first n tiles' slots (`order`) and the one-piece tile costs it was
 * sorted by (`cost`).  *n_tiles = tiles of the current schedule (0 = none measured yet;
 * then nothing is copied). */
int rtx_schedule_state(rtx_ctx* ctx, uint32_t* order, uint32_t* cost, uint32_t n, uint32_t* n_tiles);
/* Diagnostics of the XCD-affine re-deal (tests): the first n slots of the permutation the render
 * kernel consumes on a context created under RTX_XCD_ORDER=1, i.e. rtx_schedule_state's `order`
 * re-dealt by rtx_sched_xcd.  RTX_E_STATE when the context has no XCD order (the knob is off, or no
 * frame of the current schedule has been measured yet). */
int rtx_schedule_xcd_order(rtx_ctx* ctx, uint32_t* order, uint32_t n);
/* Diagnostics of the heavy set (tests): what the last measured frame's schedule update selected.  Joins as
 * rtx_schedule_state does, then copies out the heavy flags of the first n tiles (the set that update
 * staged, adopted since or not), its heavy list (RTX_MAX_HEAVY_TILES words; the entries past the count
 * are stale), the four counter words {heavy tiles (not clamped), 0, largest tile cost, cost per wave
 * slot}, the heavy threshold, and the scalars the update ran with: {effective split slots (0 no tile is
 * heavy, 0xffffffff every tile is), split permille, least split cost, wave slots}.  Null pointers are
 * skipped.  RTX_E_STATE when no frame of the current schedule has been measured, RTX_E_INVALID when n
 * exceeds the schedule size. */
#define RTX_MAX_HEAVY_TILES 8192
int rtx_schedule_heavy(rtx_ctx* ctx, uint32_t* heavy_flag, uint32_t n, uint32_t* heavy_list, uint32_t heavy_n[4],
                       uint64_t* threshold, uint32_t params[4]);
/* Diagnostics of the schedule kernels (tests): run the launches that a measured frame queues (count,
 * scan, scatter and, with `xcd`, the XCD re-deal) on costs of the caller's.  All arrays are host memory.
 * The run uses scratch device buffers of its own on the context's device, initialised like a fresh
 * launch shape's, queues on the context stream, waits, copies out and frees: no schedule, policy or
 * heavy-set state of the context is read or written, and its frames are unchanged.
 * RTX_E_INVALID, before any device work: a NULL case, result or required array (was_heavy may be NULL: no
 * tile was split; order_xcd only with `xcd`), n == 0 or above 2^20, tiles_x * tiles_y == 0, or with
 * `xcd` an n that is no multiple of tiles_x * tiles_y. */
typedef struct rtx_schedule_case {
    const uint32_t* cost;        /* [n] the measured tile costs */
    const uint32_t* was_heavy;   /* [n] non-zero: the tile was rendered split; or NULL */
    const uint32_t* saved;       /* [n] the last one-piece cost per tile */
    uint32_t n;                  /* tiles */
    uint32_t tiles_x, tiles_y;   /* tiles per view (the XCD re-deal's blocks) */
    uint32_t parts;              /* motion mode: split tiles are sorted by cost, not by saved */
    uint32_t split_slots;        /* effective: 0 no tile is heavy, 0xffffffff every tile is */
    uint32_t permille;
    uint32_t split_min;
    uint32_t wave_slots;
    uint32_t xcd;                /* non-zero: the XCD re-deal too */
} rtx_schedule_case;
typedef struct rtx_schedule_result {
    uint32_t* order;             /* [n] */
    uint32_t* order_xcd;         /* [n], with `xcd` */
    uint32_t* cost_after;        /* [n] */
    uint32_t* saved_after;       /* [n] */
    uint32_t* heavy_flag;        /* [n] */
    uint32_t* heavy_list;        /* [RTX_MAX_HEAVY_TILES]; 0xffffffff past the entries written */
    uint32_t heavy_n[4];
    uint64_t threshold;
} rtx_schedule_result;
int rtx_schedule_run(rtx_ctx* ctx, const rtx_schedule_case* in, rtx_schedule_result* out);

/* Diagnostics: 128 status words of the last update of registered mesh i (0-3 as above,
 * 4-6 subtrees / task-split ids / nodes split as tasks, 8-27 phase stamps of the device build
 * at 100 MHz; csrc/rtx_anim.h). */
int rtx_anim_stamps(rtx_anim* anim, uint32_t i, uint32_t out[128]);

#ifdef __cplusplus
}
#endif
#endif /* RTX_DIAG_H_ */
