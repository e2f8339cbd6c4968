/*
 * rtx.h — C-ABI drop-in boundary for the per-pixel render loop of
 * JonathanMenschaert/GP1_Raytracer_2223 (`Renderer::Render` → `RenderPixel`).
 *
 * The reference has no plugin API; its seam is `Renderer::Render(Scene*) const`
 * (source/Renderer.h:28, called once per frame from source/main.cpp:91) with the
 * per-pixel body `Renderer::RenderPixel` (source/Renderer.cpp:100-182).  This header
 * replaces that seam with plain C: the caller flattens its Scene into `rtx_scene`
 * (plain pointers + sizes, no C++ or torch types), uploads it once to HBM with
 * `rtx_upload_scene`, then calls `rtx_render` once per frame.
 *
 * Scene records are laid out byte-for-byte like the reference's own value types so a
 * reference Scene can hand its std::vector storage over without repacking:
 *   rtx_sphere   == dae::Sphere   (source/DataTypes.h:13-19,  20 B)
 *   rtx_plane    == dae::Plane    (source/DataTypes.h:21-27,  28 B)
 *   rtx_bvh_node == dae::BVHNode  (source/DataTypes.h:43-54,  36 B)
 *   rtx_light    == dae::Light    (source/DataTypes.h:528-536, 44 B)
 * Materials are polymorphic in the reference (source/Material.h) and are flattened
 * into the tagged `rtx_material`.
 *
 * Error convention: every entry point returns RTX_OK (0) or a negative RTX_E_* code and
 * never throws across the ABI; `rtx_last_error` gives a human-readable reason.  (The
 * reference itself has no error channel: Renderer::Render returns void.)
 *
 * Threading: like Renderer::Render (called only from the main thread), one caller
 * thread per rtx_ctx.  Different contexts (one per GPU) may be driven concurrently.
 *
 * This header is the product boundary: contexts, scene upload, rendering, the host gather, one frame
 * over several GPUs (rtx_group_*) and the device-side Update (rtx_anim_*).  Timing, work counters
 * and the scheduler's / exact cull's internals are in rtx_diag.h; the environment knobs the library
 * reads are listed in INTEGRATION.md (none of them changes a pixel).  In csrc/ the entry points
 * live by topic: rtx_context.hip, rtx_upload.hip, rtx_frame.hip, rtx_aov.hip (the hit pass),
 * rtx_deferred.hip (deferred shading), rtx_relight.hip (the shadow pass and the relight), rtx_edit.hip (scene edits in place), rtx_query.hip (ray queries and shaded rays), rtx_adaptive.hip (adaptive supersampling), rtx_group.cpp and
 * rtx_anim_host.hip; the render kernel is rtx_hip.hip.
 */
#ifndef RTX_H_
#define RTX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTX_ABI_VERSION 2

enum {
    RTX_OK = 0,
    RTX_E_INVALID = -1,   /* bad argument / malformed scene                          */
    RTX_E_DEVICE = -2,    /* HIP runtime error (message in rtx_last_error)           */
    RTX_E_NOMEM = -3,     /* host or device allocation failed                       */
    RTX_E_STATE = -4,     /* e.g. rtx_render before rtx_upload_scene                 */
    RTX_E_UNSUPPORTED = -5
};

/* dae::TriangleCullMode (source/DataTypes.h:29-34), same enumerator order */
enum { RTX_CULL_FRONT = 0, RTX_CULL_BACK = 1, RTX_CULL_NONE = 2 };
/* dae::LightType (source/DataTypes.h:522-526) */
enum { RTX_LIGHT_POINT = 0, RTX_LIGHT_DIRECTIONAL = 1 };
/* Renderer::LightingMode (source/Renderer.h:40-48), same enumerator order */
enum {
    RTX_MODE_OBSERVED_AREA = 0,
    RTX_MODE_RADIANCE = 1,
    RTX_MODE_BRDF = 2,
    RTX_MODE_COMBINED = 3,
    RTX_MODE_COUNT = 4
};
/* Material subclasses of source/Material.h */
enum {
    RTX_MAT_SOLID_COLOR = 0,   /* Material_SolidColor    Material.h:34-48   */
    RTX_MAT_LAMBERT = 1,       /* Material_Lambert       Material.h:54-68   */
    RTX_MAT_LAMBERT_PHONG = 2, /* Material_LambertPhong  Material.h:74-94   */
    RTX_MAT_COOK_TORRANCE = 3  /* Material_CookTorrence  Material.h:99-129  */
};

typedef struct rtx_sphere {
    float origin[3];
    float radius;
    uint8_t material;
    uint8_t _pad[3];
} rtx_sphere;

typedef struct rtx_plane {
    float origin[3];
    float normal[3];
    uint8_t material;
    uint8_t _pad[3];
} rtx_plane;

/* One node of the reference's binned-SAH BVH.  `idx_count` and `first_idx` count
 * INDICES (3 per triangle), leaf iff idx_count > 0, right child = left_node + 1. */
typedef struct rtx_bvh_node {
    float min[3];
    float max[3];
    uint32_t first_idx;
    uint32_t idx_count;
    uint32_t left_node;
} rtx_bvh_node;

/* A TriangleMesh after UpdateTransforms()/BuildBVH() (source/DataTypes.h:109-236):
 * world-space positions, the BVH-permuted index array, per-triangle world normals
 * (transformedNormals, indexed by index/3) and the node array (nodesUsed entries). */
typedef struct rtx_mesh {
    const float* positions;   /* 3 * n_positions floats (transformedPositions) */
    uint32_t n_positions;
    const int32_t* indices;   /* n_indices = 3 * triangles                    */
    uint32_t n_indices;
    const float* normals;     /* 3 * (n_indices / 3) floats (transformedNormals) */
    const rtx_bvh_node* nodes;
    uint32_t n_nodes;
    int32_t cull_mode;        /* RTX_CULL_*                                   */
    uint8_t material;
    uint8_t _pad[3];
} rtx_mesh;

typedef struct rtx_light {
    float origin[3];
    float direction[3];
    float color[3];
    float intensity;
    int32_t type;             /* RTX_LIGHT_* */
} rtx_light;

/* Flattened Material.  Field use per kind:
 *   SOLID_COLOR   : color
 *   LAMBERT       : color (diffuse colour), kd
 *   LAMBERT_PHONG : color, kd, ks, exponent
 *   COOK_TORRANCE : color (albedo), metalness, roughness                         */
typedef struct rtx_material {
    int32_t kind;
    float color[3];
    float kd;
    float ks;
    float exponent;
    float metalness;
    float roughness;
} rtx_material;

typedef struct rtx_scene {
    const rtx_sphere* spheres;     uint32_t n_spheres;
    const rtx_plane* planes;       uint32_t n_planes;
    const rtx_mesh* meshes;        uint32_t n_meshes;
    const rtx_light* lights;       uint32_t n_lights;
    const rtx_material* materials; uint32_t n_materials;
} rtx_scene;

/* Camera after Camera::CalculateCameraToWorld() (source/Camera.h:43-53): the rows of
 * cameraToWorld, the ray origin and fov = tanf(fovAngle*TO_RADIANS/2) (Camera.h:55-59). */
typedef struct rtx_camera {
    float origin[3];
    float right[3];
    float up[3];
    float forward[3];
    float fov;
} rtx_camera;

/* SDL_MapRGB for a palette-less 8-bit-per-channel surface:
 * pixel = r<<rshift | g<<gshift | b<<bshift | amask.  XRGB8888 = {16, 8, 0, 0}. */
typedef struct rtx_pixel_format {
    uint32_t rshift, gshift, bshift, amask;
} rtx_pixel_format;

/* Per-frame parameters (the Renderer's state: m_Width/m_Height, m_CurrentLightingMode,
 * m_ShadowsEnabled — source/Renderer.h:40-61) plus the image partition for multi-GPU:
 * rows are grouped in stripes of `stripe_rows`; this call renders stripe s iff
 * s % stripe_step == stripe_first.  stripe_rows = 0 means "the whole image". */
typedef struct rtx_render_params {
    uint32_t width, height;
    int32_t lighting_mode;        /* RTX_MODE_* (default RTX_MODE_COMBINED) */
    int32_t shadows_enabled;      /* 0/1 (default 1)                         */
    rtx_pixel_format format;
    uint32_t stripe_rows;
    uint32_t stripe_first;
    uint32_t stripe_step;
} rtx_render_params;

typedef struct rtx_ctx rtx_ctx;

/* ---- device context (librtx_hip.so) ------------------------------------------- */
int rtx_abi_version(void);
/* Bind a context to HIP device `device_id` (one context per GPU; one process per GPU
 * is the supported multi-GPU model).  Creates its own non-blocking stream. */
int rtx_create(rtx_ctx** out, int device_id);
void rtx_destroy(rtx_ctx* ctx);
/* Reason for the last error on `ctx`; with ctx == NULL, why the calling thread's last
 * rtx_create failed. */
const char* rtx_last_error(const rtx_ctx* ctx);
/* Copy the caller-owned scene into HBM (device layout of DESIGN.md §3).  The caller
 * may free its arrays afterwards.  Re-call after an animated Scene::Update. */
int rtx_upload_scene(rtx_ctx* ctx, const rtx_scene* scene);
/* Blocking frame render, like Renderer::Render: renders the rows selected by
 * `params` and writes them into the caller's host buffers (row-major, pitch = width
 * pixels; rows this call does not own are left untouched).  out_rgb (3 floats per
 * pixel, post-MaxToOne colour) may be NULL. */
int rtx_render(rtx_ctx* ctx, const rtx_camera* cam, const rtx_render_params* params,
               uint32_t* out_pixels, float* out_rgb);
/* Asynchronous variant for device-resident pipelines: renders into the context's HBM
 * frame buffer on the context stream and returns immediately. */
int rtx_render_async(rtx_ctx* ctx, const rtx_camera* cam, const rtx_render_params* params,
                     int want_rgb);
/* Multi-view batch (one launch): renders n_views (1..8) cameras of the same scene into
 * consecutive frame buffers (view v at offset v*width*height).  With stripes, view v
 * owns the stripes s with s % stripe_step == (stripe_first - v) mod stripe_step, so N
 * ranks with stripe_first = rank and stripe_step = N cover every view exactly once with
 * the same number of rows each (the weak-scaling partition of bench.py). */
int rtx_render_views_async(rtx_ctx* ctx, const rtx_camera* cams, int n_views,
                           const rtx_render_params* params, int want_rgb);
/* Supersampled anti-aliasing: every later frame of `ctx` (rtx_render*, rtx_time_*, rtx_count_work*)
 * takes k x k samples per pixel, k in {1, 2, 4, 8} (1 = one ray through the pixel centre, the
 * default).  Sample (X, Y) is pixel (X, Y) of the reference's k*width x k*height frame, up to and
 * including MaxToOne; pixel (x, y) is the box filter of the samples (k x + sx, k y + sy): per channel
 * the fp32 sum as an adjacent-pair tree over sx, then over sy, times 1/(k*k).  The render kernel
 * resolves it, so the frame buffer, the downloads and the stripes stay width x height; k*width and
 * k*height may not exceed 65536 (rtx_render* then returns RTX_E_INVALID).  Any other k returns
 * RTX_E_INVALID and leaves the factor as it was.  The work counters count the sample frame. */
int rtx_set_supersample(rtx_ctx* ctx, uint32_t k);
/* Adaptive supersampling: k x k samples for the pixels that alias only.  For a width x height frame, a
 * factor k in {2, 4, 8} and a threshold tau in [0, 255]:
 *   P  is the plain frame, what rtx_render gives with factor 1.
 *   S  is the supersampled frame of factor k exactly as rtx_set_supersample defines it: sample
 *      (k x + sx, k y + sy) is the reference's pixel of the k*width x k*height frame; per channel the
 *      adjacent-pair tree over sx, then over sy, times 1/(k*k); then the 8-bit quantisation with
 *      params->format.
 *   Channel c of a pixel word is (word >> shift_c) & 255 with params->format.
 *   E(x, y) holds iff some 4-neighbour (x +- 1, y) or (x, y +- 1) inside the frame has
 *      |c(P(x, y)) - c(P(neighbour))| > tau for some channel c: integer only, symmetric (both pixels
 *      of a pair are refined), and independent of the colour plane.
 *   The adaptive frame is A = S where E holds, else P, in both planes.
 * tau = 255 gives P; a tau that puts every pixel in E gives S.  The mask comes from the device's own P:
 * the reference's P bit for bit wherever the reference calls no powf, the device's words elsewhere.
 *
 * rtx_render_adaptive_async queues the plain frame exactly as rtx_render_async does (it is a frame for
 * the schedule and every policy), then, behind a pending split chain, the classification of the frame
 * buffer and the refinement of the classified pixels, and returns; nothing waits on the host, and the
 * number of refined pixels never leaves the device.  Afterwards the frame buffer holds A, and the
 * last-frame record is the plain frame's: rtx_download, rtx_gather_async and rtx_device_buffers work
 * unchanged.  The hit-pass planes and their record are not touched.  rtx_render_adaptive is the async
 * call followed by rtx_download.  rtx_adaptive_refined waits for the context stream and gives |E| of
 * the last adaptive frame.
 * Errors (the context renders on after each): k not 2, 4 or 8, threshold > 255, anything rtx_render
 * rejects, k*width or k*height above 65536: RTX_E_INVALID; no scene uploaded (for rtx_adaptive_refined:
 * no adaptive frame yet): RTX_E_STATE; a supersample factor other than 1 on the context (the mode
 * carries its own) and stripe_step > 1 (a stripe's neighbour rows belong to another context):
 * RTX_E_UNSUPPORTED.  Views, rtx_group_* and stripes have no adaptive form. */
int rtx_render_adaptive_async(rtx_ctx* ctx, const rtx_camera* cam, const rtx_render_params* params,
                              int want_rgb, uint32_t k, uint32_t threshold);
int rtx_render_adaptive(rtx_ctx* ctx, const rtx_camera* cam, const rtx_render_params* params,
                        uint32_t k, uint32_t threshold, uint32_t* out_pixels, float* out_rgb);
/* waits for the context stream; the number of refined pixels (|E|) of the last adaptive frame */
int rtx_adaptive_refined(rtx_ctx* ctx, uint32_t* n_refined);
int rtx_synchronize(rtx_ctx* ctx);
/* Copy the context's frame buffer (rows owned by the last render) to host memory. */
int rtx_download(rtx_ctx* ctx, uint32_t* out_pixels, float* out_rgb);
/* Host gather of one partition: queue, on the context stream, the D2H copy
 * of the rows the last render owns into the caller's FULL-FRAME host buffers (row-major,
 * pitch = width; one hipMemcpy2DAsync per view and plane for a striped render) and
 * return.  Rows the context does not own are never written, so several contexts (GPUs,
 * or processes sharing one mapping) can gather disjoint stripes into one frame.  Truly
 * asynchronous only for page-locked memory (rtx_host_register); complete after
 * rtx_synchronize. */
int rtx_gather_async(rtx_ctx* ctx, uint32_t* out_pixels, float* out_rgb);
/* Page-lock caller memory (e.g. a frame shared between the ranks' processes) for every
 * device of the process (hipHostRegister, portable), and undo it. */
int rtx_host_register(rtx_ctx* ctx, void* ptr, size_t bytes);
int rtx_host_unregister(rtx_ctx* ctx, void* ptr);
/* Device pointers of the HBM frame buffer (width*height uint32 / 3*width*height f32).  The
 * frames queued so far are complete in it after rtx_synchronize (a repeated frame may leave
 * its split launches running after rtx_render_async returns, on a stream of its own). */
int rtx_device_buffers(rtx_ctx* ctx, void** d_pixels, void** d_rgb);

/* ---- hit-record planes (AOVs): what each pixel's primary ray hit -------------------
 * The hit pass runs Scene::GetClosestHit (source/Scene.cpp:29-66) for every pixel's primary ray,
 * exactly as a colour frame does, and writes the closestHit record instead of shading it: no light
 * loop, no shadow rays, no colour.  Every plane is row-major width x height; view v starts at
 * v*width*height elements of the plane (3x that for the normal plane).  The values are the colour
 * frame's own, word for word the reference's record:
 *
 *   plane      type         hit                                             miss
 *   depth      float        closestHit.t                                    FLT_MAX (the empty HitRecord)
 *   normal     3 x float    closestHit.normal: a sphere's normalised as     0, 0, 0
 *                           Scene.cpp does, a plane's or triangle's copied
 *   material   uint32_t     closestHit.materialIndex                        0
 *   primitive  uint32_t     kind << 30 | index                              0
 *
 * kind: 1 = sphere, 2 = plane, 3 = triangle.  A sphere's or plane's index is its position in
 * rtx_scene::spheres / planes.  A triangle's is its position in the concatenation of the meshes'
 * `indices` arrays as uploaded: mesh 0's n_indices/3 triangles first, a mesh's triangle k being its
 * indices 3k .. 3k+2.  After a device Update (rtx_anim_update) the order within a mesh is the one
 * rtx_anim_download returns. */
enum { RTX_AOV_DEPTH = 1, RTX_AOV_NORMAL = 2, RTX_AOV_MATERIAL = 4, RTX_AOV_PRIMITIVE = 8, RTX_AOV_ALL = 15 };
#define RTX_PRIM_KIND(p) ((uint32_t)(p) >> 30)
#define RTX_PRIM_INDEX(p) ((uint32_t)(p) & 0x3fffffffu)
typedef struct rtx_aov_planes {
    float* depth;
    float* normal;
    uint32_t* material;
    uint32_t* primitive;
} rtx_aov_planes;
/* Queue the hit pass of n_views (1..8) cameras on the context stream, into the context's HBM planes
 * named by `mask` (RTX_AOV_* bits; planes are allocated when a mask first names them).  Stripes and
 * views are exactly those of rtx_render_views_async; lighting_mode, shadows_enabled and format are
 * ignored.  The pass is ordered with the colour frames and uploads queued on the context before and
 * after it, writes nothing of the colour frame buffer and leaves the frame schedule as it was.
 * Errors (the context renders on after each): mask 0 or with unknown bits RTX_E_INVALID; no scene
 * RTX_E_STATE; a supersample factor other than 1 on the context (rtx_set_supersample)
 * RTX_E_UNSUPPORTED: a pixel's samples may hit different primitives, and an average of ids, or of
 * normals across them, means nothing. */
int rtx_render_aov_async(rtx_ctx* ctx, const rtx_camera* cams, int n_views, const rtx_render_params* params,
                         uint32_t mask);
/* Blocking: the pass of one camera, then rtx_download_aov into `out` (whose non-NULL members must be
 * planes of `mask`). */
int rtx_render_aov(rtx_ctx* ctx, const rtx_camera* cam, const rtx_render_params* params, uint32_t mask,
                   const rtx_aov_planes* out);
/* Copy the rows the last hit pass owns (every view) into the caller's full-frame planes and wait;
 * NULL members are skipped, one the last pass did not write returns RTX_E_STATE.  The context keeps
 * the last pass's size, views, stripes and mask beside the last colour frame's: rtx_download /
 * rtx_gather_async after a pass still copy the colour frame, and the reverse. */
int rtx_download_aov(rtx_ctx* ctx, const rtx_aov_planes* out);
/* The same copies queued on the context stream (rows the pass does not own are never written, like
 * rtx_gather_async); complete after rtx_synchronize. */
int rtx_gather_aov_async(rtx_ctx* ctx, const rtx_aov_planes* out);
/* Device pointers of the HBM planes (NULL for a plane no mask has named yet); the passes queued so
 * far are complete in them after rtx_synchronize. */
int rtx_device_aov_buffers(rtx_ctx* ctx, rtx_aov_planes* out);

/* ---- deferred shading: the colour of a stored hit pass, without tracing it again -------
 * rtx_shade_aov* runs everything after Scene::GetClosestHit of Renderer::RenderPixel
 * (source/Renderer.cpp:100-181) on the records the context's last hit pass stored, and writes the
 * colour frame buffer.  The pass supplies the size, the views, the stripes and the cameras (the
 * context keeps them); `params` supplies lighting_mode, shadows_enabled and format, and its size and
 * stripe fields are ignored.  The pass must have written all four planes (RTX_AOV_ALL).
 *
 * Per owned pixel the result is RenderPixel with closestHit taken from the planes: didHit =
 * (primitive != 0), t = the depth plane's value, normal the normal plane's, materialIndex the material
 * plane's, origin = ray.origin + t * ray.direction per component (one rounded multiply, one rounded
 * add: Utils.h:67, 92, 162), and ray the frame's primary ray of that pixel and view.  From
 * originOffset on it is the frame's code: the light loop in scene order, DoesHit, the mode's term,
 * shadowFactor, MaxToOne, the quantisation.
 *
 * Guarantee: while the geometry, the material indices and the cameras are those of the pass, the
 * frame buffer holds word for word, in both planes, what rtx_render_views_async with the pass's
 * cameras, size and stripes and these mode, shadows and format leaves there; so it is the reference's
 * frame bit for bit wherever the reference calls no powf.  Lights and material VALUES are read from
 * the scene uploaded at the time of the call: upload a scene with other lights or material values
 * (same geometry, same material indices) and shade again to relight the pass.  Geometry, material
 * indices or a device Update (rtx_anim_update) that changed since the pass give unspecified colours
 * (never an out-of-range load: the material index is clamped to the scene's); keeping them is the
 * caller's responsibility.
 *
 * Afterwards the last-frame record is the pass's shape: rtx_download, rtx_gather_async and
 * rtx_device_buffers work unchanged.  The call is no frame for the schedule or any policy (tile costs
 * and order, split rendering and its tuner, motion mode, frames in flight stay as they were; it only
 * reads the dispatch order of earlier frames of the same size, views and stripes, which changes no
 * pixel), reads the planes and their record only, and queues on the context stream, ordered with the
 * frames, passes, uploads and Updates before and after it.
 * Errors (the context keeps working after each): NULL ctx or params, a lighting mode or format
 * rtx_render rejects: RTX_E_INVALID; no scene, no pass yet, a last pass whose mask is not
 * RTX_AOV_ALL, or a scene that now has fewer materials than at the time of the pass: RTX_E_STATE; a
 * supersample factor other than 1 on the context: RTX_E_UNSUPPORTED.  rtx_download of out_rgb after
 * want_rgb == 0 returns RTX_E_STATE, as after a frame. */
int rtx_shade_aov_async(rtx_ctx* ctx, const rtx_render_params* params, int want_rgb);
/* Blocking: the call above, then rtx_download into the caller's full-frame buffers (out_rgb may be
 * NULL). */
int rtx_shade_aov(rtx_ctx* ctx, const rtx_render_params* params, uint32_t* out_pixels, float* out_rgb);

/* ---- relighting: a hit pass's shadow rays stored once, then shaded with no tracing ------
 * A shadow ray depends only on the hit record and on the light's origin and type
 * (LightUtils::GetDirectionToLight, Utils.h:341-353, is light.origin - origin for both types).  So a
 * change of light colours or intensities, of any material value, of the lighting mode, of the shadow
 * toggle or of the pixel format leaves every Scene::DoesHit result as it was.  The shadow pass stores
 * those results beside the hit pass; the relight shades hit pass + results without casting a ray.
 *
 * rtx_render_shadows_async runs on the records of the context's last hit pass, which must have written
 * all four planes (RTX_AOV_ALL); size, views, stripes and cameras are the pass's, as for rtx_shade_aov*.
 * It writes one uint32_t per owned pixel into the shadow plane in HBM, view v at v * width * height:
 *     bit l = didHit && Scene::DoesHit(Ray{originOffset, directionToLight_l, 0.0001f, |l|})
 * the test of Renderer.cpp:130-141 for light l, with the hit taken from the planes as rtx_shade_aov
 * takes it (originOffset = origin + normal * 0.0001f).  Every light's bit is defined (the reference's
 * `continue` skips the shading, not the later lights); bits >= the scene's light count are 0, and so
 * is a miss's word.  The walk is the one the frame's shadow rays take for the scene.  The context
 * records which hit pass the plane belongs to (every hit pass makes an earlier plane stale) and the
 * lights it was traced for: their count, and each one's origin and type, bit for bit.
 * It is no frame for the schedule or any policy, reads the frames' dispatch order as rtx_shade_aov
 * does, and queues on the context stream.
 * Errors (the context keeps working after each): NULL ctx: RTX_E_INVALID; no scene, no hit pass yet or
 * a last pass whose mask is not RTX_AOV_ALL: RTX_E_STATE; a supersample factor other than 1, or a scene
 * with more than 32 lights: RTX_E_UNSUPPORTED. */
int rtx_render_shadows_async(rtx_ctx* ctx);
/* The plane, by the rules of the hit pass's copies (rtx_download_aov, rtx_gather_aov_async,
 * rtx_device_aov_buffers): `out` is a full-frame array of width * height * views words of which only
 * the rows the pass owns are written; download blocks, gather queues the copy on the context stream.
 * NULL ctx or out: RTX_E_INVALID; no shadow pass yet, or a hit pass since: RTX_E_STATE.  The device
 * pointer (NULL before the first shadow pass) stays valid until a larger pass or rtx_destroy; the
 * passes queued so far are complete in it after rtx_synchronize. */
int rtx_download_shadows(rtx_ctx* ctx, uint32_t* out);
int rtx_gather_shadows_async(rtx_ctx* ctx, uint32_t* out);
int rtx_device_shadow_buffer(rtx_ctx* ctx, uint32_t** d);

/* ---- incremental shadow pass: re-trace only the lights that moved ---------------------------
 * Bit l of a pixel's word depends only on the stored hit record and on light l's origin and type, so a
 * light that moved invalidates its own bit and no other.  The two calls below are the shadow pass over
 * a subset of the lights: the same checks in the same order, the same shape, views, stripes and
 * cameras, the same walk and kernel, no frame for any policy, nothing of the colour frame buffer or of
 * the hit planes written.  They differ from rtx_render_shadows_async in the lights traced and in how
 * the word is stored.  For every owned pixel
 *     new = (old & keep) | traced
 * where bit l of `traced` is the shadow pass's bit l for the scene uploaded now when l is in the trace
 * mask (0 otherwise), and `keep` holds the bits below the uploaded light count that are not traced and
 * were valid before.  Rows the pass does not own are not touched.  The full pass is keep = 0; it does
 * not read the plane.
 *
 * rtx_update_shadows_async traces the lights named in `lights` (bit l = light l).  It needs a current
 * plane (a shadow pass of the last hit pass) and an uploaded light count equal to the recorded one;
 * every light NOT named must have the recorded origin and type, bit for bit, so the plane is never
 * left silently stale.  A named light whose key did not change is traced again (the same word).
 * lights == 0 with nothing changed launches nothing.  On success the recorded lights become the
 * uploaded ones, and rtx_relight* with shadows on is accepted.
 * Errors (the plane and its record are then as before): those of rtx_render_shadows_async in its order;
 * then no shadow pass yet, a hit pass newer than the plane, a changed light count, or a light outside
 * `lights` whose origin or type changed (the message names the first): RTX_E_STATE; a bit of `lights`
 * at or above the light count: RTX_E_INVALID.
 *
 * rtx_refresh_shadows_async makes the plane valid for the uploaded lights at the least cost.  Without a
 * current plane (none yet, a newer hit pass, a larger pass) it is the full pass and *traced is the mask
 * of all lights.  Otherwise the lights whose origin or type differ from the recorded ones, and the
 * lights at or above the recorded count (appended), are traced in one launch and *traced is their
 * mask; the bits of removed trailing lights are cleared by the same launch (one with an empty trace
 * mask when nothing else changed).  Nothing to trace and nothing to clear: no launch, *traced = 0.
 * `traced` may be NULL.  Errors: those of rtx_render_shadows_async. */
int rtx_update_shadows_async(rtx_ctx* ctx, uint32_t lights);
int rtx_refresh_shadows_async(rtx_ctx* ctx, uint32_t* traced);

/* rtx_relight* is rtx_shade_aov* with DoesHit answered by the shadow plane: `params` supplies
 * lighting_mode, shadows_enabled and format (its size and stripe fields are ignored), the hit pass
 * everything else.  Per owned pixel the result is Renderer::RenderPixel from originOffset on
 * (Renderer.cpp:126-181), the hit rebuilt from the planes as rtx_shade_aov rebuilds it; with shadows
 * on, light l is occluded when bit l of the pixel's word is set; with shadows off the plane is neither
 * read nor required.  It writes the colour frame buffer and sets the last-frame record to the pass's
 * shape, so rtx_download, rtx_gather_async and rtx_device_buffers work unchanged.
 *
 * Guarantee: while the geometry, the material indices, the cameras and the lights' count, origins and
 * types are those of the two passes, the frame buffer holds word for word, in both planes, what
 * rtx_render_views_async leaves there for the pass's cameras, size and stripes and these mode, shadows
 * and format; so it is the reference's frame bit for bit wherever the reference calls no powf.  Light
 * colours and intensities and material VALUES are read from the scene uploaded at the time of the
 * call: upload, relight, upload, relight is the relighting loop, each step one pass over the planes.
 * The host checks the lights (below); changed geometry, material indices or a device Update since the
 * passes are the caller's responsibility, exactly as for rtx_shade_aov (colours unspecified, loads in
 * range).
 *
 * The call is no frame for the schedule or any policy, casts no ray, and queues on the context
 * stream, behind a pending split chain.
 * Errors: those of rtx_shade_aov, and with shadows_enabled: no shadow pass yet, a hit pass newer than
 * the shadow plane, or uploaded lights whose count, or any origin or type, differ bitwise from the
 * recorded ones: RTX_E_STATE. */
int rtx_relight_async(rtx_ctx* ctx, const rtx_render_params* params, int want_rgb);
/* Blocking: the call above, then rtx_download into the caller's full-frame buffers (out_rgb may be
 * NULL). */
int rtx_relight(rtx_ctx* ctx, const rtx_render_params* params, uint32_t* out_pixels, float* out_rgb);

/* ---- resolved relighting: anti-aliased frames from a stored sample pass -------------------------
 * rtx_set_supersample defines sample (X, Y) of a width x height frame as pixel (X, Y) of the reference's
 * k*width x k*height frame.  So a hit pass of Ws x Hs = k*W x k*H pixels, taken on a context whose own
 * supersample factor is 1, IS the sample pass of the W x H frame; the shadow pass and its incremental
 * updates run on it unchanged.  rtx_relight_resolve* reads the context's last hit pass that way: every
 * sample is shaded exactly as rtx_relight* shades a pixel of the Ws x Hs pass (up to and including
 * MaxToOne), and pixel (x, y) of view v is the box filter of rtx_set_supersample over the samples
 * (k x + sx, k y + sy): per channel the fp32 sum as an adjacent-pair tree over sx, then over sy, times
 * 1/(k*k); then the quantisation with params->format.  `params` supplies lighting_mode, shadows_enabled
 * and format (its size and stripe fields are ignored); the pass supplies cameras, views, size and stripes.
 *
 * Guarantee: while the geometry, the material indices, the cameras and the lights' count, origins and
 * types are those of the passes, the frame buffer holds word for word, in both planes, what
 * rtx_set_supersample(ctx, k) followed by rtx_render_views_async leaves there for the pass's cameras at
 * W x H with the stripes {stripe_rows / k, stripe_first, stripe_step} and these mode, shadows and format;
 * so it is the resolved reference frame bit for bit wherever the reference calls no powf.  Light colours
 * and intensities and material VALUES are read from the scene uploaded at the time of the call, as by
 * rtx_relight*: a colour, intensity, material, mode or shadow-toggle change of an anti-aliased frame is
 * one pass over the planes, and a moved light its own shadow rays (rtx_refresh_shadows_async) on top.
 *
 * Afterwards the last-frame record is W x H, the pass's views, and the stripes {stripe_rows / k,
 * stripe_first, stripe_step} (stripe_rows 0 for an unstriped pass, whose own value means nothing):
 * rtx_download, rtx_gather_async and rtx_device_buffers work unchanged, and
 * the frame buffer holds W*H*views pixels.  An output row is owned exactly when its k sample rows are.
 * The call is no frame for the schedule or any policy, casts no ray, only reads the hit planes, the
 * shadow plane and their records, and queues on the context stream, behind a pending split chain.
 * Errors, in this order (the context keeps working after each): NULL ctx or params, k not 2, 4 or 8:
 * RTX_E_INVALID; everything rtx_relight_async checks, in its order and with its codes (among them a
 * supersample factor other than 1 on the context: RTX_E_UNSUPPORTED, the mode carries its own); Ws or
 * Hs not divisible by k: RTX_E_INVALID; a striped pass (stripe_step > 1) whose stripe_rows is no
 * multiple of 16*k, so that the output stripes would be no legal frame shape: RTX_E_UNSUPPORTED. */
int rtx_relight_resolve_async(rtx_ctx* ctx, const rtx_render_params* params, uint32_t k, int want_rgb);
/* Blocking: the call above, then rtx_download into the caller's full-frame W x H buffers (out_rgb may be
 * NULL; out_pixels == NULL: RTX_E_INVALID). */
int rtx_relight_resolve(rtx_ctx* ctx, const rtx_render_params* params, uint32_t k, uint32_t* out_pixels,
                        float* out_rgb);

/* ---- scene edits: lights and materials changed in place ---------------------------------------
 * The relighting loop changes 32 bytes of a light or 48 of a material; rtx_upload_scene packs and copies
 * the whole scene for that.  An edit replaces records of the CURRENT scene image in place, on the context
 * stream, behind a pending split chain and ordered with every frame, pass, query and Update queued before
 * and after it, without waiting on the host.  After any sequence of edits every entry point behaves word
 * for word as if the scene with those records replaced had been given to rtx_upload_scene.
 *
 * rtx_edit_lights: lights first .. first+n-1 take the given origin, color and intensity (`direction` is
 * ignored: the device record never carried it).  `type` must be the uploaded light's.  A light whose
 * origin bits did not change is a value edit of its own two records.  A moved light also renews what the
 * upload derives from light origins: the room-skip record and fact (rtx_room_info; it can flip either
 * way), the light's cull bound and its exact-cull anchor records (the camera anchors stay valid), and the
 * light's key for the shadow plane: rtx_relight* with shadows on then refuses until
 * rtx_update_shadows_async or rtx_refresh_shadows_async has run, and the refresh traces exactly the
 * moved lights.
 * rtx_edit_materials: materials first .. first+n-1 take the given values; `kind` must be the uploaded one.
 *
 * The _device forms read VALUES from device memory of the context's device (queued, returning at once;
 * the memory must stay valid until the stream reaches the edit): per light 4 floats {color[3],
 * intensity}, per material 8 floats {color[3], kd, ks, exponent, metalness, roughness}.  They cannot move
 * a light or change a kind, so no host state changes; the image is the host form's bit for bit for every
 * finite value.
 *
 * An edit is no upload for any policy: the tile schedule and costs, the split tuner, the refinement, motion
 * mode and the cull worth cache stay as they were.
 * Errors, in this order (the context keeps working after each, and a refused edit changes nothing): NULL
 * ctx, NULL records with n > 0, first + n above the uploaded count: RTX_E_INVALID; no scene uploaded:
 * RTX_E_STATE; a changed type or kind (the first is named in rtx_last_error), or a context whose current
 * image belongs to a device Update's registration (rtx_anim_create): RTX_E_UNSUPPORTED.  n == 0 returns
 * RTX_OK and launches nothing.  Adding or removing records, type and kind changes, and sphere, plane or
 * mesh edits are uploads. */
int rtx_edit_lights(rtx_ctx* ctx, uint32_t first, uint32_t n, const rtx_light* lights);
int rtx_edit_materials(rtx_ctx* ctx, uint32_t first, uint32_t n, const rtx_material* materials);
int rtx_edit_light_values_device(rtx_ctx* ctx, uint32_t first, uint32_t n, const float* d_values);
int rtx_edit_material_values_device(rtx_ctx* ctx, uint32_t first, uint32_t n, const float* d_values);

/* ---- ray queries: closest hit and occlusion for caller-supplied rays ---------------
 * The traversal behind a frame's rays, for rays the caller makes: a line-of-sight test, a pick ray,
 * visibility from surface points, a bounce, a custom camera.
 *
 * A ray is eight floats and nothing about it is interpreted.  The library builds the reference's
 * dae::Ray{origin, direction, min, max} (DataTypes.h:539-565) from them as its constructor does,
 * inversedDir = 1 / direction per component, and runs the reference's function on it.  It does not
 * normalise the direction (t is in units of its length) and validates nothing: the result for a zero,
 * denormal, huge, infinite or NaN component, for tmin <= 0, for tmax < tmin and for a tmax of FLT_MAX
 * or inf is whatever the reference computes for that ray.  The tolerance is zero: every output word
 * is the reference's, except that a NaN float may be any NaN.
 *
 * Errors (the context keeps working after each): NULL ctx, or NULL rays / out with n > 0, mask 0 or
 * with unknown bits, or a non-NULL plane of `out` that `mask` does not name: RTX_E_INVALID; no scene
 * uploaded: RTX_E_STATE.  n == 0 returns RTX_OK and launches nothing.
 *
 * A query is queued on the context stream behind a pending split chain, like the hit pass, and is
 * ordered with the frames, passes, uploads and device Updates queued on the context before and after
 * it: a query after rtx_upload_scene or rtx_anim_update sees the new geometry.  It reads and writes
 * nothing of the colour frame buffer, the hit-pass planes and their last-pass record, or the frame
 * schedule; a supersample factor on the context does not matter (queries are not frames).  Rays are
 * dispatched in the caller's order, 64 consecutive rays to a wave: coherent neighbours are faster,
 * and the library neither sorts nor compacts them. */
typedef struct rtx_ray { float origin[3]; float direction[3]; float tmin, tmax; } rtx_ray;   /* 32 B */
/* Scene::GetClosestHit (Scene.cpp:29-66) on each ray: element i of every plane of `mask` (3 floats for
 * the normal) is ray i's record in the hit pass's terms (rtx_aov_planes above: depth = t or FLT_MAX,
 * normal, material, primitive = kind << 30 | index; a miss is FLT_MAX / 0,0,0 / 0 / 0).  Host pointers;
 * staged through buffers of the context that grow on demand; returns when `out` is filled. */
int rtx_trace_rays(rtx_ctx* ctx, const rtx_ray* rays, uint32_t n, uint32_t mask, const rtx_aov_planes* out);
/* Scene::DoesHit (Scene.cpp:68-96) on each ray: out[i] = 1 if anything lies in [tmin, tmax] as DoesHit
 * decides it (the any-hit front/back cull swap of Utils.h:114-127 included), else 0. */
int rtx_occluded(rtx_ctx* ctx, const rtx_ray* rays, uint32_t n, uint8_t* out);
/* The same two with DEVICE pointers (of the context's device), queued on the context stream and
 * returning at once; complete after rtx_synchronize.  The caller makes the rays visible before the
 * call and keeps every buffer alive until then. */
int rtx_trace_rays_device(rtx_ctx* ctx, const rtx_ray* d_rays, uint32_t n, uint32_t mask, const rtx_aov_planes* d_out);
int rtx_occluded_device(rtx_ctx* ctx, const rtx_ray* d_rays, uint32_t n, uint8_t* d_out);

/* ---- shaded rays: the reference's pixel for caller-supplied rays ---------------------
 * Everything of Renderer::RenderPixel after the primary ray (Renderer.cpp:116-181), for rays the caller
 * makes: a fisheye, orthographic or panoramic camera, a lens with depth of field, a jittered or foveated
 * sample pattern, a mirror bounce built from the hit pass's normal, a probe at a surface point.
 *
 * For ray i the result is RenderPixel's with two changes: viewRay is the dae::Ray built from the eight
 * floats exactly as rtx_trace_rays builds it (nothing normalised or validated, tmin / tmax as given), and
 * viewDirection is that ray's direction as given, so Material::Shade receives -direction whatever its
 * length.  From there it is the reference statement for statement: GetClosestHit; originOffset =
 * hit.origin + hit.normal * 0.0001f; per light in scene order GetDirectionToLight, Normalize and, with
 * shadows on, DoesHit(Ray{originOffset, l, 0.0001f, |l|}) then shadowFactor *= 0.95f; the lighting mode's
 * term; finalColor *= shadowFactor; MaxToOne; the 8-bit quantisation and SDL_MapRGB with params->format.
 * A miss, and any ray of a scene without lights, is black.
 *
 * `params` supplies lighting_mode, shadows_enabled and format; width, height and the stripe fields are
 * ignored.  out_pixels[i] is ray i's pixel word, out_rgb[3i .. 3i + 2] its colour before quantisation;
 * either may be NULL (not asked for, never touched), not both.
 *
 * Tolerance: every output word is the reference's (a NaN float may be any NaN) wherever the reference
 * calls no powf: the modes ObservedArea and Radiance on every scene, and every mode on scenes without
 * Phong or Cook-Torrance materials.  In Combined and BRDF on scenes with such materials the bound is the
 * frames' (1e-4 per colour channel, 1 LSB per 8-bit channel), claimed for rays with a unit-length
 * direction; for other directions the output is defined by the text above without a stated bound.
 *
 * Errors (the context keeps working after each): NULL ctx, NULL rays with n > 0, NULL params, both
 * outputs NULL with n > 0, a lighting mode or pixel format rtx_render would reject: RTX_E_INVALID; no
 * scene uploaded: RTX_E_STATE.  n == 0 returns RTX_OK and launches nothing.
 *
 * Queuing, ordering and isolation are the ray queries' (above): behind a pending split chain, ordered
 * with the frames, passes, uploads and device Updates on the context, nothing of the frame buffer, the
 * hit-pass planes, the last-frame and last-pass records or the frame schedule is read or written, and a
 * supersample factor does not matter.  Rays are dispatched in the caller's order, 64 to a wave.
 * rtx_shade_rays takes host pointers, stages through the queries' buffer and returns when the outputs
 * are filled; rtx_shade_rays_device takes DEVICE pointers, is queued and returns at once (complete after
 * rtx_synchronize).  To get the hit record as well, call rtx_trace_rays on the same rays. */
int rtx_shade_rays(rtx_ctx* ctx, const rtx_ray* rays, uint32_t n, const rtx_render_params* params,
                   uint32_t* out_pixels, float* out_rgb);
int rtx_shade_rays_device(rtx_ctx* ctx, const rtx_ray* d_rays, uint32_t n, const rtx_render_params* params,
                          uint32_t* d_pixels, float* d_rgb);

/* ---- one frame over several GPUs from one process ------------------
 * The reference's Renderer::Render covers the frame with parallel_for
 * (source/Renderer.cpp:79-85); a group covers it with G render contexts instead.  Rows are
 * dealt in `stripe_rows`-row stripes round robin (member i owns stripe s iff s % G == i);
 * each member has its own host thread and stream, renders its stripes and gathers them
 * straight into the caller's host frame (rtx_gather_async).  rtx_group_render blocks until
 * the whole frame is in out_pixels / out_rgb; the result is bit-identical to one
 * context's rtx_render.  Device ids may repeat (several contexts on one GPU). */
#define RTX_GROUP_MAX 64
typedef struct rtx_group rtx_group;
int rtx_group_create(rtx_group** out, const int* device_ids, int n);
void rtx_group_destroy(rtx_group* group);
/* Reason for the group's last error; with NULL, why this thread's last create failed. */
const char* rtx_group_last_error(const rtx_group* group);
int rtx_group_size(const rtx_group* group);
/* Member i's context (owned by the group), e.g. for rtx_time_frames on its stripes. */
rtx_ctx* rtx_group_context(rtx_group* group, int i);
int rtx_group_upload_scene(rtx_group* group, const rtx_scene* scene);
/* params: stripe_rows = stripe height (multiple of 16; 0 = 16); stripe_step must be 0/1
 * (the group assigns the stripes).  out_pixels: width*height uint32; out_rgb may be NULL. */
int rtx_group_render(rtx_group* group, const rtx_camera* cam, const rtx_render_params* params,
                     uint32_t* out_pixels, float* out_rgb);
/* rtx_set_supersample on every member (stripes stay rows of the width x height frame). */
int rtx_group_set_supersample(rtx_group* group, uint32_t k);
/* The hit pass (rtx_render_aov) over the group's members, the stripes dealt as rtx_group_render deals
 * them; blocks until every non-NULL plane of `out` (planes of `mask`) is complete. */
int rtx_group_render_aov(rtx_group* group, const rtx_camera* cam, const rtx_render_params* params, uint32_t mask,
                         const rtx_aov_planes* out);

/* ---- animated meshes: Scene::Update on the device -------------------
 * Replaces, per animated frame, the host's TriangleMesh::UpdateTransforms + BuildBVH
 * (source/DataTypes.h:210-236, 294-483, called from Scene_W4_*::Update, Scene.cpp:391-400,
 * 431-437, 468-474) followed by rtx_upload_scene: the transform, the reference's binned-SAH
 * rebuild (bit-identical node array and triangle permutation, which the next Update starts
 * from) and the scene image are produced in HBM by one workgroup per mesh. */
/* The object-space state UpdateTransforms starts from: positions (never permuted), the
 * per-triangle normals and the index array in the order the last BuildBVH left them. */
typedef struct rtx_mesh_source {
    const float* positions;   /* 3 * n_positions floats, object space                   */
    uint32_t n_positions;
    const float* normals;     /* 3 per triangle, object space (TriangleMesh::normals)    */
    const int32_t* indices;   /* n_indices = 3 * triangles                               */
    uint32_t n_indices;
} rtx_mesh_source;
typedef struct rtx_anim rtx_anim;
/* Register meshes mesh_ids[0..n) of `scene` (its current flattened state, what
 * rtx_upload_scene takes) as device-animated, with their object-space state src[0..n), and
 * upload the scene to `ctx` with rebuild-sized regions reserved for them.  n <= 32; the
 * meshes must be NaN-free, and the scene must render with the default-depth kernel (BVHs under
 * 64 levels; a rebuilt tree that deep is disabled in the image and reported, see
 * rtx_anim_status). */
int rtx_anim_create(rtx_anim** out, rtx_ctx* ctx, const rtx_scene* scene, const int32_t* mesh_ids,
                    const rtx_mesh_source* src, uint32_t n);
void rtx_anim_destroy(rtx_anim* anim);
/* Reason for the anim's last error; with NULL, why this thread's last create failed. */
const char* rtx_anim_last_error(const rtx_anim* anim);
/* One Update: registered mesh i gets finalTransform = transforms[16 i .. 16 i + 15] (the
 * reference's Matrix, data[0..3] row-major).  Queued on ctx's stream after the previous
 * update (whichever context on the anim's device ran it); frames rendered on ctx afterwards
 * see the new geometry.  Build errors are reported by rtx_anim_status. */
int rtx_anim_update(rtx_anim* anim, rtx_ctx* ctx, const float* transforms);
/* Waits for the last update.  status = {error bits (1: NaN vertex, 2: BVH too deep for the
 * render stack, 4: a build workgroup timed out waiting for a queue task; the frames
 * rendered from it are invalid), deepest level, nodesUsed, frontier parts}; returns
 * RTX_E_UNSUPPORTED when error bits are set. */
int rtx_anim_status(rtx_anim* anim, uint32_t i, uint32_t status[4]);
/* Waits for the last update and copies registered mesh i's state in the reference's own
 * form: transformedPositions (3V), indices (3T), normals (object space, 3T),
 * transformedNormals (3T), the node array pBVHNodes (3T entries).  NULL skips a part. */
int rtx_anim_download(rtx_anim* anim, uint32_t i, float* positions, int32_t* indices, float* normals,
                      float* transformed_normals, rtx_bvh_node* nodes);

#ifdef __cplusplus
}
#endif
#endif /* RTX_H_ */
