/*
 * rayq_ref.c — TEST INFRASTRUCTURE: ray queries (include/rtx.h: rtx_trace_rays, rtx_occluded) on the
 * CPU, the checker of tests/test_rayq_cpu.py and tests/test_gpu_rayq.py.
 *
 * It includes tests/aov_ref.c unchanged, which includes oracle/rtx_oracle.c unchanged.  A ray is the
 * eight floats of rtx_ray; per ray it builds the oracle's ray with mkray (the dae::Ray constructor:
 * inversedDir = 1 / direction) and calls the oracle's own closest_hit, and id_closest_hit of aov_ref.c
 * for the primitive id, failing if the tracked record differs from the oracle's in a bit (as
 * aov_ref_planes does); occlusion is the oracle's does_hit.  It also makes the two ray sets that tie the
 * queries to the renderer: a frame's primary rays and the shadow rays of its hits, statement for
 * statement as render_pixel forms them.
 */
#include "aov_ref.c"

static ray ray_of(const float* q) { return mkray(ld3(q), ld3(q + 3), q[6], q[7]); }

static void put_ray(float* q, v3 o, v3 d, float tmin, float tmax) {
    q[0] = o.x; q[1] = o.y; q[2] = o.z; q[3] = d.x; q[4] = d.y; q[5] = d.z; q[6] = tmin; q[7] = tmax;
}

/* Scene::GetClosestHit per ray: element i of the four planes.  Returns 0, or -(i + 1) of the first ray
 * where the id-tracking walk's record differs from closest_hit's. */
int rayq_ref_trace(const rtx_scene* sc, const float* rays, uint32_t n, float* depth, float* normal,
                   uint32_t* material, uint32_t* primitive) {
    for (uint32_t i = 0; i < n; ++i) {
        const ray r = ray_of(rays + 8 * (size_t)i);
        hitrec ch = empty_hit();
        closest_hit(sc, &r, &ch, NULL);
        idrec tr;
        tr.h = empty_hit();
        tr.id = 0;
        id_closest_hit(sc, &r, &tr);
        if (tr.h.did_hit != ch.did_hit || tr.h.mat != ch.mat || !same_bits(tr.h.t, ch.t) ||
            !same_bits(tr.h.normal.x, ch.normal.x) || !same_bits(tr.h.normal.y, ch.normal.y) ||
            !same_bits(tr.h.normal.z, ch.normal.z) || (ch.did_hit != 0) != (tr.id != 0))
            return -(int)(i + 1);
        depth[i] = ch.t;
        normal[3 * (size_t)i] = ch.normal.x; normal[3 * (size_t)i + 1] = ch.normal.y; normal[3 * (size_t)i + 2] = ch.normal.z;
        material[i] = ch.mat;
        primitive[i] = tr.id;
    }
    return 0;
}

/* Scene::DoesHit per ray */
void rayq_ref_occluded(const rtx_scene* sc, const float* rays, uint32_t n, uint8_t* out) {
    for (uint32_t i = 0; i < n; ++i) {
        const ray r = ray_of(rays + 8 * (size_t)i);
        out[i] = does_hit(sc, &r, NULL) ? 1 : 0;
    }
}

/* render_pixel's primary ray of pixel (px, py), statement for statement as aov_ref_planes forms it */
static ray primary_ray(const rtx_camera* cam, int W, int H, float aspect, uint32_t px, uint32_t py) {
    const float cx = (2.f * (((int)px + 0.5f) / W) - 1) * aspect * cam->fov;
    const float cy = (1.f - (2.f * ((int)py + 0.5f) / H)) * cam->fov;
    v3 vd = mk(cam->right[0] * cx + cam->up[0] * cy + cam->forward[0] * 1.f,
               cam->right[1] * cx + cam->up[1] * cy + cam->forward[1] * 1.f,
               cam->right[2] * cx + cam->up[2] * cy + cam->forward[2] * 1.f);
    normalize(&vd);
    return mkray(ld3(cam->origin), vd, 0.0001f, FLT_MAX);
}

/* The width x height primary rays of a frame, row-major. */
void rayq_ref_primary(const rtx_camera* cam, uint32_t width, uint32_t height, float* rays) {
    const int W = (int)width, H = (int)height;
    const float aspect = (int)width / (float)(int)height; /* Renderer.cpp:30, as run() */
    for (uint32_t py = 0; py < height; ++py)
        for (uint32_t px = 0; px < width; ++px) {
            const ray vr = primary_ray(cam, W, H, aspect, px, py);
            put_ray(rays + 8 * ((size_t)px + (size_t)py * (size_t)W), vr.o, vr.d, vr.tmin, vr.tmax);
        }
}

/* The renderer's shadow ray toward light `light` of every pixel whose primary ray hits, row-major in
 * the pixels that hit: {hit + n * 1e-4, normalised l, 1e-4, |l|} as render_pixel forms it.  `pixel[k]`
 * is ray k's pixel index; returns the number of rays (at most width x height). */
uint32_t rayq_ref_shadow(const rtx_scene* sc, const rtx_camera* cam, uint32_t width, uint32_t height, uint32_t light,
                         float* rays, uint32_t* pixel) {
    const int W = (int)width, H = (int)height;
    const float aspect = (int)width / (float)(int)height;
    uint32_t k = 0;
    if (light >= sc->n_lights) return 0;
    for (uint32_t py = 0; py < height; ++py)
        for (uint32_t px = 0; px < width; ++px) {
            const ray vr = primary_ray(cam, W, H, aspect, px, py);
            hitrec ch = empty_hit();
            closest_hit(sc, &vr, &ch, NULL);
            if (!ch.did_hit) continue;
            const v3 oo = add(ch.origin, scale(ch.normal, 0.0001f));
            v3 ld = dir_to_light(&sc->lights[light], oo);
            const float mag = normalize(&ld);
            put_ray(rays + 8 * (size_t)k, oo, ld, 0.0001f, mag);
            pixel[k] = px + py * width;
            ++k;
        }
    return k;
}
