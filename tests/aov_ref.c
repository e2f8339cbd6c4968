/*
 * aov_ref.c — TEST INFRASTRUCTURE: the hit-record planes of include/rtx.h (rtx_aov_planes) on the
 * CPU, the checker of tests/test_aov_cpu.py and tests/test_gpu_aov.py.
 *
 * It includes oracle/rtx_oracle.c unchanged: for every pixel it generates the primary ray exactly as
 * render_pixel does and calls the oracle's own closest_hit (the restatement pinned to the reference,
 * the shared scratch record of Scene.cpp:31 included), which gives t, normal, material and did_hit.
 * closest_hit does not say which primitive won, so a copy of the same walk that carries an id beside
 * every record names it.  The copy must reproduce closest_hit's record bit for bit for every pixel;
 * if it ever does not, aov_ref_planes returns the negated 1-based pixel index and the tests fail, so
 * the tracked walk cannot drift from the oracle.
 */
#include "../oracle/rtx_oracle.c"

typedef struct { hitrec h; uint32_t id; } idrec;   /* id: kind << 30 | index (rtx.h), 0 = none */

/* bvh_visit (closest-hit form) with the ids; tri0 = the mesh's first triangle in the scene's
 * concatenated order */
static void id_bvh_visit(const rtx_mesh* m, uint32_t tri0, uint32_t ni, const ray* r, int* didHit, idrec* hr,
                         idrec* cur) {
    const rtx_bvh_node* node = &m->nodes[ni];
    if (!slab(node->min, node->max, r)) return;
    if (node->idx_count > 0) {
        for (int idx = 0; idx < (int)node->idx_count; idx += 3) {
            const int li = (int)node->first_idx + idx;
            const v3 v0 = ld3(&m->positions[3 * m->indices[li]]);
            const v3 v1 = ld3(&m->positions[3 * m->indices[li + 1]]);
            const v3 v2 = ld3(&m->positions[3 * m->indices[li + 2]]);
            const v3 n = ld3(&m->normals[3 * (li / 3)]);
            if (hit_triangle(v0, v1, v2, n, m->cull_mode, m->material, r, &cur->h, 0)) {
                cur->id = (3u << 30) | (tri0 + (uint32_t)(li / 3));
                *didHit = 1;
                if (cur->h.t < hr->h.t) *hr = *cur;
            }
        }
    } else {
        id_bvh_visit(m, tri0, node->left_node, r, didHit, hr, cur);
        id_bvh_visit(m, tri0, node->left_node + 1, r, didHit, hr, cur);
    }
}

static int id_hit_mesh(const rtx_mesh* m, uint32_t tri0, const ray* r, idrec* hr) {
    idrec closest;
    closest.h = empty_hit();
    closest.id = 0;
    int didHit = 0;
    if (m->n_nodes == 0) return 0;
    id_bvh_visit(m, tri0, 0, r, &didHit, hr, &closest);
    return didHit;
}

/* closest_hit with the ids: every write of the scratch record writes its id too */
static void id_closest_hit(const rtx_scene* sc, const ray* r, idrec* closest) {
    idrec hr;
    hr.h = empty_hit();
    hr.id = 0;
    for (uint32_t i = 0; i < sc->n_spheres; ++i) {
        if (hit_sphere(&sc->spheres[i], r, &hr.h, 0)) {
            hr.id = (1u << 30) | i;
            if (hr.h.t < closest->h.t) { *closest = hr; normalize(&closest->h.normal); }
        }
    }
    for (uint32_t i = 0; i < sc->n_planes; ++i) {
        if (hit_plane(&sc->planes[i], r, &hr.h, 0)) {
            hr.id = (2u << 30) | i;
            if (hr.h.t < closest->h.t) *closest = hr;
        }
    }
    uint32_t tri0 = 0;
    for (uint32_t i = 0; i < sc->n_meshes; ++i) {
        if (id_hit_mesh(&sc->meshes[i], tri0, r, &hr)) {
            if (hr.h.t < closest->h.t) *closest = hr;
        }
        tri0 += sc->meshes[i].n_indices / 3;
    }
}

static int same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }

/* The four planes of the whole width x height frame (stripes ignored).  Returns 0, or -(pixel + 1)
 * of the first pixel where the tracked walk's record differs from closest_hit's. */
int aov_ref_planes(const rtx_scene* sc, const rtx_camera* cam, uint32_t width, uint32_t height, float* depth,
                   float* normal, uint32_t* material, uint32_t* primitive) {
    const int W = (int)width, H = (int)height;
    const float aspect = (int)width / (float)(int)height; /* Renderer.cpp:30, as run() */
    for (uint32_t py = 0; py < height; ++py) {
        for (uint32_t px = 0; px < width; ++px) {
            /* render_pixel's ray, statement for statement */
            const float cx = (2.f * (((int)px + 0.5f) / W) - 1) * aspect * cam->fov;
            const float cy = (1.f - (2.f * ((int)py + 0.5f) / H)) * cam->fov;
            v3 vd = mk(cam->right[0] * cx + cam->up[0] * cy + cam->forward[0] * 1.f,
                       cam->right[1] * cx + cam->up[1] * cy + cam->forward[1] * 1.f,
                       cam->right[2] * cx + cam->up[2] * cy + cam->forward[2] * 1.f);
            normalize(&vd);
            const ray vr = mkray(ld3(cam->origin), vd, 0.0001f, FLT_MAX);

            hitrec ch = empty_hit();
            closest_hit(sc, &vr, &ch, NULL);
            idrec tr;
            tr.h = empty_hit();
            tr.id = 0;
            id_closest_hit(sc, &vr, &tr);

            const size_t o = (size_t)px + (size_t)py * (size_t)W;
            if (tr.h.did_hit != ch.did_hit || tr.h.mat != ch.mat || !same_bits(tr.h.t, ch.t) ||
                !same_bits(tr.h.normal.x, ch.normal.x) || !same_bits(tr.h.normal.y, ch.normal.y) ||
                !same_bits(tr.h.normal.z, ch.normal.z) || (ch.did_hit != 0) != (tr.id != 0))
                return -(int)(o + 1);
            depth[o] = ch.t;
            normal[3 * o] = ch.normal.x; normal[3 * o + 1] = ch.normal.y; normal[3 * o + 2] = ch.normal.z;
            material[o] = ch.mat;
            primitive[o] = tr.id;
        }
    }
    return 0;
}
