/*
 * deferred_ref.c — TEST INFRASTRUCTURE: deferred shading (include/rtx.h: rtx_shade_aov) on the CPU, the
 * checker of tests/test_deferred_cpu.py.
 *
 * It includes tests/shade_ref.c unchanged, and through it tests/rayq_ref.c, tests/aov_ref.c and
 * oracle/rtx_oracle.c.  Per ray it shades from (ray, t, normal, material, primitive) as the contract
 * words it: closestHit is rebuilt from the four plane values and the ray alone, no traversal, and from
 * originOffset on it is the oracle's render_pixel, calling the oracle's own does_hit, dir_to_light,
 * radiance, shade and q8.  Equal to shade_ref_rays on the same rays, word for word, it pins the statement
 * that the stored record plus the ray is enough.
 */
#include "shade_ref.c"

/* closestHit from the planes: didHit = (primitive != 0), t, normal and materialIndex as stored, origin =
 * ray.origin + t * ray.direction per component, one rounded multiply and one rounded add. */
static hitrec deferred_hit(const ray* vr, float t, const float* n3, uint32_t material, uint32_t primitive) {
    hitrec ch = empty_hit();
    if (primitive == 0u) return ch;
    ch.did_hit = 1;
    ch.t = t;
    ch.normal = ld3(n3);
    ch.mat = material;
    ch.origin = add(vr->o, scale(vr->d, t));
    return ch;
}

/* Renderer::RenderPixel (source/Renderer.cpp:116-181) per ray, with closestHit taken from element i of the
 * four planes instead of Scene::GetClosestHit: pixels[i], rgb[3i .. 3i + 2]. */
void deferred_ref_shade(const rtx_scene* sc, const float* rays, uint32_t n, const float* depth, const float* normal,
                        const uint32_t* material, const uint32_t* primitive, const rtx_render_params* p,
                        uint32_t* pixels, float* rgb_out) {
    for (uint32_t i = 0; i < n; ++i) {
        const ray vr = ray_of(rays + 8 * (size_t)i);
        const hitrec ch = deferred_hit(&vr, depth[i], normal + 3 * (size_t)i, material[i], primitive[i]);

        float shadowFactor = 1.f;
        rgb fc = mkc(0.f, 0.f, 0.f);
        if (ch.did_hit) {
            const v3 oo = add(ch.origin, scale(ch.normal, 0.0001f));
            const v3 negv = mk(-vr.d.x, -vr.d.y, -vr.d.z);
            for (uint32_t li = 0; li < sc->n_lights; ++li) {
                const rtx_light* L = &sc->lights[li];
                v3 ld = dir_to_light(L, oo);
                const float mag = normalize(&ld);
                if (p->shadows_enabled) {
                    const ray sr = mkray(oo, ld, 0.0001f, mag);
                    if (does_hit(sc, &sr, NULL)) {
                        shadowFactor *= 0.95f;
                        continue;
                    }
                }
                switch (p->lighting_mode) {
                case RTX_MODE_COMBINED: {
                    const float oa = smax(dot(ch.normal, ld), 0.f);
                    const rgb rad = radiance(L, ch.origin);
                    const rgb br = shade(&sc->materials[ch.mat], ch.normal, ld, negv, NULL);
                    fc.r += (rad.r * oa) * br.r; fc.g += (rad.g * oa) * br.g; fc.b += (rad.b * oa) * br.b;
                    break;
                }
                case RTX_MODE_OBSERVED_AREA: {
                    const float oa = smax(dot(ch.normal, ld), 0.f);
                    fc.r += oa; fc.g += oa; fc.b += oa;
                    break;
                }
                case RTX_MODE_RADIANCE: {
                    const rgb rad = radiance(L, ch.origin);
                    fc.r += rad.r; fc.g += rad.g; fc.b += rad.b;
                    break;
                }
                case RTX_MODE_BRDF: {
                    const rgb br = shade(&sc->materials[ch.mat], ch.normal, ld, negv, NULL);
                    fc.r += br.r; fc.g += br.g; fc.b += br.b;
                    break;
                }
                default: break;
                }
            }
            fc.r *= shadowFactor; fc.g *= shadowFactor; fc.b *= shadowFactor;
        }
        /* ColorRGB::MaxToOne (ColorRGB.h:12-17) */
        const float mv = smax(fc.r, smax(fc.g, fc.b));
        if (mv > 1.f) { fc.r /= mv; fc.g /= mv; fc.b /= mv; }
        pixels[i] = (q8(fc.r) << p->format.rshift) | (q8(fc.g) << p->format.gshift) |
                    (q8(fc.b) << p->format.bshift) | p->format.amask;
        rgb_out[3 * (size_t)i] = fc.r; rgb_out[3 * (size_t)i + 1] = fc.g; rgb_out[3 * (size_t)i + 2] = fc.b;
    }
}
