/*
 * relight_ref.c — TEST INFRASTRUCTURE: the relight (include/rtx.h: rtx_relight) on the CPU, the checker of
 * tests/test_relight_cpu.py.
 *
 * It includes tests/deferred_ref.c unchanged, and through it tests/shade_ref.c, tests/rayq_ref.c,
 * tests/aov_ref.c and oracle/rtx_oracle.c.  Per ray it shades from (ray, t, normal, material, primitive)
 * plus the pixel's word of the shadow plane as the contract words it: closestHit is deferred_ref.c's
 * rebuild, the light loop is its loop with does_hit replaced by bit l of the word, and nothing is
 * traversed.  Equal to shade_ref_rays on the same rays, word for word, when the words hold does_hit's
 * answers, it pins the statement that the record, the ray and one bit per light are enough.
 */
#include "deferred_ref.c"

/* Renderer::RenderPixel (source/Renderer.cpp:116-181) per ray, with closestHit taken from element i of the
 * four planes and Scene::DoesHit for light l from bit l of bits[i] (read only with shadows on; bits may
 * be NULL otherwise): pixels[i], rgb[3i .. 3i + 2]. */
void relight_ref_shade(const rtx_scene* sc, const float* rays, uint32_t n, const float* depth, const float* normal,
                       const uint32_t* material, const uint32_t* primitive, const uint32_t* bits,
                       const rtx_render_params* p, uint32_t* pixels, float* rgb_out) {
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
                (void)normalize(&ld);
                if (p->shadows_enabled && li < 32u && ((bits[i] >> li) & 1u)) {
                    shadowFactor *= 0.95f;
                    continue;
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
