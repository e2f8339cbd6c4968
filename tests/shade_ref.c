/*
 * shade_ref.c — TEST INFRASTRUCTURE: shaded rays (include/rtx.h: rtx_shade_rays) on the CPU, the
 * checker of tests/test_shade_cpu.py and tests/test_gpu_shade.py.
 *
 * It includes tests/rayq_ref.c unchanged, and through it tests/aov_ref.c and oracle/rtx_oracle.c.  A ray
 * is the eight floats of rtx_ray; per ray it restates the oracle's render_pixel from closest_hit on, with
 * ray_of(q) in the place of the camera's ray and -direction (as given) as Shade's view vector, calling
 * the oracle's own closest_hit, does_hit, dir_to_light, radiance, shade and q8.
 */
#include "rayq_ref.c"

enum { SHADE_HIT = 1, SHADE_OCCLUDED = 2, SHADE_DIVIDED = 4 };

/* Renderer::RenderPixel (source/Renderer.cpp:116-181) per ray: pixels[i], rgb[3i .. 3i + 2] and, when
 * `flags` is not NULL, what the ray exercised (SHADE_*: it hit, a light of it was occluded, MaxToOne
 * divided). */
void shade_ref_rays(const rtx_scene* sc, const float* rays, uint32_t n, const rtx_render_params* p, uint32_t* pixels,
                    float* rgb_out, uint8_t* flags) {
    for (uint32_t i = 0; i < n; ++i) {
        const ray vr = ray_of(rays + 8 * (size_t)i);
        uint8_t fl = 0;
        hitrec ch = empty_hit();
        closest_hit(sc, &vr, &ch, NULL);

        float shadowFactor = 1.f;
        rgb fc = mkc(0.f, 0.f, 0.f);
        if (ch.did_hit) {
            fl |= SHADE_HIT;
            const v3 oo = add(ch.origin, scale(ch.normal, 0.0001f));
            const v3 negv = mk(-vr.d.x, -vr.d.y, -vr.d.z);
            for (uint32_t li = 0; li < sc->n_lights; ++li) {
                const rtx_light* L = &sc->lights[li];
                v3 ld = dir_to_light(L, oo);
                const float mag = normalize(&ld);
                if (p->shadows_enabled) {
                    const ray sr = mkray(oo, ld, 0.0001f, mag);
                    if (does_hit(sc, &sr, NULL)) {
                        fl |= SHADE_OCCLUDED;
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
        if (mv > 1.f) { fc.r /= mv; fc.g /= mv; fc.b /= mv; fl |= SHADE_DIVIDED; }
        pixels[i] = (q8(fc.r) << p->format.rshift) | (q8(fc.g) << p->format.gshift) |
                    (q8(fc.b) << p->format.bshift) | p->format.amask;
        rgb_out[3 * (size_t)i] = fc.r; rgb_out[3 * (size_t)i + 1] = fc.g; rgb_out[3 * (size_t)i + 2] = fc.b;
        if (flags) flags[i] = fl;
    }
}
