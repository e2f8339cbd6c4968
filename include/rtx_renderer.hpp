// rtx_renderer.hpp — header-only C++ mirror of dae::Renderer (source/Renderer.h:17-61) on
// top of the C-ABI (rtx.h + rtx_host.h).  Same member names and state as the reference:
//
//   rtx::Renderer r(width, height);          // Renderer(SDL_Window*) — size of the surface
//   r.Render(scene);                         // Renderer::Render(Scene*) — fills r.Pixels()
//   r.CycleLightingMode(); r.ToggleShadows(); r.SaveBufferToImage("RayTracing_Buffer.bmp");
//
// `scene` is an rtx_host_scene (the C++ scene catalogue of librtx_host.so) or any
// caller-built rtx_scene + rtx_camera.  Errors throw std::runtime_error (the C-ABI below
// never throws).
#pragma once
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "rtx.h"
#include "rtx_host.h"

namespace rtx {

class Renderer {
public:
    enum class LightingMode { ObservedArea, Radiance, BRDF, Combined, Count };   // Renderer.h:40-48

    Renderer(int width, int height, int device = 0) : m_Width(width), m_Height(height) {
        if (rtx_create(&m_Ctx, device) != RTX_OK) throw std::runtime_error("rtx_create failed (no HIP device?)");
        m_Pixels.resize(static_cast<size_t>(width) * height);
    }
    ~Renderer() { rtx_destroy(m_Ctx); }
    Renderer(const Renderer&) = delete;
    Renderer& operator=(const Renderer&) = delete;

    // Upload only when the scene changed (after Initialize / Update), like the reference
    // which reads the Scene in place every frame.
    void Upload(const rtx_scene& scene) { Check(rtx_upload_scene(m_Ctx, &scene), "rtx_upload_scene"); }

    void Render(const rtx_camera& cam) {
        const rtx_render_params p = Params();
        m_Cam = cam; m_HaveCam = true;
        Check(rtx_render(m_Ctx, &cam, &p, m_Pixels.data(), nullptr), "rtx_render");
    }

    void Render(rtx_host_scene* scene, bool upload = true) {
        rtx_scene s;
        rtx_camera cam;
        Check(rtx_host_scene_view(scene, &s, &cam), "rtx_host_scene_view");
        if (upload) Upload(s);
        Render(cam);
    }

    // Render with adaptive supersampling (rtx_render_adaptive; not in the reference): k x k samples
    // (k = 2, 4, 8) for the pixels whose 8-bit colour differs from a 4-neighbour's by more than `threshold`
    // (0..255) in a channel, the plain pixel elsewhere.  AdaptiveRefined: how many pixels that was.
    void RenderAdaptive(const rtx_camera& cam, uint32_t k, uint32_t threshold) {
        const rtx_render_params p = Params();
        m_Cam = cam; m_HaveCam = true;
        Check(rtx_render_adaptive(m_Ctx, &cam, &p, k, threshold, m_Pixels.data(), nullptr), "rtx_render_adaptive");
    }
    void RenderAdaptive(rtx_host_scene* scene, uint32_t k, uint32_t threshold, bool upload = true) {
        rtx_scene s;
        rtx_camera cam;
        Check(rtx_host_scene_view(scene, &s, &cam), "rtx_host_scene_view");
        if (upload) Upload(s);
        RenderAdaptive(cam, k, threshold);
    }
    uint32_t AdaptiveRefined() {
        uint32_t n = 0;
        Check(rtx_adaptive_refined(m_Ctx, &n), "rtx_adaptive_refined");
        return n;
    }

    // The hit pass of the frame Render would render (rtx_render_aov; not in the reference): what every
    // pixel's primary ray hit, the planes of `mask` filled and the others left empty (rtx.h gives the
    // values: depth, normal, material index, primitive kind << 30 | index).
    struct AovFrame {
        std::vector<float> depth, normal;          // width*height, 3*width*height
        std::vector<uint32_t> material, primitive; // width*height each
    };
    AovFrame RenderAov(const rtx_camera& cam, uint32_t mask = RTX_AOV_ALL) {
        const rtx_render_params p = Params();
        m_Cam = cam; m_HaveCam = true;
        const size_t n = static_cast<size_t>(m_Width) * m_Height;
        AovFrame f;
        if (mask & RTX_AOV_DEPTH) f.depth.resize(n);
        if (mask & RTX_AOV_NORMAL) f.normal.resize(3 * n);
        if (mask & RTX_AOV_MATERIAL) f.material.resize(n);
        if (mask & RTX_AOV_PRIMITIVE) f.primitive.resize(n);
        const rtx_aov_planes out = {f.depth.empty() ? nullptr : f.depth.data(), f.normal.empty() ? nullptr : f.normal.data(),
                                    f.material.empty() ? nullptr : f.material.data(),
                                    f.primitive.empty() ? nullptr : f.primitive.data()};
        Check(rtx_render_aov(m_Ctx, &cam, &p, mask, &out), "rtx_render_aov");
        m_SampleK = 0;   // (the context's last hit pass is this width x height one, no sample pass)
        return f;
    }
    AovFrame RenderAov(rtx_host_scene* scene, uint32_t mask = RTX_AOV_ALL, bool upload = true) {
        rtx_scene s;
        rtx_camera cam;
        Check(rtx_host_scene_view(scene, &s, &cam), "rtx_host_scene_view");
        if (upload) Upload(s);
        return RenderAov(cam, mask);
    }
    // Deferred shading (rtx_shade_aov; not in the reference): the frame Render would render, shaded
    // from the last RenderAov's planes (all four) with the renderer's CURRENT lighting mode, shadows and
    // pixel format, without tracing a primary ray.  Explicit: nothing is cached or reused on its own,
    // and the scene is whatever was uploaded last.  Fills Pixels() (the renderer's size is the pass's).
    void ShadeAov() {
        NoSamplePass("ShadeAov");
        const rtx_render_params p = Params();
        Check(rtx_shade_aov(m_Ctx, &p, m_Pixels.data(), nullptr), "rtx_shade_aov");
    }
    // Relighting (rtx_render_shadows_async, rtx_relight; not in the reference).  RenderShadows stores the
    // shadow rays of the last RenderAov (all four planes) for the uploaded lights, one word of occlusion bits
    // per pixel, and returns them.  Relight then shades that pass with the renderer's CURRENT lighting mode,
    // shadows and pixel format without casting a ray, reading light colours, intensities and material values
    // from the scene uploaded last; it fills Pixels().  Explicit, like ShadeAov.
    std::vector<uint32_t> RenderShadows() {
        std::vector<uint32_t> bits(PassWords());
        Check(rtx_render_shadows_async(m_Ctx), "rtx_render_shadows_async");
        Check(rtx_download_shadows(m_Ctx, bits.data()), "rtx_download_shadows");
        return bits;
    }
    // The incremental shadow pass (rtx_update_shadows_async, rtx_refresh_shadows_async): after an upload that
    // moved lights, UpdateShadows re-traces the lights named in `lights` (bit l = light l; every other light
    // must be where the plane recorded it) and RefreshShadows re-traces whichever lights changed, or all of
    // them when there is no plane of the last RenderAov.  Both return the plane as RenderShadows does.
    // After RenderSamplePasses (below) all three work on the sample pass: the plane they return is the
    // k*width x k*height one.
    std::vector<uint32_t> UpdateShadows(uint32_t lights) {
        std::vector<uint32_t> bits(PassWords());
        Check(rtx_update_shadows_async(m_Ctx, lights), "rtx_update_shadows_async");
        Check(rtx_download_shadows(m_Ctx, bits.data()), "rtx_download_shadows");
        return bits;
    }
    std::vector<uint32_t> RefreshShadows(uint32_t* traced = nullptr) {
        std::vector<uint32_t> bits(PassWords());
        Check(rtx_refresh_shadows_async(m_Ctx, traced), "rtx_refresh_shadows_async");
        Check(rtx_download_shadows(m_Ctx, bits.data()), "rtx_download_shadows");
        return bits;
    }
    void Relight() {
        NoSamplePass("Relight");
        const rtx_render_params p = Params();
        Check(rtx_relight(m_Ctx, &p, m_Pixels.data(), nullptr), "rtx_relight");
    }
    // Scene edits (rtx_edit_lights, rtx_edit_materials; not in the reference): records first .. of the scene
    // uploaded last replaced in place, without packing or copying anything else; types and kinds stay the
    // uploaded ones.  The caller keeps its host scene in step (rtx_host_light_set_origin, or the same values
    // through the scene's view), so that a later call with upload = true uploads the same scene.  After a
    // moved light, RefreshShadows or UpdateShadows before Relight, as after an upload.
    void EditLights(uint32_t first, const std::vector<rtx_light>& lights) {
        Check(rtx_edit_lights(m_Ctx, first, static_cast<uint32_t>(lights.size()), lights.data()), "rtx_edit_lights");
    }
    void EditMaterials(uint32_t first, const std::vector<rtx_material>& materials) {
        Check(rtx_edit_materials(m_Ctx, first, static_cast<uint32_t>(materials.size()), materials.data()),
              "rtx_edit_materials");
    }
    // Resolved relighting (rtx_relight_resolve; not in the reference): the anti-aliased form of the loop above.
    // RenderSamplePasses stores the hit pass (all four planes) of the k*width x k*height sample frame of the
    // frame Render would render, k = 2, 4 or 8, and its shadow pass; RelightResolved then fills Pixels() with the
    // frame SetSupersample(k) + Render gives, from those passes alone: every sample relit with the renderer's
    // CURRENT lighting mode, shadows and pixel format and the scene uploaded last, each pixel's k x k samples
    // box-filtered.  After an upload that moved a light, RefreshShadows or UpdateShadows first: while the
    // sample passes are the context's last, they run and return the plane at sample size, and ShadeAov and Relight,
    // which would fill Pixels() with k*width x k*height pixels, throw; RenderAov ends that state.
    // Without a camera the passes take the one of the last Render, RenderAdaptive or RenderAov.
    void RenderSamplePasses(const rtx_camera& cam, uint32_t k) {
        if (k != 2 && k != 4 && k != 8) throw std::runtime_error("RenderSamplePasses: k must be 2, 4 or 8");
        rtx_render_params p = Params();
        p.width *= k; p.height *= k;
        m_Cam = cam; m_HaveCam = true;
        // (a refused hit pass throws here and leaves the context's last pass, and m_SampleK, as they were)
        Check(rtx_render_aov_async(m_Ctx, &cam, 1, &p, RTX_AOV_ALL), "rtx_render_aov_async");
        m_SampleK = k;   // the context's last hit pass from here on, whatever the shadow pass answers
        Check(rtx_render_shadows_async(m_Ctx), "rtx_render_shadows_async");
    }
    void RenderSamplePasses(uint32_t k) {
        if (!m_HaveCam) throw std::runtime_error("RenderSamplePasses: no camera yet (Render or RenderAov first, or pass one)");
        const rtx_camera cam = m_Cam;
        RenderSamplePasses(cam, k);
    }
    void RenderSamplePasses(rtx_host_scene* scene, uint32_t k, bool upload = true) {
        rtx_scene s;
        rtx_camera cam;
        Check(rtx_host_scene_view(scene, &s, &cam), "rtx_host_scene_view");
        if (upload) Upload(s);
        RenderSamplePasses(cam, k);
    }
    void RelightResolved() {
        if (!m_SampleK) throw std::runtime_error("RelightResolved: no sample passes yet (RenderSamplePasses)");
        const rtx_render_params p = Params();
        Check(rtx_relight_resolve(m_Ctx, &p, m_SampleK, m_Pixels.data(), nullptr), "rtx_relight_resolve");
    }

    // Ray queries against the uploaded scene (rtx_trace_rays / rtx_occluded; not in the reference's
    // Renderer): Scene::GetClosestHit and Scene::DoesHit on the caller's rays, uninterpreted (rtx.h).
    // TraceRays: element i of every plane of `mask` is ray i's record, the other planes stay empty.
    AovFrame TraceRays(const std::vector<rtx_ray>& rays, uint32_t mask = RTX_AOV_ALL) {
        const size_t n = rays.size();
        AovFrame f;
        if (mask & RTX_AOV_DEPTH) f.depth.resize(n);
        if (mask & RTX_AOV_NORMAL) f.normal.resize(3 * n);
        if (mask & RTX_AOV_MATERIAL) f.material.resize(n);
        if (mask & RTX_AOV_PRIMITIVE) f.primitive.resize(n);
        const rtx_aov_planes out = {f.depth.empty() ? nullptr : f.depth.data(), f.normal.empty() ? nullptr : f.normal.data(),
                                    f.material.empty() ? nullptr : f.material.data(),
                                    f.primitive.empty() ? nullptr : f.primitive.data()};
        Check(rtx_trace_rays(m_Ctx, rays.data(), static_cast<uint32_t>(n), mask, &out), "rtx_trace_rays");
        return f;
    }
    AovFrame TraceRays(rtx_host_scene* scene, const std::vector<rtx_ray>& rays, uint32_t mask = RTX_AOV_ALL,
                       bool upload = true) {
        rtx_scene s;
        rtx_camera cam;
        Check(rtx_host_scene_view(scene, &s, &cam), "rtx_host_scene_view");
        if (upload) Upload(s);
        return TraceRays(rays, mask);
    }
    // Occluded: element i is 1 when anything lies in ray i's [tmin, tmax] as DoesHit decides it.
    std::vector<uint8_t> Occluded(const std::vector<rtx_ray>& rays) {
        std::vector<uint8_t> out(rays.size());
        Check(rtx_occluded(m_Ctx, rays.data(), static_cast<uint32_t>(rays.size()), out.data()), "rtx_occluded");
        return out;
    }
    std::vector<uint8_t> Occluded(rtx_host_scene* scene, const std::vector<rtx_ray>& rays, bool upload = true) {
        rtx_scene s;
        rtx_camera cam;
        Check(rtx_host_scene_view(scene, &s, &cam), "rtx_host_scene_view");
        if (upload) Upload(s);
        return Occluded(rays);
    }

    // Shaded rays (rtx_shade_rays; not in the reference's Renderer): RenderPixel from GetClosestHit on
    // for the caller's rays, with the renderer's current lighting mode, shadows and pixel format
    // (Params()).  Element i of `pixels` and elements 3i .. 3i + 2 of `rgb` are ray i's.
    struct ShadedRays {
        std::vector<uint32_t> pixels;
        std::vector<float> rgb;
    };
    ShadedRays ShadeRays(const std::vector<rtx_ray>& rays) {
        const rtx_render_params p = Params();
        ShadedRays out;
        out.pixels.resize(rays.size());
        out.rgb.resize(3 * rays.size());
        Check(rtx_shade_rays(m_Ctx, rays.data(), static_cast<uint32_t>(rays.size()), &p, out.pixels.data(), out.rgb.data()),
              "rtx_shade_rays");
        return out;
    }
    ShadedRays ShadeRays(rtx_host_scene* scene, const std::vector<rtx_ray>& rays, bool upload = true) {
        rtx_scene s;
        rtx_camera cam;
        Check(rtx_host_scene_view(scene, &s, &cam), "rtx_host_scene_view");
        if (upload) Upload(s);
        return ShadeRays(rays);
    }

    void CycleLightingMode() {                                                    // Renderer.cpp:189-193
        m_CurrentLightingMode = static_cast<LightingMode>((static_cast<int>(m_CurrentLightingMode) + 1) %
                                                          static_cast<int>(LightingMode::Count));
    }
    void ToggleShadows() { m_ShadowsEnabled = !m_ShadowsEnabled; }                // Renderer.h:34-36
    // k x k samples per pixel (1, 2, 4 or 8) for every later Render (rtx_set_supersample); not in the reference
    void SetSupersample(uint32_t k) { Check(rtx_set_supersample(m_Ctx, k), "rtx_set_supersample"); }

    // SDL_SaveBMP of the XRGB8888 surface (Renderer.cpp:184-187): 32-bit BI_RGB, bottom-up.
    bool SaveBufferToImage(const std::string& path = "RayTracing_Buffer.bmp") const {
        FILE* f = std::fopen(path.c_str(), "wb");
        if (!f) return false;
        const uint32_t data = static_cast<uint32_t>(m_Pixels.size() * 4);
        const uint32_t hdr[13] = {0, 0, 54, 40, static_cast<uint32_t>(m_Width), static_cast<uint32_t>(m_Height),
                                  (32u << 16) | 1u, 0, data, 2835, 2835, 0, 0};
        const uint16_t bm = 0x4D42;
        const uint32_t size = 54 + data;
        bool ok = std::fwrite(&bm, 2, 1, f) == 1 && std::fwrite(&size, 4, 1, f) == 1 &&
                  std::fwrite(hdr + 1, 4, 12, f) == 12;
        for (int y = m_Height - 1; ok && y >= 0; --y)
            ok = std::fwrite(&m_Pixels[static_cast<size_t>(y) * m_Width], 4, m_Width, f) == static_cast<size_t>(m_Width);
        std::fclose(f);
        return ok;
    }

    const std::vector<uint32_t>& Pixels() const { return m_Pixels; }
    std::vector<uint32_t>& Pixels() { return m_Pixels; }
    int Width() const { return m_Width; }
    int Height() const { return m_Height; }
    rtx_ctx* Context() const { return m_Ctx; }
    LightingMode m_CurrentLightingMode{LightingMode::Combined};
    bool m_ShadowsEnabled{true};

    // The render parameters of the current state (Renderer::Render reads the same members).
    rtx_render_params Params() const {
        rtx_render_params p{};
        p.width = static_cast<uint32_t>(m_Width);
        p.height = static_cast<uint32_t>(m_Height);
        p.lighting_mode = static_cast<int32_t>(m_CurrentLightingMode);
        p.shadows_enabled = m_ShadowsEnabled ? 1 : 0;
        p.format = {16, 8, 0, 0};   // XRGB8888 window surface
        p.stripe_step = 1;
        return p;
    }
private:
    // Words of a plane of the context's last hit pass as this renderer queued it: the sample pass's after
    // RenderSamplePasses, else width x height.
    size_t PassWords() const {
        const size_t k = m_SampleK ? m_SampleK : 1;
        return k * static_cast<size_t>(m_Width) * k * static_cast<size_t>(m_Height);
    }
    void NoSamplePass(const char* what) const {
        if (m_SampleK)
            throw std::runtime_error(std::string(what) + ": the last hit pass is RenderSamplePasses' " +
                                     std::to_string(m_SampleK) + " x " + std::to_string(m_SampleK) +
                                     " sample pass, larger than Pixels(); RelightResolved shades it, RenderAov replaces it");
    }
    void Check(int rc, const char* what) const {
        if (rc != RTX_OK) throw std::runtime_error(std::string(what) + ": " + rtx_last_error(m_Ctx));
    }

    rtx_ctx* m_Ctx{};
    int m_Width, m_Height;
    std::vector<uint32_t> m_Pixels;
    rtx_camera m_Cam{};         // the camera of the last Render / RenderAdaptive / RenderAov / RenderSamplePasses
    bool m_HaveCam{false};
    uint32_t m_SampleK{0};      // the factor of the last RenderSamplePasses (0: none yet)
};

}  // namespace rtx
