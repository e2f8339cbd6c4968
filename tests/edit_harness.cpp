// edit_harness.cpp — the in-place edits' packer functions (csrc/rtx_pack.h: edit_inputs, pack_light_edit,
// pack_material_edit, apply_ranges) on the CPU: TEST INFRASTRUCTURE of tests/test_edit_cpu.py, which compiles
// this file and csrc/rtx_pack.cpp with the address and undefined-behaviour sanitizers and links
// librtx_host.so for the scenes.  One scenario per input line:
//   edit LABEL NAME ASSET_DIR [room_skip_off=1] [nocull=1] -- STEP STEP ...
//       NAME: a catalogue scene, file:PATH, or mats256:SCENE (SCENE with 256 materials: its own, then
//       Lambert ones whose values follow from their index).  Pack it and emit its image.  Then each STEP,
//           L<first>:REC;REC;...    REC = ox,oy,oz,cr,cg,cb,intensity[,type]     (binary32 bit patterns, hex)
//           M<first>:REC;REC;...    REC = cr,cg,cb,kd,ks,exponent,metalness,roughness[,kind]
//       replaces those records in the scene, packs the edited scene from scratch and emits it (image B),
//       applies the edit's ranges to the running image, and prints
//           LABEL step=K rc=RC equal=0|1 facts=0|1 differ=SEC,... room_fact=F room_M=HEX spec=N moved=M
//                 ranges=R words=W err=MESSAGE
//       equal: the patched image is B byte for byte; facts: the retained room_fact, room_M and spec are B's;
//       differ: the sections in which the image before the step and B differ.  A refused step (rc != 0) must
//       yield no range; the scene and the image stay as they were.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "rtx_host.h"
#include "rtx_pack.h"

using namespace rtxh;
using namespace rtxd;

namespace {

const char* const kSections[kSecCount] = {"spheres", "sphere_mat", "planes", "tris", "nodes", "meshes", "lights",
                                          "materials", "parts", "cull_rng", "cull_T"};

[[noreturn]] void die(const std::string& what) {
    std::fprintf(stderr, "edit_harness: %s\n", what.c_str());
    std::exit(1);
}

float fbits(const std::string& hex) {
    const uint32_t u = static_cast<uint32_t>(std::stoul(hex, nullptr, 16));
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
uint32_t ubits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

std::vector<std::string> split(const std::string& s, char sep) {
    std::vector<std::string> out;
    std::stringstream ss(s);
    for (std::string tok; std::getline(ss, tok, sep);) out.push_back(tok);
    return out;
}

struct Scene {
    rtx_host_scene* host = nullptr;
    rtx_scene s{};
    std::vector<rtx_light> lights;
    std::vector<rtx_material> mats;
    ~Scene() { if (host) rtx_host_scene_destroy(host); }
};

void load(Scene& S, std::string name, const std::string& assets) {
    const bool many = name.rfind("mats256:", 0) == 0;
    if (many) name = name.substr(8);
    char err[512] = "";
    if (rtx_host_scene_create(name.c_str(), assets.c_str(), &S.host, err, sizeof err) != RTX_OK) die(name + ": " + err);
    rtx_camera cam;
    if (rtx_host_scene_view(S.host, &S.s, &cam) != RTX_OK) die("view");
    S.lights.assign(S.s.lights, S.s.lights + S.s.n_lights);
    S.mats.assign(S.s.materials, S.s.materials + S.s.n_materials);
    for (uint32_t i = S.s.n_materials; many && i < 256; ++i) {
        rtx_material m{};
        m.kind = RTX_MAT_LAMBERT;
        m.color[0] = 0.25f + i / 512.f; m.color[1] = 1.f - i / 300.f; m.color[2] = 0.5f;
        m.kd = 0.5f + i / 1024.f;
        m.ks = 0.25f; m.exponent = 8.f + i; m.metalness = 0.f; m.roughness = 0.5f;
        S.mats.push_back(m);
    }
    S.s.lights = S.lights.data();
    S.s.materials = S.mats.data();
    S.s.n_materials = static_cast<uint32_t>(S.mats.size());
}

void pack(const Scene& S, const PackOptions& o, PackedScene& P, std::vector<char>& img) {
    std::string err;
    if (pack_scene(&S.s, o, P, err) != RTX_OK) die("refused: " + err);
    img.assign(P.total, char(0x5a));
    emit(P, img.data(), 8);
}

void scenario(const std::string& label, const std::string& name, const std::string& assets,
              const std::map<std::string, std::string>& kv, const std::vector<std::string>& steps) {
    Scene S;
    load(S, name, assets);
    PackOptions o;
    o.want_cull = !kv.count("nocull") && S.s.n_lights <= static_cast<uint32_t>(kMaxCullLights);
    o.room_skip_off = kv.count("room_skip_off");
    PackedScene P;
    std::vector<char> img;
    pack(S, o, P, img);
    EditInputs E;
    edit_inputs(&S.s, o, P, E);
    int k = 0;
    for (const std::string& step : steps) {
        ++k;
        const bool is_light = step[0] == 'L';
        if (!is_light && step[0] != 'M') die("bad step " + step);
        const size_t colon = step.find(':');
        const uint32_t first = static_cast<uint32_t>(std::stoul(step.substr(1, colon - 1)));
        std::vector<rtx_light> ls;
        std::vector<rtx_material> ms;
        for (const std::string& rec : split(step.substr(colon + 1), ';')) {
            const std::vector<std::string> w = split(rec, ',');
            const size_t at = first + (is_light ? ls.size() : ms.size());
            if (is_light) {
                if (w.size() != 7 && w.size() != 8) die("light record of " + std::to_string(w.size()) + " words");
                rtx_light l{};
                for (int a = 0; a < 3; ++a) { l.origin[a] = fbits(w[a]); l.color[a] = fbits(w[3 + a]); }
                l.direction[0] = 123.f;   // (ignored: the device record never carried it)
                l.intensity = fbits(w[6]);
                l.type = w.size() == 8 ? std::atoi(w[7].c_str()) : (at < S.lights.size() ? S.lights[at].type : 0);
                ls.push_back(l);
            } else {
                if (w.size() != 8 && w.size() != 9) die("material record of " + std::to_string(w.size()) + " words");
                rtx_material m{};
                for (int a = 0; a < 3; ++a) m.color[a] = fbits(w[a]);
                m.kd = fbits(w[3]); m.ks = fbits(w[4]); m.exponent = fbits(w[5]); m.metalness = fbits(w[6]);
                m.roughness = fbits(w[7]);
                m.kind = w.size() == 9 ? std::atoi(w[8].c_str()) : (at < S.mats.size() ? S.mats[at].kind : 0);
                ms.push_back(m);
            }
        }
        const uint32_t n = static_cast<uint32_t>(is_light ? ls.size() : ms.size());
        LightPatch lp;
        MaterialPatch mp;
        std::string err;
        const int rc = is_light ? pack_light_edit(E, first, n, ls.data(), lp, err)
                                : pack_material_edit(E, first, n, ms.data(), mp, err);
        const std::vector<EditRange>& ranges = is_light ? lp.ranges : mp.ranges;
        size_t words = 0;
        for (const EditRange& r : ranges) {
            if (r.off % 4 || r.off + 4 * r.words.size() > img.size()) die(label + ": a range outside the image");
            words += r.words.size();
        }
        if (rc != RTX_OK) {
            if (!ranges.empty()) die(label + ": a refused edit yields ranges");
            std::printf("%s step=%d rc=%d equal=1 facts=1 differ= room_fact=%d room_M=%08x spec=%d moved=0 ranges=0 words=0 err=%s\n",
                        label.c_str(), k, rc, E.facts.room_fact, ubits(E.facts.room_M), E.facts.spec, err.c_str());
            continue;
        }
        // the edited scene, packed from scratch: type and direction as the scene has them
        for (uint32_t i = 0; i < n; ++i) {
            if (is_light) {
                rtx_light& l = S.lights[first + i];
                std::memcpy(l.origin, ls[i].origin, 12);
                std::memcpy(l.color, ls[i].color, 12);
                l.intensity = ls[i].intensity;
            } else {
                S.mats[first + i] = ms[i];
            }
        }
        PackedScene B;
        std::vector<char> imgB;
        pack(S, o, B, imgB);
        if (imgB.size() != img.size()) die(label + ": the edited scene's image has another size");
        std::string differ;
        for (int s = 0; s < kSecCount; ++s) {
            const size_t end = s + 1 < kSecCount ? B.sec[s + 1].off : B.total;
            if (B.sec[s].off != P.sec[s].off) die(label + ": a section moved");
            if (std::memcmp(img.data() + B.sec[s].off, imgB.data() + B.sec[s].off, end - B.sec[s].off) != 0)
                differ += std::string(differ.empty() ? "" : ",") + kSections[s];
        }
        apply_ranges(ranges, img.data());
        if (is_light) commit_light_edit(E, lp);
        const bool equal = std::memcmp(img.data(), imgB.data(), img.size()) == 0;
        const bool facts = E.facts.room_fact == B.facts.room_fact && ubits(E.facts.room_M) == ubits(B.facts.room_M) &&
                           E.facts.spec == B.facts.spec;
        std::printf("%s step=%d rc=0 equal=%d facts=%d differ=%s room_fact=%d room_M=%08x spec=%d moved=%u ranges=%zu words=%zu err=\n",
                    label.c_str(), k, equal, facts, differ.c_str(), B.facts.room_fact, ubits(B.facts.room_M), B.facts.spec,
                    is_light ? lp.moved : 0u, ranges.size(), words);
    }
}

}  // namespace

int main() {
    for (std::string line; std::getline(std::cin, line);) {
        std::stringstream ss(line);
        std::string cmd, label, name, assets;
        ss >> cmd >> label >> name >> assets;
        if (cmd != "edit") die("unknown command " + cmd);
        std::map<std::string, std::string> kv;
        std::vector<std::string> steps;
        bool in_steps = false;
        for (std::string tok; ss >> tok;) {
            if (tok == "--") { in_steps = true; continue; }
            if (in_steps) { steps.push_back(tok); continue; }
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) die("bad option " + tok);
            kv[tok.substr(0, eq)] = tok.substr(eq + 1);
        }
        scenario(label, name, assets, kv, steps);
        std::fflush(stdout);
    }
    return 0;
}
