// pack_harness.cpp — the scene packer (csrc/rtx_pack.h) on the CPU: TEST INFRASTRUCTURE of
// tests/test_pack_cpu.py, which compiles this file and csrc/rtx_pack.cpp with the address and
// undefined-behaviour sanitizers and links librtx_host.so for the scenes.  One command per input line:
//   scene LABEL NAME ASSET_DIR [t=TIME] [parts=N] [nocull=1] [no_octant=1] [room_skip_off=1]
//                              [refine=I,J] [reserve=1] [uploads=N] [min_sa=RATIO]
//       pack NAME (a catalogue scene, file:PATH, chain:T, lights:N or tris:A.B,...), emit it with all 8 octant copies
//       on the host, check the image's structure, print one line of hashes and facts per upload
//   refuse CASE     pack one of the minimal hand-built refusals, print the code and the message
//   time NAME ASSET_DIR REPS    print the best pack_scene + emit time
#include <algorithm>
#include <chrono>
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

[[noreturn]] void die(const std::string& what) {
    std::fprintf(stderr, "pack_harness: %s\n", what.c_str());
    std::exit(1);
}

uint64_t fnv(const char* p, size_t n) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ static_cast<unsigned char>(p[i])) * 0x100000001b3ull;
    return h;
}

uint32_t fbits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// A scene and what its pointers refer to.
struct Loaded {
    rtx_host_scene* host = nullptr;
    rtx_scene s{};
    std::vector<float> pos, nrm;
    std::vector<int32_t> idx;
    std::vector<rtx_bvh_node> nodes;
    std::vector<rtx_light> lights;
    rtx_mesh mesh{};
    std::vector<int32_t> spinning;
    ~Loaded() { if (host) rtx_host_scene_destroy(host); }
};

// tests/test_gpu_deep_bvh.py's chain_mesh: T small triangles on a staircase and a chain BVH over them
// (left = leaf k, right = the rest), T - 1 levels deep.  The coordinates are computed in double and
// rounded to binary32, as numpy does there.
void chain_mesh(Loaded& L, int T) {
    for (int k = 0; k < T; ++k) {
        const double x = -2.0 + 4.0 * k / T, y = 0.6 + 1.8 * ((k * 37) % T) / T, s = 4.0 / T + 0.05;
        const double v[9] = {x, y, 0.5, x + s, y, 0.5, x, y + s, 0.5};
        const int32_t b = static_cast<int32_t>(L.pos.size() / 3);
        for (double c : v) L.pos.push_back(static_cast<float>(c));
        L.idx.insert(L.idx.end(), {b, b + 2, b + 1});
        L.nrm.insert(L.nrm.end(), {0.f, 0.f, -1.f});
    }
    std::vector<float> lo(3 * T), hi(3 * T);   // per triangle, then as suffix boxes
    for (int k = 0; k < T; ++k)
        for (int a = 0; a < 3; ++a) {
            const float p0 = L.pos[9 * k + a], p1 = L.pos[9 * k + 3 + a], p2 = L.pos[9 * k + 6 + a];
            lo[3 * k + a] = std::min(p0, std::min(p1, p2));
            hi[3 * k + a] = std::max(p0, std::max(p1, p2));
        }
    L.nodes.assign(2 * T - 1, rtx_bvh_node{});
    auto leaf = [&](int n, int k) {
        for (int a = 0; a < 3; ++a) { L.nodes[n].min[a] = lo[3 * k + a]; L.nodes[n].max[a] = hi[3 * k + a]; }
        L.nodes[n].first_idx = 3 * k; L.nodes[n].idx_count = 3; L.nodes[n].left_node = 0;
    };
    leaf(2 * (T - 1), T - 1);
    std::vector<float> slo(lo.end() - 3, lo.end()), shi(hi.end() - 3, hi.end());   // the box of triangles k..T-1
    for (int k = T - 2; k >= 0; --k) {
        leaf(2 * k + 1, k);
        for (int a = 0; a < 3; ++a) {
            slo[a] = std::min(slo[a], lo[3 * k + a]);
            shi[a] = std::max(shi[a], hi[3 * k + a]);
            L.nodes[2 * k].min[a] = slo[a]; L.nodes[2 * k].max[a] = shi[a];
        }
        L.nodes[2 * k].first_idx = 0; L.nodes[2 * k].idx_count = 0; L.nodes[2 * k].left_node = 2 * k + 1;
    }
    L.mesh.positions = L.pos.data(); L.mesh.n_positions = static_cast<uint32_t>(L.pos.size() / 3);
    L.mesh.indices = L.idx.data(); L.mesh.n_indices = static_cast<uint32_t>(L.idx.size());
    L.mesh.normals = L.nrm.data();
    L.mesh.nodes = L.nodes.data(); L.mesh.n_nodes = static_cast<uint32_t>(L.nodes.size());
    L.mesh.cull_mode = RTX_CULL_NONE;
    L.mesh.material = 2;
    L.s.meshes = &L.mesh;
    L.s.n_meshes = 1;
}

// One mesh without a tree in W4_Bunny, its triangles (0, 0, 0), (a, 0, 0), (0, b, 0) given as the bit
// patterns "A.B,A.B,..." of a and b: |e1| |e2| = |a| |b| exactly (DevScene::tri_fast's cases)
void edge_tris(Loaded& L, const std::string& spec) {
    std::stringstream ss(spec);
    for (std::string tok; std::getline(ss, tok, ',');) {
        const uint32_t ua = static_cast<uint32_t>(std::stoul(tok.substr(0, tok.find('.')), nullptr, 16));
        const uint32_t ub = static_cast<uint32_t>(std::stoul(tok.substr(tok.find('.') + 1), nullptr, 16));
        float a, b;
        std::memcpy(&a, &ua, 4);
        std::memcpy(&b, &ub, 4);
        const int32_t i0 = static_cast<int32_t>(L.pos.size() / 3);
        L.pos.insert(L.pos.end(), {0.f, 0.f, 0.f, a, 0.f, 0.f, 0.f, b, 0.f});
        L.idx.insert(L.idx.end(), {i0, i0 + 1, i0 + 2});
        L.nrm.insert(L.nrm.end(), {0.f, 0.f, 1.f});
    }
    L.mesh.positions = L.pos.data(); L.mesh.n_positions = static_cast<uint32_t>(L.pos.size() / 3);
    L.mesh.indices = L.idx.data(); L.mesh.n_indices = static_cast<uint32_t>(L.idx.size());
    L.mesh.normals = L.nrm.data();
    L.mesh.cull_mode = RTX_CULL_NONE;
    L.s.meshes = &L.mesh;
    L.s.n_meshes = 1;
}

// N point lights in W4_Bunny (tests/pack_cases.py's many_lights: every value exact in binary32)
void many_lights(Loaded& L, int N) {
    for (int i = 0; i < N; ++i) {
        rtx_light l{};
        l.origin[0] = -2.f + 0.125f * i; l.origin[1] = 5.f; l.origin[2] = -3.f + 0.0625f * i;
        l.color[0] = 1.f; l.color[1] = 0.5f + i / 64.f; l.color[2] = 0.25f;
        l.intensity = 2.f + i;
        l.type = RTX_LIGHT_POINT;
        L.lights.push_back(l);
    }
    L.s.lights = L.lights.data();
    L.s.n_lights = static_cast<uint32_t>(N);
}

void load(Loaded& L, const std::string& name, const std::string& assets, const std::map<std::string, std::string>& kv) {
    const bool chain = name.rfind("chain:", 0) == 0, lights = name.rfind("lights:", 0) == 0;
    const bool tris = name.rfind("tris:", 0) == 0;
    const std::string host = (chain || lights || tris) ? "W4_Bunny" : name;
    char err[512] = "";
    if (rtx_host_scene_create(host.c_str(), assets.c_str(), &L.host, err, sizeof err) != RTX_OK) die(name + ": " + err);
    if (kv.count("t") && rtx_host_scene_update(L.host, std::strtof(kv.at("t").c_str(), nullptr)) != RTX_OK) die("update");
    rtx_camera cam;
    if (rtx_host_scene_view(L.host, &L.s, &cam) != RTX_OK) die("view");
    if (chain) chain_mesh(L, std::atoi(name.c_str() + 6));
    if (lights) many_lights(L, std::atoi(name.c_str() + 7));
    if (tris) edge_tris(L, name.substr(5));
    L.spinning.resize(64);
    const int n = rtx_host_scene_spinning(L.host, L.spinning.data(), 64);
    L.spinning.resize(n > 0 ? std::min(n, 64) : 0);
}

PackOptions options(const Loaded& L, const std::map<std::string, std::string>& kv) {
    PackOptions o;
    o.want_cull = !kv.count("nocull") && !kv.count("reserve") && L.s.n_lights <= static_cast<uint32_t>(kMaxCullLights);
    if (kv.count("parts")) o.split_parts = static_cast<uint32_t>(std::atoi(kv.at("parts").c_str()));
    o.no_octant = kv.count("no_octant");
    o.room_skip_off = kv.count("room_skip_off");
    if (kv.count("min_sa")) o.cull_min_sa = std::strtod(kv.at("min_sa").c_str(), nullptr);
    if (kv.count("refine")) {
        std::stringstream ss(kv.at("refine"));
        for (std::string tok; std::getline(ss, tok, ',');) o.part_refine.push_back(std::atoi(tok.c_str()));
    }
    if (kv.count("reserve")) {
        o.reserve.assign(L.s.n_meshes, 0);
        for (int32_t id : L.spinning) o.reserve[id] = 1;
    }
    return o;
}

#define REQUIRE(cond, what) do { if (!(cond)) die(label + ": structure: " + (what)); } while (0)

// The image's structure: what a later change to the layout must keep.
void check_structure(const std::string& label, const PackedScene& P, const std::vector<char>& img) {
    for (int i = 0; i < kSecCount; ++i) {
        const size_t end = i + 1 < kSecCount ? P.sec[i + 1].off : P.total;
        REQUIRE(P.sec[i].off % 256 == 0, "section offset not a multiple of 256");
        REQUIRE(P.sec[i].off + P.sec[i].n <= end, "sections overlap");
        for (size_t b = P.sec[i].off + P.sec[i].n; b < end; ++b) REQUIRE(img[b] == 0, "padding byte not zero");
    }
    REQUIRE(P.sec[0].off == 0 && P.total % 256 == 0 && img.size() == P.total, "image size");
    const char* nodes = img.data() + P.sec[kSecNodes].off;   // octant copy 0
    const int4* meshes = reinterpret_cast<const int4*>(img.data() + P.sec[kSecMeshes].off);
    const int4* parts = reinterpret_cast<const int4*>(img.data() + P.sec[kSecParts].off);
    const size_t node_bytes = static_cast<size_t>(P.n_nodes) * 32;
    std::vector<uint32_t> under, cover;
    // the triangles under the node at byte offset `at`, counted into `count`
    auto walk = [&](uint32_t at, std::vector<uint32_t>& count) {
        std::vector<uint32_t> todo{at};
        size_t visited = 0;
        while (!todo.empty()) {
            const uint32_t o = todo.back();
            todo.pop_back();
            REQUIRE(++visited <= P.n_nodes, "walk does not end");
            REQUIRE(o % 32 == 0 && o + 32 <= node_bytes, "node offset outside the section");
            uint32_t link, cnt;
            std::memcpy(&link, nodes + o + 24, 4);
            std::memcpy(&cnt, nodes + o + 28, 4);
            if (cnt) {
                REQUIRE(link % 64 == 0 && link / 64 + cnt <= P.n_tris, "leaf link is not a triangle of the section");
                for (uint32_t t = link / 64; t < link / 64 + cnt; ++t) ++count[t];
            } else {
                REQUIRE(link % 64 == 0 && link + 64 <= node_bytes, "inner link is not an even slot pair");
                todo.push_back(link + 32);
                todo.push_back(link);
            }
        }
    };
    for (uint32_t m = 0; m < P.n_meshes; ++m) {
        if (meshes[m].y == 0) continue;
        const uint32_t root = static_cast<uint32_t>(meshes[m].x);
        REQUIRE(root % 32 == 0 && (root / 32) % 2 == 1, "root not at an odd slot");
        under.assign(P.n_tris, 0);
        cover.assign(P.n_tris, 0);
        walk(root, under);
        if (!P.n_parts) continue;
        for (uint32_t k = 0; k < P.n_parts; ++k)
            if (parts[k].x == static_cast<int>(m)) walk(static_cast<uint32_t>(parts[k].y) * 32u, cover);
        for (uint32_t t = 0; t < P.n_tris; ++t)
            REQUIRE(cover[t] == under[t] && under[t] <= 1, "frontier does not cover the mesh's triangles exactly once");
    }
    for (size_t k = P.n_parts; k < P.sec[kSecParts].n / 16; ++k) REQUIRE(parts[k].x == -1, "reserved frontier entry not empty");
}

void print_scene(const std::string& label, const PackedScene& P, const std::vector<char>& img) {
    std::printf("%s total=%zu img=%016" PRIx64 " sec=", label.c_str(), P.total, fnv(img.data(), img.size()));
    for (int i = 0; i < kSecCount; ++i) std::printf("%s%016" PRIx64, i ? "," : "", fnv(img.data() + P.sec[i].off, P.sec[i].n));
    std::printf(" off=");
    for (int i = 0; i < kSecCount; ++i) std::printf("%s%zu", i ? "," : "", P.sec[i].off);
    std::printf(" n=");
    for (int i = 0; i < kSecCount; ++i) std::printf("%s%zu", i ? "," : "", P.sec[i].n);
    const SceneFacts& f = P.facts;
    std::printf(" spec=%d split_ok=%d deep=%d hbm=%d max_depth=%u room_fact=%d room_M=%08x sig=%s tri_fast=%u oct_bytes=%u"
                " n_parts=%u refinable=%d cull_on=%d worth=%d%d%d cull_T=",
                f.spec, f.split_ok, f.deep_stack, f.hbm_stack, f.max_depth, f.room_fact, fbits(f.room_M), f.sig.c_str(),
                P.tri_fast, P.oct_bytes, P.n_parts, P.refinable, P.cull_on, P.worth_from == PackedScene::kWorthComputed, P.worth_from == PackedScene::kWorthReused, P.worth);
    for (size_t i = 0; i < P.cull_T.size(); ++i) std::printf("%s%08x", i ? "," : "", fbits(P.cull_T[i]));
    std::printf("\n");
}

void cmd_scene(const std::string& label, const std::string& name, const std::string& assets,
               const std::map<std::string, std::string>& kv) {
    Loaded L;
    load(L, name, assets, kv);
    PackOptions o = options(L, kv);
    const int uploads = kv.count("uploads") ? std::atoi(kv.at("uploads").c_str()) : 1;
    // the worth cache as the uploads of an animated loop carry it (rtx_ctx::cull_worth*)
    int worth = -1;
    uint32_t age = 0;
    std::string sig;
    for (int u = 0; u < uploads; ++u) {
        o.worth_reuse = u >= 1 && worth >= 0 && age + 1 < kCullWorthReuse;
        o.worth = worth == 1;
        o.worth_sig = sig;
        PackedScene P;
        std::string err;
        const int rc = pack_scene(&L.s, o, P, err);
        if (rc != RTX_OK) die(label + ": refused: " + err);
        if (P.worth_from == PackedScene::kWorthReused) ++age;
        if (P.worth_from == PackedScene::kWorthComputed) { worth = P.worth; age = 0; sig = P.worth_sig; }
        std::vector<char> img(P.total, char(0x5a));   // (emit clears the padding itself)
        emit(P, img.data(), 8);
        check_structure(label, P, img);
        print_scene(uploads > 1 ? label + "#" + std::to_string(u + 1) : label, P, img);
    }
}

void cmd_time(const std::string& name, const std::string& assets, int reps) {
    Loaded L;
    load(L, name, assets, {});
    const PackOptions o = options(L, {});
    double best = 1e30;
    std::vector<char> img;
    for (int r = 0; r < reps; ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        PackedScene P;
        std::string err;
        if (pack_scene(&L.s, o, P, err) != RTX_OK) die(err);
        if (img.size() < P.total) img.resize(P.total);
        emit(P, img.data(), P.node_bytes >= kOctantDeviceMinBytes ? 1 : 8);
        best = std::min(best, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::printf("time %s pack+emit best of %d: %.3f ms\n", name.c_str(), reps, best);
}

// The refusals, each a minimal scene: one material, and where a mesh is needed one triangle under a
// one-leaf tree, with the one thing wrong.
void cmd_refuse(const std::string& what) {
    std::vector<rtx_material> mats(257);
    rtx_sphere sph{};
    rtx_plane pl{};
    const float pos[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0}, nrm[6] = {0, 0, 1, 0, 0, 1};
    int32_t idx[6] = {0, 1, 2, 0, 1, 2};
    rtx_bvh_node nd[5] = {};
    for (rtx_bvh_node& n : nd) { n.max[0] = n.max[1] = 1.f; n.idx_count = 3; }
    rtx_mesh m{};
    m.positions = pos; m.n_positions = 3; m.indices = idx; m.n_indices = 3; m.normals = nrm;
    m.nodes = nd; m.n_nodes = 1; m.cull_mode = RTX_CULL_BACK;
    rtx_scene s{};
    s.materials = mats.data(); s.n_materials = 1;
    s.meshes = &m; s.n_meshes = 1;
    auto inner = [&](int n, uint32_t left) { nd[n].idx_count = 0; nd[n].left_node = left; };
    if (what == "null_array") { s.n_spheres = 1; }
    else if (what == "materials_0") { s.n_materials = 0; }
    else if (what == "materials_257") { s.n_materials = 257; }
    else if (what == "sphere_material") { sph.material = 1; s.spheres = &sph; s.n_spheres = 1; }
    else if (what == "plane_material") { pl.material = 1; s.planes = &pl; s.n_planes = 1; }
    else if (what == "mesh_material") { m.material = 1; }
    else if (what == "cull_mode") { m.cull_mode = 3; }
    else if (what == "index_count") { m.n_indices = 4; }
    else if (what == "arrays_missing") { m.normals = nullptr; }
    else if (what == "index_range") { idx[1] = 3; }
    else if (what == "index_negative") { idx[2] = -1; }
    else if (what == "nodes_missing") { m.nodes = nullptr; }
    else if (what == "child_range") { m.n_nodes = 3; inner(0, 2); }
    else if (what == "child_0") { m.n_nodes = 3; inner(0, 0); }
    else if (what == "cycle") { m.n_nodes = 5; inner(0, 1); inner(1, 3); inner(3, 1); }
    else if (what == "leaf_first") { nd[0].first_idx = 1; m.n_indices = 6; }
    else if (what == "leaf_count") { nd[0].idx_count = 4; m.n_indices = 6; }
    else if (what == "leaf_beyond") { nd[0].idx_count = 6; }
    else if (what != "valid") die("unknown refusal " + what);
    PackedScene P;
    std::string err;
    const int rc = pack_scene(&s, PackOptions{}, P, err);
    std::printf("refuse %s code=%d msg=%s\n", what.c_str(), rc, err.c_str());
}

}  // namespace

int main() {
    for (std::string line; std::getline(std::cin, line);) {
        std::stringstream ss(line);
        std::string cmd, a, b, c;
        ss >> cmd;
        if (cmd == "refuse") { ss >> a; cmd_refuse(a); continue; }
        ss >> a >> b;
        if (cmd == "time") { ss >> c; cmd_time(a, b, std::atoi(c.c_str())); continue; }
        if (cmd != "scene") die("unknown command " + cmd);
        ss >> c;
        std::map<std::string, std::string> kv;
        for (std::string tok; ss >> tok;) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) die("bad option " + tok);
            kv[tok.substr(0, eq)] = tok.substr(eq + 1);
        }
        cmd_scene(a, b, c, kv);
        std::fflush(stdout);
    }
    return 0;
}
