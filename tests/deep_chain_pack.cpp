// deep_chain_pack.cpp — the scene packer's facts for a hand-built mesh read from a file: TEST
// INFRASTRUCTURE of tests/test_deep_chain_cpu.py.  tests/pack_harness.cpp builds its chains itself and
// has no command for another tree, so this file includes it unchanged (its main renamed) and adds one:
//   mesh LABEL FILE ASSET_DIR [parts=N] [nocull=1] ...
//       W4_Bunny with its mesh replaced by FILE's (tests/deep_chain.py's write_mesh: int32 T, positions,
//       indices, normals, nodes), packed, emitted with all 8 octant copies, checked for the image's
//       structure and printed as pack_harness prints a scene.
// Compiled with csrc/rtx_pack.cpp by test_pack_cpu.build_harness's command line, this file in
// pack_harness.cpp's place.
#define main pack_harness_main
#include "pack_harness.cpp"
#undef main

#include <fstream>

namespace {

template <typename V>
void read_into(std::ifstream& f, V& v, size_t n, const std::string& path) {
    v.resize(n);
    f.read(reinterpret_cast<char*>(v.data()), static_cast<std::streamsize>(n * sizeof(v[0])));
    if (!f) die(path + ": short file");
}

void cmd_mesh(const std::string& label, const std::string& path, const std::string& assets,
              const std::map<std::string, std::string>& kv) {
    Loaded L;
    load(L, "W4_Bunny", assets, {});
    std::ifstream f(path, std::ios::binary);
    int32_t T = 0;
    f.read(reinterpret_cast<char*>(&T), 4);
    if (!f || T < 2 || T > (1 << 20)) die(path + ": bad triangle count");
    static_assert(sizeof(rtx_bvh_node) == 36, "write_mesh writes 36-byte nodes");
    const size_t n = static_cast<size_t>(T);
    read_into(f, L.pos, 9 * n, path);
    read_into(f, L.idx, 3 * n, path);
    read_into(f, L.nrm, 3 * n, path);
    read_into(f, L.nodes, 2 * n - 1, path);
    L.mesh.positions = L.pos.data(); L.mesh.n_positions = static_cast<uint32_t>(3 * n);
    L.mesh.indices = L.idx.data(); L.mesh.n_indices = static_cast<uint32_t>(3 * n);
    L.mesh.normals = L.nrm.data();
    L.mesh.nodes = L.nodes.data(); L.mesh.n_nodes = static_cast<uint32_t>(2 * n - 1);
    L.mesh.cull_mode = RTX_CULL_NONE;
    L.mesh.material = 2;
    L.s.meshes = &L.mesh;
    L.s.n_meshes = 1;
    const PackOptions o = options(L, kv);
    PackedScene P;
    std::string err;
    if (pack_scene(&L.s, o, P, err) != RTX_OK) die(label + ": refused: " + err);
    std::vector<char> img(P.total, char(0x5a));
    emit(P, img.data(), 8);
    check_structure(label, P, img);
    print_scene(label, P, img);
}

}  // namespace

int main() {
    for (std::string line; std::getline(std::cin, line);) {
        std::stringstream ss(line);
        std::string cmd, label, path, assets;
        ss >> cmd >> label >> path >> assets;
        if (cmd != "mesh") die("unknown command " + cmd);
        std::map<std::string, std::string> kv;
        for (std::string tok; ss >> tok;) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) die("bad option " + tok);
            kv[tok.substr(0, eq)] = tok.substr(eq + 1);
        }
        cmd_mesh(label, path, assets, kv);
        std::fflush(stdout);
    }
    return 0;
}
