// host_sanitizer_driver.cpp -- TEST INFRASTRUCTURE (tests/test_host_malformed_inputs.py): the host loaders
// (csrc/host/obj_loader.cpp, png_decode.cpp, scene.cpp, bvh.cpp) behind the C API of csrc/host/scene_capi.cpp, built
// with AddressSanitizer + UndefinedBehaviorSanitizer on the CPU, fed one file per line of a manifest:
//     <mode> <path>        mode = obj (rt_scene_add_obj with its MTL, then rt_scene_build) | png (decode_png_file)
//                                 | pack (both phases of the host packer, csrc/host/scene_pack.cpp, on the arrays of a file:
//                                   four u32 counts -- spheres, meshes, triangles, nodes -- then the four arrays as
//                                   include/rt_abi.h lays them out; memory safety and return codes only, no blob bits)
//                                 | options (no file: the option setter, csrc/host/launch_options.cpp, with every name of its
//                                   table at a grid of values, and with names it has to refuse)
// Prints "BEGIN <path>" before and "END <rc>" after each file, so that a sanitizer abort names its input.
// The reference panics on a file it cannot read (src/core/asset.rs:72-75,118); here every malformed input has to come
// back as an error code.
#include <climits>
#include <cstdio>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/rt_abi.h"
#include "../../ray_tracer_2_amd/csrc/host/launch_options.h"
#include "../../ray_tracer_2_amd/csrc/host/scene.h"
#include "../../ray_tracer_2_amd/csrc/host/scene_pack.h"

namespace rt2 {
// (the device-side plane search lives in csrc/rt_bvh_search.hip; not part of this CPU build)
LevelSearch make_device_level_search(int, const float*, size_t) { throw std::runtime_error("HIP: no device in the sanitizer build"); }
}  // namespace rt2

// The arrays of a `pack` file, each in a heap block of exactly its size (so that a read past an end is a report).
template <typename T>
static bool read_array(std::ifstream& in, uint32_t n, std::vector<T>& out) {
    out.resize(n);
    return n == 0 || (bool)in.read(reinterpret_cast<char*>(out.data()), (std::streamsize)n * sizeof(T));
}
static int pack_file(const std::string& path) {
    std::ifstream in(path, std::ios::binary);
    uint32_t n[4];
    std::vector<rt_sphere> spheres;
    std::vector<rt_mesh_uniform> meshes;
    std::vector<rt_packed_triangle> triangles;
    std::vector<rt_node> nodes;
    if (!in.read(reinterpret_cast<char*>(n), sizeof(n)) || !read_array(in, n[0], spheres) || !read_array(in, n[1], meshes) ||
        !read_array(in, n[2], triangles) || !read_array(in, n[3], nodes))
        return RT_ERR_IO;
    rt2::SceneGeom g;
    rt2::InstanceFacts facts;
    std::vector<rt2::Quad> head, tail;
    std::string why;
    int rc = rt2::pack_geometry(meshes.data(), n[1], triangles.data(), n[2], nodes.data(), n[3], g, tail, why);
    if (rc == RT_OK) rc = rt2::pack_instances(rt2::PackOptions{}, g, spheres.data(), n[0], meshes.data(), n[1], facts, head, why);
    if (rc == RT_OK && ((uint64_t)head.size() * 16u != facts.lay.wide_off || facts.lay.wide_off + g.tail_bytes() > facts.lay.bytes)) rc = -100;
    return rc;
}

// Every row's name and six names without a row (a 4 KiB one, one with bytes >= 0x80), each at the grid of
// tests/golden/option_behaviour.json: an accepted value is stored inside the row's range with the row's effects, a refusal
// stores nothing, has a text and no effect.
static int set_options() {
    static const int values[] = {INT_MIN, -2, -1, 0, 1, 2, 3, 7, 8, 9, 63, 64, 65, 2048, 2049, INT_MAX};
    std::vector<std::string> names = {"", "Pipeline", "pipeline ", "no_such_option", std::string(4096, 'p'), "pipeline\x80\xff"};
    for (size_t k = 0; rt2::option_row(k); ++k) names.push_back(rt2::option_row(k)->name);
    for (size_t k = 0; k < names.size(); ++k)
        for (const int value : values) {
            rt2::Options opt;
            const rt2::SetResult r = rt2::set_option(opt, names[k].c_str(), value);
            if ((r.row != nullptr) != (k >= 6)) return -100;
            if (r.code() != RT_OK && (r.code() != RT_ERR_INVALID_ARGUMENT || r.error.empty() || r.effects != 0u)) return -101;
            if (!r.row) {
                if (r.code() == RT_OK || r.error != "unknown option " + names[k]) return -102;
                continue;
            }
            rt2::Options fresh;
            const int stored = r.row->at(opt), before = r.row->at(fresh);
            if (r.code() != RT_OK) {
                if (stored != before) return -103;
            } else if (stored < r.row->lo || stored > r.row->hi || r.effects != (r.row->flags & rt2::OPT_EFFECTS)) {
                return -104;
            }
        }
    return RT_OK;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::ifstream manifest(argv[1]);
    std::string mode, path;
    while (manifest >> mode && std::getline(manifest >> std::ws, path)) {
        std::printf("BEGIN %s\n", path.c_str());
        std::fflush(stdout);
        int rc = 0;
        if (mode == "obj") {
            rt_scene* s = nullptr;
            rc = rt_scene_create(&s);
            if (rc == RT_OK) {
                const size_t slash = path.find_last_of('/');
                const std::string dir = slash == std::string::npos ? "." : path.substr(0, slash);
                const std::string file = slash == std::string::npos ? path : path.substr(slash + 1);
                rc = rt_scene_add_obj(s, dir.c_str(), file.c_str(), nullptr, 1, nullptr);
                if (rc == RT_OK) rc = rt_scene_build(s, 2);
                if (rc == RT_OK) {
                    // what an upload would read: every array through its accessor
                    volatile uint32_t sink = rt_scene_num_meshes(s) + rt_scene_num_triangles(s) + rt_scene_num_nodes(s) + rt_scene_num_textures(s);
                    (void)sink;
                }
                rt_scene_destroy(s);
            }
        } else if (mode == "png") {
            rt2::Image img;
            rc = rt2::decode_png_file(path, img) ? RT_OK : RT_ERR_IO;
            if (rc == RT_OK && img.rgba.size() != (size_t)img.width * img.height * 4) rc = -100;  // (a decoder that lies about its output)
        } else if (mode == "pack") {
            rc = pack_file(path);
        } else if (mode == "options") {
            rc = set_options();
        } else {
            rc = -101;
        }
        std::printf("END %d\n", rc);
        std::fflush(stdout);
    }
    return 0;
}
