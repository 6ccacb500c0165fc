// launch_options.cpp -- the option table and its setter (launch_options.h).
#include "launch_options.h"

namespace rt2 {

#define AT(member) [](Options& o) -> int& { return o.member; }
constexpr uint32_t B = OPT_BOOLEAN, UP = OPT_UPLOAD, EXP = OPT_EXPERIMENT;

// One row per option, in the order of the table in include/rt_abi.h, which says what each one means.
constexpr OptionRow OPTION_TABLE[] = {
    {"kernel_variant", AT(kernel_variant), 0, -1, 1, "-1 (auto), 0 or 1"},
    {"persistent_blocks", AT(persistent_blocks), 0, 1, INT_MAX, ">= 1"},
    {"specialise", AT(specialise), B, 0, 1, nullptr},
    {"lds_scene", AT(lds_scene), B, 0, 1, nullptr},  // (0: tuning / tests)
    {"pixel_cache", AT(pixel_cache), 0, 0, 2, "0, 1 or 2 (memo in global memory)"},
    {"primary_table", AT(primary_table), B, 0, 1, nullptr},
    {"primary_hits", AT(primary_hits), B | OPT_DROPS_PRIMARY, 0, 1, nullptr},
    {"max_device_mb", AT(max_device_mb), 0, 0, INT_MAX, ">= 0 (0 = no cap)"},
    {"memo_in_table", AT(memo_in_table), B, 0, 1, nullptr},
    {"vote_eighths", AT(vote_eighths), 0, -1, 8, "-1 (automatic) or 0..8"},
    {"vote_patience", AT(vote_patience), 0, -1, INT_MAX, "-1 (automatic) or >= 0"},
    {"tile_feedback", AT(tile_feedback), B | OPT_RESETS_TILES, 0, 1, nullptr},
    {"tile_feedback_period", AT(tile_feedback_period), OPT_RESETS_TILES, 1, INT_MAX, ">= 1"},
    {"pipeline", AT(pipeline), OPT_ONE_IS_AUTO, -1, (int)PIPE_MAX, "-1 (automatic), 0 (off) or 2 .. 8 (frames in flight)"},
    {"pipeline_when_idle", AT(pipeline_when_idle), B, 0, 1, nullptr},
    {"primary_per_slot", AT(primary_per_slot), B, 0, 1, nullptr},
    {"frame_ahead", AT(frame_ahead), OPT_NOT_ONE | OPT_CLEARS_AHEAD_FAILED, -1, (int)MAX_BATCH_FRAMES, "-1 (automatic), 0 (off) or 2 .. 64 (frames per batch)"},
    {"cross_prune", AT(cross_prune), B | OPT_DROPS_PRIMARY, 0, 1, nullptr},  // (the hits in the tables were found by the other walk)
    {"batch_frames", AT(batch_frames), 0, 1, (int)MAX_BATCH_FRAMES, "1..64"},
    {"batch_tile_major", AT(batch_tile_major), B, 0, 1, nullptr},
    {"forest", AT(pack.forest), B | UP, 0, 1, nullptr},
    {"flat2", AT(pack.flat2), B | UP, 0, 1, nullptr},
    {"stack_wide", AT(stack_wide), 0, -1, 1, "-1 (auto), 0 or 1"},
    {"tlas", AT(pack.tlas), B | UP, 0, 1, nullptr},
    {"tlas_min", AT(pack.tlas_min), UP, 2, INT_MAX, ">= 2"},
    {"cull_roots", AT(cull_roots), 0, -1, 1, "-1 (auto), 0 or 1"},
    {"sort_rounds", AT(sort_rounds), 0, -1, 64, "-1 (automatic), 0 (off) or 1 .. 64"},
    {"defer_min_nodes", AT(pack.defer_min_nodes), UP, 1, INT_MAX, ">= 1 (takes effect at the next rt_upload_scene)"},  // (tests lower it)
    {"fast_miss", AT(fast_miss), B, 0, 1, nullptr},
    {"roulette_skip", AT(roulette_skip), B, 0, 1, nullptr},
    {"park_levels", AT(park_levels), B, 0, 1, nullptr},
    {"multi_rccl", AT(multi_rccl), 0, 0, 2, "0 (peer copies), 1 (RCCL between distinct devices) or 2 (RCCL always)"},
    {"lds_top", AT(lds_top), EXP, -1, 2048, "-1 (auto), 0 (off) or a record count <= 2048"},
    {"lds_tlas", AT(lds_tlas), EXP, 0, 2, "0 (off), 1 (when it costs no occupancy) or 2 (whenever it fits)"},
    {"hybrid", AT(hybrid), EXP | B, 0, 1, nullptr},
    {"wavefront", AT(wavefront), EXP, 0, 1, "0 (off) or 1 (whenever legal)"},
};
#undef AT

const OptionRow* option_row(size_t index) { return index < sizeof(OPTION_TABLE) / sizeof(OPTION_TABLE[0]) ? &OPTION_TABLE[index] : nullptr; }

SetResult set_option(Options& opt, const char* name, int value) {
    SetResult r;
    for (const OptionRow& row : OPTION_TABLE)
        if (!r.row && strcmp(row.name, name) == 0) r.row = &row;
    if (!r.row) {
        r.error = std::string("unknown option ") + name;
    } else if ((r.row->flags & OPT_EXPERIMENT) && !RT_EXPERIMENTS && value != 0) {
        // (0 = "off" is what this build does anyway, and what every such row accepts: scripts that reset their options keep working)
        r.error = std::string("option ") + name + " belongs to the measured-slower experiments: "
                  "build with -DRT_EXPERIMENTS=1 (tools/build_variant.sh exp -DRT_EXPERIMENTS=1)";
    } else if (r.row->flags & OPT_BOOLEAN) {
        value = value ? 1 : 0;
    } else if (value < r.row->lo || value > r.row->hi || ((r.row->flags & OPT_NOT_ONE) && value == 1)) {
        r.error = std::string(name) + " must be " + r.row->must_be;
    }
    if (!r.error.empty()) return r;
    r.row->at(opt) = (r.row->flags & OPT_ONE_IS_AUTO) && value == 1 ? -1 : value;
    r.effects = r.row->flags & OPT_EFFECTS;
    return r;
}

TerminalScene terminal_skip_scene(const Quad* head, const rtd::SceneLayout& lay, uint32_t n_items, uint32_t n_meshes) {
    using namespace rtd;
    TerminalScene t;
    if (!head || n_meshes == 0u || n_meshes > 32u) return t;
    auto finite = [](float f) { return (as_bits(f) & 0x7f800000u) != 0x7f800000u; };
    bool colours_finite = true;
    float c[3] = {0.0f, 0.0f, 0.0f};
    bool have_c = false;
    for (uint32_t i = 0; i < n_meshes; ++i) {
        // rt_material: color, emission_color, specular_color, absorption, (absorption_strength, emission_strength, ...)
        const Quad* m = head + (lay.mat_off + (size_t)i * MATERIAL_BYTES) / 16u;
        const Quad &col = m[0], &ec = m[1], &sc = m[2];
        const volatile float es = m[4].y;  // (the product as the kernels form it: one binary32 multiplication each)
        const volatile float ex = ec.x * es, ey = ec.y * es, ez = ec.z * es, ew = ec.w * es;
        if ((as_bits(ex) | as_bits(ey) | as_bits(ez) | as_bits(ew)) != 0u) continue;
        t.dark |= 1u << i;
        const float both[2][4] = {{col.x, col.y, col.z, col.w}, {sc.x, sc.y, sc.z, sc.w}};
        for (const float* v : {both[0], both[1]}) {
            for (int k = 0; k < 4; ++k) colours_finite = colours_finite && finite(v[k]);
            for (int k = 0; k < 3; ++k) c[k] = have_c && !(v[k] > c[k]) ? c[k] : v[k];
            have_c = true;
        }
    }
    // the items in the kernels' order: everything from the first lane-sparse one on has to be dark
    bool sparse_seen = false, all_dark_behind = true;
    for (uint32_t it = 0; it < n_items; ++it) {
        const Quad* q = head + (lay.item_off + (size_t)it * ITEM_BYTES) / 16u;
        const uint32_t kind = as_bits(q[0].x), ia = as_bits(q[0].y);
        if (kind & ITEM_TLAS) return TerminalScene{0u, t.dark, {0.0f, 0.0f, 0.0f}};
        if (kind & ITEM_FOREST) {
            sparse_seen = true;
            const uint32_t n = as_bits(q[0].w);
            for (uint32_t j = 0; j < n; ++j) {
                const uint32_t mesh = as_bits(head[(lay.forest_off + (size_t)(ia + j) * FOREST_ENTRY_BYTES) / 16u].y);
                all_dark_behind = all_dark_behind && mesh < n_meshes && ((t.dark >> mesh) & 1u) != 0u;
            }
            continue;
        }
        if ((kind & ITEM_FLAT2) == 0u && as_bits(q[1].z) == 0u) sparse_seen = true;  // (an internal root, walked on its own)
        if (sparse_seen) all_dark_behind = all_dark_behind && ia < n_meshes && ((t.dark >> ia) & 1u) != 0u;
    }
    if (sparse_seen && all_dark_behind && colours_finite && have_c) {
        t.ok = 1u;
        for (int k = 0; k < 3; ++k) t.c[k] = c[k];
    }
    return t;
}

}  // namespace rt2
