// launch_options.h -- the options of rt_set_option in one table, and the rules that turn them into a launch.  Plain C++
// without HIP, like the host packer: set, refused and evaluated on a machine without a GPU (tests/test_options_host.py,
// tests/test_launch_rules_host.py).  include/rt_abi.h documents every option; the rules that keep state on the handle
// from one call to the next are launch_state.h's; rt_api.hip keeps the HIP calls: what touches the handle's buffers, the
// device's memory or a stream.
#ifndef RT_LAUNCH_OPTIONS_H
#define RT_LAUNCH_OPTIONS_H

#include <algorithm>
#include <climits>

#include "scene_pack.h"  // PackOptions (and <string>, <cstring>, include/rt_abi.h: rt_params, the codes)

#ifndef RT_EXPERIMENTS
#define RT_EXPERIMENTS 0
#endif
#ifndef RT_MIN_WAVES
#define RT_MIN_WAVES 5
#endif

namespace rt2 {

// The kernels' figures that the rules read (csrc/rt_device.h, which needs HIP: rt_api.hip asserts that they agree).
constexpr uint32_t BLOCKS_PER_CU = RT_MIN_WAVES, WAVES_PER_BLOCK = 4, MAX_BATCH_FRAMES = 64, PIPE_MAX = 8;  // (PIPE_MAX: most frames in flight)
constexpr size_t CU_LDS_BYTES = 160u * 1024u;

// Every value rt_set_option sets, under the option's name, with its default.
struct Options {
    int kernel_variant = -1, persistent_blocks = 0;  // (persistent_blocks: 0 until rt_create has asked the device, CUs x BLOCKS_PER_CU)
    int specialise = 1, lds_scene = 1, stack_wide = -1, cull_roots = -1, cross_prune = 0;  // which kernels run, and on what
    int pixel_cache = 1, primary_table = 1, primary_hits = 1, memo_in_table = 1, primary_per_slot = 1, fast_miss = 1, roulette_skip = 1;  // the pixel memo
    int vote_eighths = -1, vote_patience = -1;
    int tile_feedback = 1, tile_feedback_period = 8;
    int pipeline = -1, pipeline_when_idle = 0, frame_ahead = -1;  // one-frame calls
    int batch_frames = 32, batch_tile_major = 1, multi_rccl = 1;  // frame sequences, the gather of rt_render_multi
    int sort_rounds = -1, park_levels = 1, max_device_mb = 0;  // deferred walks; the cap on what the library allocates on its own
    int lds_top = 0, lds_tlas = 0, hybrid = 0, wavefront = 0;  // (the experiments build's)
    PackOptions pack;  // tlas, forest, flat2, tlas_min, defer_min_nodes
    size_t max_device_bytes() const { return (size_t)max_device_mb << 20; }
};

enum : uint32_t {
    OPT_BOOLEAN = 1u,               // any non-zero value stores 1 (else: lo <= value <= hi is accepted)
    OPT_UPLOAD = 2u,                // takes effect at the next rt_upload_scene
    OPT_EXPERIMENT = 4u,            // a library without RT_EXPERIMENTS accepts 0 only
    OPT_DROPS_PRIMARY = 8u,         // the primary tables hold hits found under the other setting
    OPT_RESETS_TILES = 16u,         // the tile history starts again
    OPT_CLEARS_AHEAD_FAILED = 32u,  // the automatic frames rendered ahead may try again
    OPT_ONE_IS_AUTO = 64u,          // 1 is stored as -1
    OPT_NOT_ONE = 128u,             // 1 is refused inside the range
    OPT_EFFECTS = OPT_DROPS_PRIMARY | OPT_RESETS_TILES | OPT_CLEARS_AHEAD_FAILED,  // what rt_set_option owes its handle
};
struct OptionRow {
    const char* name;
    int& (*at)(Options&);
    uint32_t flags;
    int lo, hi;           // the values it can hold (INT_MIN / INT_MAX: no bound)
    const char* must_be;  // the error text after "<name> must be "
};
const OptionRow* option_row(size_t index);  // (null past the last row)

// Sets `name` to `value`: the text of a refusal (empty: set), the row (null: unknown name) and the OPT_EFFECTS (none after
// a refusal).
struct SetResult {
    uint32_t effects = 0;
    const OptionRow* row = nullptr;
    std::string error;
    int code() const { return error.empty() ? RT_OK : RT_ERR_INVALID_ARGUMENT; }
};
SetResult set_option(Options& opt, const char* name, int value);

// ---- the rules that read them: plain arithmetic over the options and a few numbers of the launch ----

// Frames in flight of the pipelined single frames; `queues`: the hardware queues the host asked the runtime for.
// The pipeline keeps up to four streams of a handle busy, and ROCm maps a process's streams onto GPU_MAX_HW_QUEUES hardware
// queues (default 4): with a fifth stream in the process -- the null stream, a framework's copy stream -- two of them
// share a queue and, if those are two of the pipeline's, their launches serialise (measured: 1.30 -> 1.42 ms per frame,
// 1.34 -> 1.60 at two frames in flight).  The library does not touch the environment (the variable is the host's, read
// when the HIP runtime initialises: INTEGRATION.md section 3; the Python package and bench.py set it before they load
// anything): the automatic depth is four frames in flight when the host has asked for five queues or more, three
// otherwise (1.29 against 1.23 ms per frame on four queues).  A rank of a strip split whose share no longer fills the
// machine (world >= 4: 518 K pixels and fewer for 328 K resident lanes) runs seven frames deep when the host has asked for
// twelve queues or more -- room for the seven streams beside the host's own (a framework's compute and copy streams,
// RCCL's): a frame's latency is then set by its longest pixel chain, not by its work (rank 0's share of config 2 at
// world 8: 0.226 -> 0.207 ms per frame; profiles/r04_strip_pipeline_depth.txt).
inline int pipeline_depth(const Options& opt, int queues, uint32_t world) {
    if (opt.pipeline >= 0) return opt.pipeline;
    if (world >= 4 && queues >= 12) return 7;
    return queues >= 5 ? 4 : 3;
}

// How many frames a call that continues an accumulation renders at once (0: just its own).  `counters`: rt_set_counters;
// `failed`: a batch could not be set up once; `scene_in_lds`: the uploaded scene fits the LDS; `host_waits`: the call
// found the handle's stream idle.  Automatic: only when the host runs ahead of the device -- a host that waits for every
// frame gets its frame from a launch of its own, never behind frames it has not asked for --, and then only for scenes
// staged in LDS (rays of known cost) and shares so small that a launch of their own leaves lanes idle -- in units of a
// config-2 frame (1920 x 1080, 8 spp, 5 segments: 1.13 ms), batches of about 4 ms: 28 frames for a strip share of eight
// ranks (0.201 ms per frame pipelined -> 0.16), 14 for one of four (0.404 -> 0.30), 7 for one of two (0.647 -> 0.59), and
// none for the whole frame, whose pipelined launches (1.15 ms) a batch of three (1.2 ms) does not beat
// (tools/strip_scaling.py, profiles/r04_strip_scaling.txt).
inline uint32_t ahead_depth(const Options& opt, const rt_params& params, bool counters, bool failed, bool scene_in_lds,
                            uint64_t need_texels, bool host_waits) {
    if (params.debug_flag != 0 || params.rays_per_pixel <= 0 || counters || params.frames < 1) return 0;
    if (opt.frame_ahead >= 0) return opt.frame_ahead >= 2 ? std::min<uint32_t>((uint32_t)opt.frame_ahead, MAX_BATCH_FRAMES) : 0u;
    if (failed || host_waits) return 0;
    const double segments = (double)need_texels * (double)params.rays_per_pixel *
                            (double)((params.number_of_bounces < 0 ? 0 : params.number_of_bounces) + 1);
    // (Scenes read from global memory: rays of unknown cost -- the rule of round 4, "up to 8 frames and about 33 ms by a
    // work estimate", guessed a frame time and needed a timing probe to take the guess back; a host that wants batches on
    // such a scene asks for them: frame_ahead = 8 gives config 5's geometry 4.43 -> 3.40 ms per call.)
    if (!scene_in_lds || !opt.lds_scene) return 0;
    const double ms = segments / (1920.0 * 1080.0 * 8.0 * 5.0) * 1.13;
    const double d = 4.0 / (ms > 1e-3 ? ms : 1e-3);
    const uint32_t n = d >= (double)MAX_BATCH_FRAMES ? MAX_BATCH_FRAMES : (uint32_t)d;
    return n >= 6u ? n : 0u;
}

// Rounds of an automatic deferred-walk sequence (option "sort_rounds" = -1) over `park_records` pixels (times frames of
// the batch) and a deferred mesh of `defer_internal` internal nodes; 0: none.
inline uint32_t automatic_rounds(size_t park_records, int rays_per_pixel, uint32_t defer_internal) {
    // (work of the launch in units of one 1920 x 1080 frame at 16 samples per pixel)
    const double units = (double)park_records * (double)(rays_per_pixel > 0 ? rays_per_pixel : 0) / (1920.0 * 1080.0 * 16.0);
    // (tuned on the config 3 and config 5 stand-ins: the longer the walks -- the bigger the mesh's BVH --, the earlier a
    // round pays for its fixed cost, its longest chain of dependent segments, which only a big launch amortises)
    if (defer_internal >= 400000u)
        // (config 5 stand-in at 3840 x 2160, 64 spp, 16 frames per launch = 256 units: 102.9 / 98.4 / 96.8 / 96.8 / 97.3 ms
        // per frame with 8 / 12 / 16 / 24 / 32 rounds)
        // (32 frames per launch = 512 units: 95.6 ms with 16 rounds, 95.0 with 24)
        return units >= 384.0 ? 24u : units >= 96.0 ? 16u : units >= 48.0 ? 12u : units >= 24.0 ? 8u : units >= 12.0 ? 4u : units >= 4.0 ? 3u : units >= 2.0 ? 2u : 0u;
    return units >= 24.0 ? 6u : units >= 12.0 ? 4u : units >= 8.0 ? 3u : 0u;
}

// The intersection vote (path_begin).  `rounds`: inside a deferred-walk sequence; `costly`: scene read from global memory
// or walked by the many-mesh kernels.  The more a traversal costs beside the rest of an iteration, the longer it pays to
// let the lanes on memoised primary segments catch up first: 6/8 of the lanes or 3 iterations when the scene is in LDS
// and walked by the few-mesh kernels (config 2: 1.221 ms per frame; 1.222 with 7/8 and 16, 1.366 with 8/8), 7/8 or 16
// iterations otherwise (sponza-sized stand-in 10.69 -> 10.21 ms, 200-mesh stand-in 5.00 -> 4.85), every lane or 16
// iterations in a deferred-walk sequence, whose resumed pixels arrive in every phase (config 3 stand-in 5.86 -> 5.45,
// config 5 geometry 3.35 -> 3.22; profiles/r03_experiments/ab_*_vote*.txt).
inline void vote_thresholds(const Options& opt, bool rounds, bool costly, uint32_t& eighths, uint32_t& patience) {
    eighths = opt.vote_eighths >= 0 ? (uint32_t)opt.vote_eighths : rounds ? 8u : costly ? 7u : 6u;
    patience = opt.vote_patience >= 0 ? (uint32_t)opt.vote_patience : (rounds || costly) ? 16u : 3u;
}

// 0 persistent waves with lane refill, 1 one wave per tile.
inline uint32_t kernel_variant_for(const Options& opt, uint64_t tiles, uint32_t n_batch, bool counters) {
    // auto: with about one tile per resident wave there is nothing to refill from, and the
    // plain one-wave-per-tile dispatch is a little faster (tools/strip_scaling.py)
    const uint32_t resident_waves = (uint32_t)opt.persistent_blocks * WAVES_PER_BLOCK;
    uint32_t variant = opt.kernel_variant >= 0 ? (uint32_t)opt.kernel_variant : (tiles * 4 <= (uint64_t)resident_waves * 5 ? 1u : 0u);
    if (n_batch) variant = 0;   // (frame, tile) work items are the persistent kernel's
    if (counters) variant = 0;  // (the counter instantiations exist for the persistent kernel only)
    return variant;
}

// Frames per launch of a sequence of n_frames cut into batches of equal size of at most `cap` (>= 1) frames (20 frames at
// 16 per launch: 10 + 10, not 16 + 4)
inline uint32_t equal_batch(uint32_t n_frames, uint32_t cap) {
    const uint32_t launches = (n_frames + cap - 1) / cap;
    return launches ? (n_frames + launches - 1) / launches : 0;
}

// Frames of a batch that a lane renders back to back for the pixel it took (RenderArgs::frame_group; 1: every frame of a
// tile is a work item of its own).  The work items of a grouped launch are (tile, group) pairs, ceil(n_batch / G) groups
// per tile: a lane that finishes its pixel's frame starts the pixel's next frame itself, with the memo it already holds,
// instead of handing the pixel back to be taken -- and its 64-byte table entry to be read -- once per frame.  Groups
// need the tile-major order (a tile's frames are neighbours there) and a plain launch (the launches of a deferred-walk
// sequence hand pixels on through park records), and they are taken by the few-mesh kernels on a scene staged in LDS
// only (`costly`, as for the vote, is every other launch: on the 200-mesh stand-in at 16 frames per launch groups of 4
// were 2.4 % SLOWER, 4.436 -> 4.543 ms per frame, on the sponza-sized one at 64 per launch 0.5 %: their items are long as
// it is).
// What a group saves grows as 1 - 1 / G; what it costs is the launch's tail, which lasts as long as an item, G frames of a
// tile.  Config 2 at 64 frames per launch (405 tile-frames per resident wave): 1.019 ms per frame ungrouped, 0.943 /
// 0.896 / 0.882 / 0.899 with G = 2 / 4 / 8 / 16; at 20 per launch (127 per wave): 1.026, and 0.948 / 0.916 / 0.950 / 1.035
// (profiles/frame_groups_ab.txt).  So G is the largest value up to FRAME_GROUP_CAP and n_batch that leaves the launch
// FRAME_GROUP_MIN_ITEMS_PER_WAVE items per resident wave -- 8 at 64 frames per launch of the whole frame, 5 at 20, 1 (no
// groups) for a strip share of eight ranks, 0.8 tiles per resident wave, at the 28 frames of its batches -- and then the
// smallest value that needs no more groups (20 frames at 8 per group: 7 + 7 + 6, not 8 + 8 + 4; the same number of
// pixels taken, a shorter longest item).  -DRT_FRAME_GROUP=1 compiles the groups out of the kernels.
// The taper (frame_taper_table, below) cuts that tail where it arises: the tiles pulled while little work is left behind
// them get groups of G / 2, G / 4, ... 1 frames, so the launch ends on items of one frame and G prices the head alone.
// A launch that carries a taper table therefore takes its head from the same rule under a cap and a floor of its own,
// FRAME_GROUP_CAP_TAPERED and FRAME_GROUP_MIN_ITEMS_PER_WAVE_TAPERED (frame_group_tapered_for): a whole batch and 6 items
// per resident wave.  Config 2 under the taper, ms per frame by the head: 64 per launch 0.8641 / 0.8558 / 0.8486 / 0.8448 /
// 0.8433 / 0.8427 with heads of 8 / 11 / 16 / 22 / 32 / 64; 20 per launch 0.8908 / 0.8799 / 0.8717 / 0.8685 with 5 / 7 / 10 / 20
// (profiles/frame_head_ab.txt; the taper's alpha stays 4: 2 and 8 are slower under every head).  So the whole frame's
// batches start from items of a whole batch -- 64 at 64 frames per launch, 20 at 20: its 32,400 tiles alone are 6.3 items
// per resident wave --, and a strip share of eight ranks from groups of 8 at 64 frames per launch and of 3 at its 28.
// A launch without a table -- the first launch of a shape, another batch size, no tile order yet, option tile_feedback
// off -- keeps the cap and the floor above (8 / 5 / 2 / 1 for the same four launches): untapered, groups of 16 are slower
// than groups of 8, so a long head never runs without its table (launch_state.h: TileSchedule decides).
#ifndef RT_FRAME_GROUP
#define RT_FRAME_GROUP 8
#endif
#ifndef RT_FRAME_GROUP_FLOOR  // (the item floor, for tools/build_variant.sh: profiles/frame_taper_ab.txt section 6)
#define RT_FRAME_GROUP_FLOOR 24
#endif
#ifndef RT_FRAME_GROUP_TAPERED  // (the cap and the floor of a launch with a taper table, for tools/build_variant.sh)
#define RT_FRAME_GROUP_TAPERED 64
#endif
#ifndef RT_FRAME_GROUP_FLOOR_TAPERED
#define RT_FRAME_GROUP_FLOOR_TAPERED 6
#endif
constexpr uint32_t FRAME_GROUP_CAP = RT_FRAME_GROUP, FRAME_GROUP_MIN_ITEMS_PER_WAVE = RT_FRAME_GROUP_FLOOR;
// (-DRT_FRAME_GROUP=1 compiles the groups out: no head either)
constexpr uint32_t FRAME_GROUP_CAP_TAPERED = FRAME_GROUP_CAP > 1u ? RT_FRAME_GROUP_TAPERED : 1u,
                   FRAME_GROUP_MIN_ITEMS_PER_WAVE_TAPERED = RT_FRAME_GROUP_FLOOR_TAPERED;
static_assert(FRAME_GROUP_CAP >= 1 && FRAME_GROUP_CAP <= MAX_BATCH_FRAMES, "RT_FRAME_GROUP: 1 .. 64");
// (a head is at most a batch: the kernels' fields hold MAX_BATCH_FRAMES -- rt_kernel.hip asserts them beside the fields)
static_assert(FRAME_GROUP_CAP_TAPERED >= 1 && FRAME_GROUP_CAP_TAPERED <= MAX_BATCH_FRAMES, "RT_FRAME_GROUP_TAPERED: 1 .. 64");
inline uint32_t frame_group_for(uint32_t n_batch, uint64_t tiles, uint32_t resident_waves, bool tile_major, bool rounds,
                                bool costly = false, uint32_t cap = FRAME_GROUP_CAP, uint32_t floor = FRAME_GROUP_MIN_ITEMS_PER_WAVE) {
    if (n_batch < 2u || !tile_major || rounds || costly) return 1u;
    uint32_t g = std::max(std::min(cap, n_batch), 1u);
    while (g > 1u && tiles * ((n_batch + g - 1u) / g) < (uint64_t)resident_waves * floor) g -= 1u;
    const uint32_t groups = (n_batch + g - 1u) / g;
    return (n_batch + groups - 1u) / groups;
}
// ... and the head of a launch that carries a taper table: the same rule under the tapered cap and floor
inline uint32_t frame_group_tapered_for(uint32_t n_batch, uint64_t tiles, uint32_t resident_waves, bool tile_major, bool rounds,
                                        bool costly = false) {
    return frame_group_for(n_batch, tiles, resident_waves, tile_major, rounds, costly, FRAME_GROUP_CAP_TAPERED,
                           FRAME_GROUP_MIN_ITEMS_PER_WAVE_TAPERED);
}

// The taper of a grouped launch (RenderArgs::frame_taper): the tile order, heaviest first, is cut into at most
// TAPER_MAX_SEGMENTS segments of ranks, and the tiles of a segment are cut into ceil(n / g) groups of the segment's own g
// frames.  The table: TAPER_HEAD_WORDS words {segments, items of the launch, n, G}, then per segment {first rank of the
// tile order, g, first item index}.  The rule reads the tile costs (rays per tile of an earlier frame) as a histogram over
// TAPER_BINS bins in the order's own sense -- frame_taper_bin: bin 0 holds the heaviest tiles, a bin's tiles are
// neighbours in the order --, count[b] tiles in bin b and weight[b] = the sum of their effective costs c' = max(cost -
// floor, 0) (frame_taper_effective; `floor`: the rays a tile is charged for segments that the primary table serves at
// almost no cost, 64 x rays_per_pixel when the launch has a complete table: sky tiles count as no work).  With R(b) =
// the weight of bins b and later, bin b takes the largest g of G, ceil(G / 2), ceil(G / 4), ..., 1 with
//     g x (weight[b] / count[b]) x alpha x waves <= n x R(b):
// an item is at most 1 / alpha of what every resident wave still has to do when the item is pulled.  A bin without
// effective cost takes G (sky tiles keep their groups: their takes would cost more than the tail they leave), neighbours
// of equal g merge, empty bins are skipped, and while more than TAPER_MAX_SEGMENTS segments result the bins are merged
// in pairs and the rule runs again.  G <= 1, n < 2 or waves = 0: one segment of G.  The host and rt_frame_taper_kernel
// evaluate this one function (products in double: the same IEEE operations in the same order on both sides); count and
// weight are scratch (merged in place).  -DRT_FRAME_TAPER=0 compiles the taper out of the kernels and the host.
#ifndef RT_FRAME_TAPER
#define RT_FRAME_TAPER 1
#endif
#ifndef RT_FRAME_TAPER_ALPHA
#define RT_FRAME_TAPER_ALPHA 4
#endif
#ifdef __HIP__
#define RT_RULE_FN __host__ __device__ inline
#else
#define RT_RULE_FN inline
#endif
constexpr uint32_t TAPER_MAX_SEGMENTS = 8, TAPER_BINS = 64, TAPER_HEAD_WORDS = 4, TAPER_WORDS = TAPER_HEAD_WORDS + 3u * TAPER_MAX_SEGMENTS;
constexpr uint32_t TILE_ORDER_BINS = 2048;  // (rt_tile_order_kernel's counting sort; a taper bin is TILE_ORDER_BINS / TAPER_BINS of them)
constexpr uint32_t FRAME_TAPER_ALPHA = RT_FRAME_TAPER_ALPHA;
static_assert(TILE_ORDER_BINS % TAPER_BINS == 0 && FRAME_TAPER_ALPHA >= 1, "taper bins are whole runs of order bins");
RT_RULE_FN uint32_t frame_taper_bin(uint32_t cost, uint32_t max_cost) {
    const unsigned long long scale = max_cost ? max_cost : 1u;
    const unsigned long long b = (unsigned long long)(cost < max_cost ? cost : max_cost) * (TILE_ORDER_BINS - 1u) / scale;
    return ((TILE_ORDER_BINS - 1u) - (uint32_t)b) / (TILE_ORDER_BINS / TAPER_BINS);
}
RT_RULE_FN uint32_t frame_taper_effective(uint32_t cost, uint32_t cost_floor) { return cost > cost_floor ? cost - cost_floor : 0u; }
RT_RULE_FN void frame_taper_table(uint32_t* count, unsigned long long* weight, uint32_t bins, uint32_t n, uint32_t head, uint32_t waves,
                                  uint32_t alpha, uint32_t* table) {
    const uint32_t G = head ? head : 1u;
    const bool plain = G <= 1u || n < 2u || waves == 0u;
    for (;;) {
        unsigned long long behind = 0;
        for (uint32_t b = 0; b < bins; ++b) behind += weight[b];
        uint32_t segments = 0, rank = 0, item = 0, last = 0;
        bool over = false;
        for (uint32_t b = 0; b < bins && !over; ++b) {
            if (count[b] == 0u) continue;
            uint32_t g = G;
            if (!plain) {
                const double have = (double)n * (double)behind * (double)count[b];
                while (g > 1u && (double)g * (double)alpha * (double)waves * (double)weight[b] > have) g = (g + 1u) / 2u;
            }
            if (segments == 0u || g != last) {
                if (segments == TAPER_MAX_SEGMENTS) {
                    over = true;
                    break;
                }
                uint32_t* seg = table + TAPER_HEAD_WORDS + 3u * segments;
                seg[0] = rank;
                seg[1] = g;
                seg[2] = item;
                segments += 1u;
                last = g;
            }
            rank += count[b];
            item += count[b] * ((n + g - 1u) / g);
            behind -= weight[b];
        }
        if (!over) {
            if (segments == 0u) {  // (no tiles)
                table[TAPER_HEAD_WORDS] = 0u;
                table[TAPER_HEAD_WORDS + 1u] = G;
                table[TAPER_HEAD_WORDS + 2u] = 0u;
                segments = 1u;
            }
            table[0] = segments;
            table[1] = item;
            table[2] = n;
            table[3] = G;
            for (uint32_t w = TAPER_HEAD_WORDS + 3u * segments; w < TAPER_WORDS; ++w) table[w] = 0u;
            return;
        }
        const uint32_t half = (bins + 1u) / 2u;  // (at TAPER_MAX_SEGMENTS bins and fewer nothing is over)
        for (uint32_t b = 0; b < half; ++b) {
            const bool two = 2u * b + 1u < bins;
            count[b] = count[2u * b] + (two ? count[2u * b + 1u] : 0u);
            weight[b] = weight[2u * b] + (two ? weight[2u * b + 1u] : 0ull);
        }
        bins = half;
    }
}
// ... and its histogram on the host, from the costs themselves (the device builds the same one: rt_frame_taper_kernel)
inline void frame_taper_histogram(const uint32_t* cost, uint32_t n_tiles, uint32_t max_cost, uint32_t cost_floor, uint32_t* count,
                                  unsigned long long* weight) {
    for (uint32_t b = 0; b < TAPER_BINS; ++b) count[b] = 0u, weight[b] = 0ull;
    for (uint32_t t = 0; t < n_tiles; ++t) {
        const uint32_t b = frame_taper_bin(cost[t], max_cost);
        count[b] += 1u;
        weight[b] += frame_taper_effective(cost[t], cost_floor);
    }
}

// The terminal skip (csrc/rt_kernel.hip: intersect_scene's TERM; RenderArgs::terminal_dark, ::terminal_c).  A path segment
// whose path is certain to end at its hit -- the last allowed bounce, or a roulette value that no dark material's
// throughput can reach -- and whose closest hit so far is a dark mesh leaves the lane-sparse items of the mesh loop out:
// the forest items and the single meshes with an internal root that is not a two-leaf one.  That is exact when everything
// it leaves out, and everything behind it, is dark too.  A mesh is DARK when the four products emission_color *
// emission_strength are +0 bitwise.  terminal_skip_scene reads the packed head (the items in the order the kernels visit
// them, the forest entries, the materials) and says
//   ok   1 iff the scene has a lane-sparse item, every mesh of the first such item and of every item behind it is dark,
//        no item is a top-level tree, there are at most 32 meshes (the mask) and every dark material's color and
//        specular_color components are finite;
//   dark bit i: mesh i is dark (all of them, wherever their items are);
//   c    the componentwise maximum of color.xyz and specular_color.xyz over the dark meshes (ok only).
// terminal_skip_for adds the launch: the few-mesh kernels on a scene staged in LDS in their SIMPLE instantiation -- no
// glass, no texture, no sphere, so a hit makes 8 draws --, no counters (the shader's test counts stay exact), no parking.
// The result is the mask the launch runs with, 0: nothing is skipped.  -DRT_TERMINAL_SKIP=0 compiles the skip out.
#ifndef RT_TERMINAL_SKIP
#define RT_TERMINAL_SKIP 1
#endif
struct TerminalScene {
    uint32_t ok = 0, dark = 0;
    float c[3] = {0.0f, 0.0f, 0.0f};
};
TerminalScene terminal_skip_scene(const Quad* head, const rtd::SceneLayout& lay, uint32_t n_items, uint32_t n_meshes);
inline uint32_t terminal_skip_for(const TerminalScene& t, bool scene_in_lds, bool many_mesh, bool takes_simple, bool counters, bool parks,
                                  bool enabled = true) {
    // (an experiments build has none: its wavefront sequence keeps two pointers in the arguments' slot, RenderArgs)
    return RT_TERMINAL_SKIP != 0 && !RT_EXPERIMENTS && enabled && t.ok != 0u && scene_in_lds && !many_mesh && takes_simple && !counters && !parks ? t.dark : 0u;
}

// The fixed switches (csrc/rt_kernel.hip: the FIXED instantiations of the persistent SIMPLE render kernels on a scene staged
// in LDS, grouped and ungrouped; fix_switches).  The render kernels carry wave-uniform switches that have one value in every
// default launch -- each a scalar register or two across the render loop, a branch and a dead path.  A FIXED instantiation
// compiles the values below in: the same operations, a branch whose condition is known.  FixedSwitches states each value
// once, for the kernels and for the rule; FixedSwitchValues is what a launch has in those places (the RenderArgs fields of
// the same names; `primary`: the launch has a primary table; `spp_reciprocal`: 1 / rays_per_pixel is exact, a power of
// two), and fixed_switches_ok is true exactly when every compiled-in constant equals the launch's value -- a switch that
// the kernels only test against zero is compared as such.  `grouped_kernel`: the launch takes the grouped kernel, which
// has the batch's three switches compiled in too (a batch, in tile-major order, in frame groups); the ungrouped one runs
// single frames, pipelined frames and ungrouped batches and keeps those three as the launch has them.  A frame without a
// complete table (the first one behind a camera change), an option switched off, 3 samples per pixel, no skybox and a
// strip share run the general kernel; a counter launch and a scene with a sphere never get here (rt_kernel.hip:
// render_takes_fixed asks for the SIMPLE kernel first).  -DRT_FIXED_SWITCHES=0 compiles the instantiations out.
#ifndef RT_FIXED_SWITCHES
#define RT_FIXED_SWITCHES 1
#endif
struct FixedSwitches {
    static constexpr uint32_t stack_wide = 0;        // one dword per stack entry
    static constexpr uint32_t forest_cull = 1;       // forest members behind their root boxes
    static constexpr uint32_t roulette_skip = 1, fast_miss = 1;
    static constexpr uint32_t pixel_cache = 1;       // the memo in LDS
    static constexpr uint32_t primary_complete = 1;  // ... and equal to the pixel's table entry (so: a table)
    static constexpr uint32_t skybox = 1;
    static constexpr uint32_t strip_world = 1;       // the whole frame
    static constexpr uint32_t batch_tile_major = 1;
    // (tested against zero only: the launch's own value stays in its place)
    static constexpr bool terminal_dark = true, primary = true, spp_reciprocal = true, samples = true, batch = true, grouped = true;
};
struct FixedSwitchValues {
    uint32_t stack_wide, forest_cull, roulette_skip, fast_miss, terminal_dark, pixel_cache, primary, primary_complete;
    int32_t skybox, rays_per_pixel;
    uint32_t spp_reciprocal, strip_world, batch_frames, batch_tile_major, frame_group;
};
inline bool fixed_switches_ok(const FixedSwitchValues& v, bool grouped_kernel) {
    using F = FixedSwitches;
    return RT_FIXED_SWITCHES != 0 && v.stack_wide == F::stack_wide && (v.forest_cull != 0u) == (F::forest_cull != 0u) &&
           (v.roulette_skip != 0u) == (F::roulette_skip != 0u) && (v.fast_miss != 0u) == (F::fast_miss != 0u) &&
           (v.terminal_dark != 0u) == F::terminal_dark && v.pixel_cache == F::pixel_cache && (v.primary != 0u) == F::primary &&
           (v.primary_complete != 0u) == (F::primary_complete != 0u) && (v.skybox != 0) == (F::skybox != 0u) &&
           (v.rays_per_pixel > 0) == F::samples && (v.spp_reciprocal != 0u) == F::spp_reciprocal && v.strip_world == F::strip_world &&
           (!grouped_kernel || ((v.batch_frames != 0u) == F::batch && (v.batch_tile_major != 0u) == (F::batch_tile_major != 0u) &&
                                (v.frame_group > 1u) == F::grouped));
}

// workgroups that fit a CU's 160 KiB of LDS (BLOCKS_PER_CU when the register budget is the limit)
inline uint32_t blocks_per_cu_for(size_t lds_bytes) {
    const uint32_t per_cu = lds_bytes ? (uint32_t)(CU_LDS_BYTES / lds_bytes) : BLOCKS_PER_CU;
    return per_cu > BLOCKS_PER_CU ? BLOCKS_PER_CU : per_cu < 1u ? 1u : per_cu;
}
// ... and the persistent grid at that occupancy (option "persistent_blocks" counts BLOCKS_PER_CU per CU)
inline uint32_t persistent_blocks_for(const Options& opt, size_t lds_bytes) {
    const uint32_t blocks = (uint32_t)opt.persistent_blocks;
    const uint32_t fit = (blocks / BLOCKS_PER_CU) * blocks_per_cu_for(lds_bytes);
    return fit < blocks && fit > 0 ? fit : blocks;
}

}  // namespace rt2

#endif
