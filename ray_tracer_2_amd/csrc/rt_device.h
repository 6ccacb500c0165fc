// rt_device.h -- device-side data layout shared by rt_api.hip (upload) and
// rt_kernel.hip (render).  The reference's arrays (include/rt_abi.h) are
// re-laid-out once at upload time for 16-byte vector loads; every derived
// value is computed with the same IEEE operations the shader would execute
// per ray, so the re-layout is results-preserving.
#ifndef RT_DEVICE_H
#define RT_DEVICE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rt_abi.h"
#include "rt_scene_format.h"  // SceneLayout, the record sizes and flags of the blob

// Features that were built, parity-tested and measured SLOWER than what ships -- the LDS-staged top of a big mesh's BVH
// (option "lds_top"), the LDS-staged top-level tree ("lds_tlas"), the hybrid launches of a deferred-walk sequence
// ("hybrid") and the wavefront sequence ("wavefront"); measurements in DESIGN.md sections 5.4 / 5.5 -- are compiled only
// with -DRT_EXPERIMENTS=1 (tools/build_variant.sh exp -DRT_EXPERIMENTS=1 -> librt2_mi355x_exp.so; their parity tests run
// against that build: RT2_LIB=... pytest).  The product library contains none of their kernels and rejects the options.
#ifndef RT_EXPERIMENTS
#define RT_EXPERIMENTS 0
#endif

// Experiment of round 5 (tools/experiments/README.md): two-level records for rt_walk_kernel --
// the record of an internal node carries its children's boxes AND a copy of both children's own records (192 B), so that
// the near-first descent fetches once per two levels.  -DRT_WALK2=1 (tools/build_variant.sh walk2 -DRT_WALK2=1).
#ifndef RT_WALK2
#define RT_WALK2 0
#endif

namespace rtd {

// Occupancy target: workgroups of 256 threads (one wave per SIMD) resident per CU = waves per
// SIMD.  The render kernels are compiled for that register budget (512 / RT_MIN_WAVES VGPRs) and
// the LDS budget per workgroup is the CU's 160 KiB divided by it.
#ifndef RT_MIN_WAVES
#define RT_MIN_WAVES 5
#endif
constexpr uint32_t BLOCKS_PER_CU = RT_MIN_WAVES;
constexpr uint32_t LDS_BUDGET_BYTES = 160 * 1024 / BLOCKS_PER_CU;
constexpr uint32_t BLOCK_THREADS = 256;
constexpr uint32_t WAVES_PER_BLOCK = BLOCK_THREADS / 64;
// Per-lane state kept in LDS instead of registers (see path_step): the pixel's running sum
// `total`, 4 floats.  It is touched once per path but would otherwise occupy 4 VGPRs across the
// whole traversal.
#ifndef RT_TOTAL_IN_LDS
#define RT_TOTAL_IN_LDS 1   // 0 (experiment): the pixel sum stays in registers in every kernel
#endif
constexpr uint32_t LANE_STATE_DWORDS = RT_TOTAL_IN_LDS ? 4 : 0;
// The same in the kernels that read the scene from global memory: held in registers the sum was spilled
// around the traversal in every iteration (6 scratch stores + 6 loads per wave-iteration = 1.2 GB of writes
// per frame on the config 3 stand-in, profiles/r02_dragon9_summary.txt); 4 KiB of LDS per workgroup.
#ifndef RT_TOTAL_LDS_GLOBAL
#define RT_TOTAL_LDS_GLOBAL 1
#endif
constexpr bool total_in_lds(bool lds_scene) { return RT_TOTAL_IN_LDS != 0 && (lds_scene || RT_TOTAL_LDS_GLOBAL != 0); }
// Per-lane primary-ray memo (see path_step): rd, hit record (dst, point, normal, u, v), and
// one word = mat_off | hit | backface << 1 | ray valid << 2 | hit valid << 3.
constexpr uint32_t PIXEL_MEMO_DWORDS = 13;
// LDS of a workgroup beside the scene (the render kernels' LDS map): every wave's BVH stack (two dwords per entry and
// lane when `stack_wide`), tree stack and cost tables, and its per-lane regions -- the pixel sum (`lane_state`) and
// the primary-ray memo (`pixel_memo`) when they live in LDS.
inline uint64_t wave_lds_bytes(uint32_t stack_entries, bool stack_wide, uint32_t tlas_entries, bool lane_state, bool pixel_memo) {
    const uint64_t lane_dwords = (uint64_t)stack_entries * (stack_wide ? 2u : 1u) + tlas_entries +
                                 (lane_state ? LANE_STATE_DWORDS : 0u) + (pixel_memo ? PIXEL_MEMO_DWORDS : 0u);
    return (lane_dwords * 64u + 8u * 3u) * sizeof(uint32_t) * WAVES_PER_BLOCK;
}

struct DTexture {
    const uint8_t* rgba8;
    uint32_t width, height;
};

struct Counters {
    unsigned long long segments;
    unsigned long long paths;
    unsigned long long node_tests;
    unsigned long long triangle_tests;
    unsigned long long reused;  // segments whose hit came from the primary-ray memo (no traversal)
};

// Kernel argument block (lives in kernarg SGPRs).
struct RenderArgs {
    rt_params params;
    rt_camera_uniform camera;
    const float4* blob;  // the scene, see SceneLayout
    SceneLayout lay;
    const DTexture* textures;
    const float* srgb_lut;
    float4* image;  // full frame, or compact strips when strip_world > 1
    Counters* counters;
    uint32_t* work_counter;  // persistent kernel: next 8x8 tile to hand out (zeroed per launch)
    const uint32_t* tile_order;  // optional: tiles sorted by last frame's cost, heaviest first
    uint32_t* tile_cost;         // optional: rays per tile of this frame (feeds the next frame's order)
    uint32_t n_meshes, n_spheres, n_textures, n_items;
    uint32_t stack_entries;  // per-lane BVH stack depth
    uint32_t stack_wide;     // 1 => two dwords per entry (a leaf reference does not fit one dword)
    uint32_t tlas_entries;   // per-lane TLAS stack depth (1 dword per entry), >= 1
    uint32_t many_mesh;      // 1 => use the kernels with top-level trees / root-box culling compiled in
    uint32_t simple;         // 1 => no spheres, no glass, no textured material, camera without jitter: the few-mesh product
                             // kernels have an instantiation with those branches compiled out (option "specialise")
    uint32_t pixel_cache;    // per-lane primary-ray memo (PIXEL_MEMO_DWORDS per lane): 0 off, 1 in LDS,
                             // 2 in `pixel_cache_mem` (persistent kernel only, when LDS has no room)
    uint32_t* pixel_cache_mem;
    const void* primary;     // primary table of the frame (rt_primary_kernel: one 64-byte memo entry per pixel -- the constant
                             // primary ray and, with option "primary_hits", its hit), or null: compute per pixel
    uint32_t primary_complete;  // != 0: the table holds the hits too, so a lane's memo EQUALS its table entry for the whole pixel
                             // (memo_hit_store rewrites the same bits): park records leave the memo out and a resumed pixel
                             // reloads it from the table
    float spp_reciprocal;     // 1 / rays_per_pixel when that is a power of two (exact), else 0
    float blend_weight, blend_rest;  // 1 / f32(frames + 1) and 1 - that (wgsl:157-158)
    float memo_ro[3];        // (origin + right * 0) + up * 0: the memoised primary rays' common origin
    uint32_t vote_eighths;   // intersection vote: run when wanting lanes * 8 >= lanes * vote_eighths
    uint32_t vote_patience;  // ... or when somebody has waited this many iterations
    uint32_t strip_rank, strip_world;
    uint32_t tiles_x, tiles_y;  // 8x8 tiles of the (local) image
    uint32_t count_tests;       // 1 => accumulate node/triangle test counters
    uint32_t kernel_variant;    // 0 = persistent waves + lane refill, 1 = one wave per tile
    uint32_t persistent_blocks; // grid size of the persistent kernel
    uint32_t lds_scene;         // 1 => the blob is staged into LDS
    uint32_t forest_cull;       // 1 => forest members are skipped when the ray misses their root box
    uint32_t cull_roots;        // 1 => skip a mesh with an internal root when the ray misses the root box
    // Cross-mesh pruning (option "cross_prune"; many-mesh product kernels): a tree box, a mesh's
    // root box or a BVH box whose entry distance lies beyond what the closest hit so far allows -- t_cut, a local-space
    // bound with a written error budget and 12.5 % of slack on top -- is not entered.  The counter (STATS) and debug
    // kernels never prune.
    uint32_t cross_prune;
    // Frame batch (rt_render_frames): one persistent launch renders frames params.frames ..
    // params.frames + batch_frames - 1; work items are (frame, tile) pairs, frame k's samples go
    // unblended to image + k * batch_stride and rt_blend_frames_kernel applies wgsl:154-161 in frame
    // order afterwards.  0 = a plain one-frame launch that blends in place.
    uint32_t batch_frames;
    uint32_t batch_tile_major;  // 1 => work items in (tile, frame) order instead of (frame, tile)
    unsigned long long batch_stride;  // texels between the scratch frames
    // LDS-staged top of a big mesh's BVH (scenes read from global memory): wide records top_base ..
    // top_base + top_count - 1 -- the first levels of the biggest mesh, numbered breadth-first at upload
    // -- are copied into LDS by every workgroup (coalesced 16-byte loads) and read from there.
    uint32_t top_base, top_count;
    // LDS-staged top-level tree (many-mesh scenes read from global memory; option "lds_tlas"): all tlas_lds wide
    // records of the scene's top-level tree(s) are copied into LDS by every workgroup, behind the staged BVH top;
    // 0 = read in place.
    uint32_t tlas_lds;
    // Deferred walks (option "sort_rounds"; scenes with one big mesh, few-mesh kernels).  The walk through a big
    // mesh is entered by a few lanes of a wave at a time and costs the whole wave its full length.  With park != 0
    // a render launch does not walk that mesh (its item, ITEM_DEFER, is the last of the mesh loop -- the order of the
    // loop is free): a lane whose ray can enter it PARKS its pixel -- the pixel's state and the closest-hit record
    // of the segment so far go to a queue in global memory (park records, below) -- and takes other work.
    // rt_walk_kernel then walks the big mesh for all parked rays, every lane fetching its next ray as soon as its
    // walk ends, and the next render launch resumes the parked pixels behind the walk: offer the mesh's hit, finish
    // the segment, go on until the next entry into the big mesh.  A pixel's operations and their order are those of
    // the undeferred loop, so the image is the same bit for bit; the last launch of a sequence has park = 0 and
    // walks what is left inline.
    uint32_t fast_miss;           // != 0: a memoised primary ray that misses ends its pixel in one step (path_end, option "fast_miss")
    uint32_t roulette_skip;       // != 0: the samples that die at the roulette of a memoised primary hit are not shaded (path_step's pre-step, option "roulette_skip")
    uint32_t park;
    uint32_t park_levels;        // != 0: a ray parks only if the walk's first two levels reach a grandchild box (option "park_levels")
    float4* q_in;                 // park records to resume instead of tiles (null: the work items are tiles)
    const uint32_t* q_in_count;   // their number (written by the launch before)
    // (one slot of the kernarg segment for two launches that exclude each other -- a grouped launch never parks, its
    // instantiations have no PARK --, so that every field keeps its place and no kernel's argument offsets move)
    union {
        float4* q_out;            // where this launch parks
        // The taper of a grouped launch (host/launch_options.h: frame_taper_table), or null: every tile in groups of
        // frame_group.  rt2::TAPER_WORDS words: {segments, items, batch_frames, frame_group}, then {first rank of the tile
        // order, frames per group, first item index} per segment: a segment's tiles are cut into groups of its own size.
        const uint32_t* frame_taper;
    };
    uint32_t* q_out_count;
    uint32_t defer_mesh, defer_xform;  // the deferred mesh and the mesh whose matrices give its local ray
#if RT_WALK2
    const float4* walk2;               // 12 float4 per internal node of the deferred mesh: its wide record, then copies of
    uint32_t walk2_base;               // its two children's wide records (zeros for a leaf child); index = wide index - base
#endif
    // Hybrid launch of a deferred-walk sequence (option "hybrid"): `blob` / `lay` are the SMALL blob -- the scene without
    // the deferred mesh's BVH and triangles, staged into LDS -- and only a winner on the deferred mesh reads its shading
    // record from the full blob in global memory.
    uint32_t hybrid;
    uint32_t big_shade_off;
    const float4* big_blob;
    // Wavefront sequence (option "wavefront"; many-mesh scenes).  Every ray of a many-mesh scene walks the top-level
    // tree and a few meshes, the walks are of very unequal length, and inside the render kernel a wave-iteration lasts
    // as long as its longest walk (lane utilisation 0.18 on the sponza-sized stand-in).  Here the path state of every
    // pixel of the launch lives in a SLOT in global memory and two kernels alternate: rt_wf_shade_kernel finishes a
    // segment (winner's normal / uv, shading, russian roulette, end of path / pixel) and begins the next one -- the
    // operations of path_step around the traversal, unchanged -- and lists the slots whose new segment needs a
    // traversal; rt_wf_walk_kernel intersects the scene for the listed rays with per-lane refill (a lane takes its
    // next ray the moment its walk ends) and phase-scheduled passes (box steps / leaf triangles / bookkeeping, the
    // most populated phase next).  A pixel's operations and their order are those of the undeferred loop.
    //   wf_state: 6 float4 planes per slot, blocks of 64 slots: (x | out_row << 16, rng, j | fresh << 31, seg)
    //             (ro, rd.x) (rd.yz, T.xy) (T.zw, light.xy) (light.zw, total.xy) (total.zw, meta, -)
    //   wf_hit:   2 planes: (closest, object code | any << 24 | sphere inside << 25, win_u, win_v) (win_tri, win_point)
    //             object code: mesh index, or 0x800000 | sphere index
    //   the primary-ray memo of a slot: pixel_cache_mem, 13 dwords per slot (pixel_cache == 3)
    // (the two planes' 16 bytes are one slot of the kernarg segment for two things that exclude each other, like q_out's:
    // only the wavefront kernels of the experiments build read the planes, and that build has no terminal skip)
    // Terminal skip (SIMPLE few-mesh render kernels on a scene staged in LDS; host/launch_options.h: terminal_skip_scene /
    // terminal_skip_for; intersect_scene's TERM): bit i of terminal_dark: mesh i emits nothing; 0: the launch skips nothing
    // (the rule refused, or the switch is off).  terminal_c: the componentwise maximum of color.xyz and specular_color.xyz
    // over the dark meshes.
    union {
        struct {
            float4* wf_state;
            float4* wf_hit;
        };
        struct {
            uint32_t terminal_dark;
            float terminal_c[3];
        };
    };
    const uint32_t* wf_list_in;    // slots to shade (their hits are in wf_hit) / rays to walk
    const uint32_t* wf_count_in;
    uint32_t* wf_list_out;         // slots whose next segment needs a traversal
    uint32_t* wf_count_out;
    uint32_t wf_round0;            // 1 => the shade launch that takes the pixels: slots 0 .. wf_slots - 1, no hits yet
    uint32_t wf_slots;             // slots of the launch = wf_frame_slots x frames
    uint32_t wf_frame_slots;       // slots per frame = tiles x 64 (whole 8x8 tiles; pixels outside the image stay empty)
    // Frame groups (persistent kernel, batch_frames >= 2 in tile-major order; host/launch_options.h: frame_group_for):
    // >= 2: the work items are (tile, group) pairs, group g = batch frames g * frame_group .. min(batch_frames,
    // (g + 1) * frame_group) - 1, and the lane that took a pixel renders the group's frames of that pixel back to back.
    // 0 / 1: (tile, frame) items.  (The last member: the fields above keep their places in the kernarg segment.)
    uint32_t frame_group;
};
// -DRT_FRAME_GROUP=1 compiles the frame groups out of the kernels (RT_FRAME_GROUP caps the G of the rule and has its
// default there: host/launch_options.h)
#if defined(RT_FRAME_GROUP) && RT_FRAME_GROUP <= 1
constexpr bool FRAME_GROUPS = false;
#else
constexpr bool FRAME_GROUPS = true;
#endif
// -DRT_FRAME_TAPER=0 compiles the taper out of the grouped kernels (its default and its rule: host/launch_options.h)
#if defined(RT_FRAME_TAPER) && RT_FRAME_TAPER == 0
constexpr bool FRAME_TAPER = false;
#else
constexpr bool FRAME_TAPER = FRAME_GROUPS;
#endif
constexpr uint32_t WF_STATE_PLANES = 6, WF_HIT_PLANES = 2;
// Park record of a pixel: 14 x 16 B, stored in blocks of 64 records, plane by plane (plane p of record i of block b at
// float4 index (b * PARK_PLANES + p) * 64 + i), so that the lanes of a wave, which hold consecutive records, store and
// load contiguous kilobytes.  Planes: 0 (x, out_row, rng, j)  1 (seg, fresh, meta, memo[12])  2 (ro, rd.x)
// 3 (rd.yz, T.xy)  4 (T.zw, light.xy)  5 (light.zw, win_point.yz)  6 total  7-9 memo[0..11] (left untouched when the
// primary table holds the whole memo: RenderArgs::primary_complete)  10 (closest, object, any | inside << 1, sphere
// dst)  11 (win_u, win_v, win_tri, win_point.x)  12 unused  13 the walk's result (t, u, v, tri | det sign; tri = ~0:
// no hit), written by rt_walk_kernel.  A park writes 9 planes (144 B) and a resume reads 11 (176 B) in the usual case.
constexpr uint32_t PARK_PLANES = 14;

constexpr uint32_t RT_MAX_BATCH_FRAMES = 64;  // (config 3 stand-in: 5.24 ms per frame at 32 per launch, 5.09 at 64; config 2: 1.126 / 1.119)
// rt_blend_frames_kernel: image = the accumulation image, scratch = batch frame 0
struct BlendArgs {
    float4* image;
    const float4* scratch;
    unsigned long long texels, stride;
    uint32_t n;
    int32_t frames0;  // Params.frames of batch frame 0
    float weight[RT_MAX_BATCH_FRAMES], rest[RT_MAX_BATCH_FRAMES];  // wgsl:157-158 per frame, from the host
};

// rt_gbuffer_kernel (rt_render_gbuffer): rows [row0, row0 + rows) of the width x height frame; every plane pointer
// addresses the first texel of row row0 (a NULL plane is not produced).
struct GBufferArgs {
    uint32_t width, height, row0, rows;
    float *depth, *dir, *point, *normal, *bary, *texcoord;
    float4 *albedo, *emission;
    uint32_t *object, *primitive;
    uint8_t* flags;
};
// 64-texel work items of the band: runs of 64 consecutive texels, or (tiles: the many-mesh kernels) tiles of 8x8, partial
// ones at the right and top edges included
__host__ __device__ inline uint32_t gbuffer_chunks(const GBufferArgs& g, bool tiles) {
    if (!tiles) return (uint32_t)(((unsigned long long)g.rows * g.width + 63u) / 64u);
    return ((g.width + 7u) / 8u) * ((g.rows + 7u) / 8u);
}

}  // namespace rtd

#endif
