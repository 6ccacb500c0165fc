/* rt_test_abi.h -- test-only entry points (round 5: out of the product library).
 *
 * The product, ray_tracer_2_amd/librt2_mi355x.so, exports include/rt_abi.h and nothing else.  The entry points below
 * exist only in ray_tracer_2_amd/librt2_mi355x_test.so: the SAME sources and compile flags plus -DRT_TEST_ENTRIES=1
 * (ray_tracer_2_amd/build.py: build_test_library), which also exports every symbol of rt_abi.h, so that a test can
 * drive a handle and these entry points through one library.  tests/test_abi.py checks both export lists.
 */
#ifndef RT_TEST_ABI_H
#define RT_TEST_ABI_H

#include "rt_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Test-only: the device's evaluation of the kernels' arithmetic building blocks, element-wise over
 * host arrays of n floats (bit patterns for integer inputs/outputs).  fn: 0 log, 1 cos, 2 sin, 3 exp,
 * 4 exp2, 5 log2, 6 pow(x,y), 7 acos, 8 atan2(x,y), 9 sqrt, 10 x/y, 11 rand() from RNG state bits x,
 * 12 next_random_number of state x (bits), 13 trig_signbits(x) (bits), 14 rand_normal_dist() from
 * state x, 15 f32(u32 bits x) * 2^-32, 16 normalize(x, y, x*y).x, 17 the kernels' reciprocal rcp_(x), 18 their
 * sqrt_dev(x), 19 the RNG jumps of the roulette skip for state x (bits), y (bits) selecting the value: 0 / 1 the generator's
 * output 5 steps on, by one jump / by stepping next_random_number; 2 / 3 the output 12 steps on; 4 / 5 the state 12 steps
 * on, 20 the RNG jump of the terminal skip for state x (bits), y (bits): 0 / 1 the generator's output 8 steps on, by one
 * jump / by stepping next_random_number; 2 / 3 the state 8 steps on.  The second call filters one RGBA8 sRGB texture at n (u, v) pairs (wgsl:455 as csrc/rt_texture.h defines
 * it).  The third compares the kernels' short reciprocal (which = 0) / square root (which = 1) with the compiler's IEEE
 * 1.0f / x / sqrt on the device for EVERY float in the range the short form serves, and the sky's three shortcuts
 * (which = 2, 3, 4: wgsl:215-218 with the branches of smoothstep / pow taken apart) with their literal forms for every
 * float in [-1.5, 1.5] / [0, 1.5]: out3 = {floats checked, mismatches, a mismatching bit pattern}. */
int rt_test_device_units(rt_handle* h, int fn, const float* x, const float* y, float* out, uint64_t n);
int rt_test_sweep(rt_handle* h, int which, uint64_t* out3);
int rt_test_device_sample_texture(rt_handle* h, const rt_texture_desc* tex, const float* uv, float* rgba_out,
                                  uint64_t n);

/* Test-only: the kernels' ray-scene intersection (intersect_scene) for n host-given rays on the uploaded scene, one lane
 * per ray, with the arguments a render launches and the instantiation it would take -- unless `flags` force the general
 * (RT_TEST_ISECT_GENERAL) or the SIMPLE one (RT_TEST_ISECT_SIMPLE: refused with RT_ERR_INVALID_ARGUMENT on a many-mesh scene
 * or one with spheres, glass or textures); RT_TEST_ISECT_STATS takes the counter instantiation.  A ray whose `active`
 * byte is 0 (active may be NULL: all rays) is not traced and its record stays zero.  Rays must be finite with a non-zero
 * direction (else RT_ERR_INVALID_ARGUMENT), n <= RT_TEST_ISECT_MAX_RAYS.  Record per ray, RT_TEST_ISECT_WORDS u32 words:
 * hit, dst, point xyz, normal xyz, u, v (floats as bits), backface, the winner (mesh index, or number of meshes + sphere
 * index; 0xffffffff on a miss), node tests, triangle tests (counter instantiation only), the instantiation that ran (1
 * many-mesh, 2 SIMPLE as in rt_last_launch out[3]; 32 counters, 64 scene in LDS), 0. */
#define RT_TEST_ISECT_WORDS 16
#define RT_TEST_ISECT_MAX_RAYS (1ull << 24)
#define RT_TEST_ISECT_GENERAL 1
#define RT_TEST_ISECT_STATS 2
#define RT_TEST_ISECT_SIMPLE 4
int rt_test_intersect(rt_handle* h, const float* ro, const float* rd, const uint8_t* active, uint64_t n, int flags,
                      uint32_t* out);

/* Test-only: the kernels' shading step (path_end: sky, glass, diffuse / specular mix, emission, texture, russian roulette,
 * end-of-sample bookkeeping; which = RT_TEST_SHADE_PATH_END) or the pre-step's roulette skip (roulette_skip; which =
 * RT_TEST_SHADE_ROULETTE_SKIP) for n host-given lane states on the uploaded scene's materials and textures, one lane per
 * case, with the prologue of the render kernels and the instantiation a render would take -- unless `flags` force the
 * general (RT_TEST_SHADE_GENERAL) or the SIMPLE one (RT_TEST_SHADE_SIMPLE: refused on a many-mesh scene or one with
 * spheres, glass or textures).  RT_TEST_SHADE_NO_FAST_MISS takes path_end's FAST_MISS = false instantiation (the counter
 * builds') instead of the product's; RT_TEST_SHADE_TOTAL_REGS the one that keeps the pixel sum in registers instead of
 * the lane's LDS state.  The arguments are a render's (a copy of the handle's) with pixel_cache = 0 and fast_miss = 0 and
 * the call's number_of_bounces, rays_per_pixel and skybox.  A case whose `active` byte is 0 (active may be NULL: all
 * cases) stays out of the call and its record stays zero.  Floats may be anything, non-finite values included.
 * RT_ERR_INVALID_ARGUMENT, before anything reaches the device: an object index outside the scene, a mode other than
 * RT_TEST_SHADE_STEP_END / _STEP_TRAVERSE, an unknown `which` or flag, both GENERAL and SIMPLE, n > RT_TEST_SHADE_MAX_CASES.
 * Case, RT_TEST_SHADE_WORDS u32 words (floats as bits): rd xyz, T xyzw, light xyzw, total xyzw, RNG state, seg, j, mode,
 * hit, dst, point xyz, normal xyz, u, v, backface, object (mesh index, or number of meshes + sphere index: word 11 of the
 * intersect record), meta (PixelState::meta: the pixel's ray count in bits 0-15).  The roulette skip reads object, RNG
 * state, j, total and meta only (its memo word is the object's material | hit).
 * Record, RT_TEST_SHADE_WORDS words: ro xyz (zero going in), rd xyz, T xyzw, light xyzw, total xyzw (from the LDS where it
 * lives there), RNG state, seg, j, fresh, the return value, the n_segments increment, meta, the instantiation that ran (1
 * many-mesh, 2 SIMPLE, 32 FAST_MISS = false, 64 scene in LDS, 128 pixel sum in LDS), the more_reused increment (the roulette
 * skip's dead count), zeros. */
#define RT_TEST_SHADE_WORDS 32
#define RT_TEST_SHADE_MAX_CASES (1ull << 20)
#define RT_TEST_SHADE_PATH_END 0
#define RT_TEST_SHADE_ROULETTE_SKIP 1
#define RT_TEST_SHADE_STEP_END 0
#define RT_TEST_SHADE_STEP_TRAVERSE 3
#define RT_TEST_SHADE_GENERAL 1
#define RT_TEST_SHADE_NO_FAST_MISS 2
#define RT_TEST_SHADE_SIMPLE 4
#define RT_TEST_SHADE_TOTAL_REGS 8
int rt_test_shade(rt_handle* h, int which, const uint32_t* cases, const uint8_t* active, uint64_t n, int number_of_bounces,
                  int rays_per_pixel, int skybox, int flags, uint32_t* out);

/* Test-only: the uploaded scene's blob as the kernels read it (out may be NULL; else bytes >= its size, which
 * layout_out[9] gives), its SceneLayout (csrc/rt_scene_format.h, 12 words) and its device address.  Waits for the launches
 * enqueued on the handle's streams. */
int rt_test_scene_blob(rt_handle* h, void* out, uint64_t bytes, uint32_t layout_out[12], uint64_t* device_ptr);

/* Test-only, no device and no handle: the host packer (csrc/host/scene_pack.h) on scene arrays -- both phases, as
 * rt_upload_scene runs them -- with the five options it reads: options = {tlas, forest, flat2, tlas_min, defer_min_nodes}.
 * Two calls, like rt_test_scene_blob: out = NULL returns the sizes (layout_out[9] = bytes of the blob); else bytes >= that
 * and out receives the blob as the device would hold it: head, tail, zero padding.  layout_out: the SceneLayout
 * (csrc/rt_scene_format.h, 12 words).  facts_out, RT_TEST_PACK_FACTS words: the instance phase's n_items, n_tlas_records,
 * n_forest_entries, tlas_entries, has_tlas, has_forest, plain_materials, have_defer, defer_mesh, defer_xform,
 * defer_internal; the geometry phase's max_height, max_leaf_ref, top_mesh_records, top_mesh_base, roots_are_unions,
 * any_deep; and 1 when a second run of the instance phase on the same geometry facts gave the same head and layout.
 * Returns the packer's code; error text: rt_last_error(NULL). */
#define RT_TEST_PACK_FACTS 18
int rt_test_pack_scene(const rt_sphere* spheres, uint32_t n_spheres, const rt_mesh_uniform* meshes, uint32_t n_meshes,
                       const rt_packed_triangle* triangles, uint32_t n_triangles, const rt_node* nodes, uint32_t n_nodes,
                       const int32_t options[5], void* out, uint64_t bytes, uint32_t layout_out[12],
                       uint32_t facts_out[RT_TEST_PACK_FACTS]);

/* Test-only: raw copy of a buffer of the last wavefront sequence (which: 0 path state, 1 hit records, 2 the two slot
 * lists, 3 the per-round list counts; layouts in csrc/rt_device.h), or (which = 4) the pixels parked in front of each round
 * of the last deferred-walk sequence (72 u32), or (which = 5, 6) the park records of its even / odd rounds. */
int rt_test_read_wavefront(rt_handle* h, int which, void* out, uint64_t bytes);
/* The grouped ncclSend / ncclRecv gather of rt_render_multi against the RCCL-shaped library at `lib_path`, on fake
 * buffers and without any HIP call (runs without a GPU): checks that a failure inside the group still closes the group
 * and aborts the communicators.  Error text: rt_last_error(NULL). */
int rt_test_rccl_gather(const char* lib_path, int n_ranks);
/* The automatic depth of option "frame_ahead" for a one-frame call that continues an accumulation (no GPU needed): the
 * scene staged in LDS (1) or read from global memory (0), the texels of the call's share, samples per pixel, bounces,
 * and whether the host counts as one that waits for every frame.  0 = the call renders its own frame only. */
int rt_test_frame_ahead_depth(int lds_scene, uint64_t texels, int rays_per_pixel, int number_of_bounces, int host_waits);

/* The option table (csrc/host/launch_options.cpp), no device and no handle.  rt_test_option_table: row `index` -- its name
 * and info_out = {lower bound, upper bound of the values it can hold (INT_MIN / INT_MAX: none), default, flags};
 * RT_ERR_INVALID_ARGUMENT past the last row.  rt_test_set_option: the setter behind rt_set_option on a fresh set of options -- returns its code, error text
 * in rt_last_error(NULL); stored_out = {the value of that option the library would act on now (0 for an unknown name),
 * the side effects rt_set_option owes its handle: the RT_TEST_OPT_DROPS_PRIMARY / RESETS_TILES / CLEARS_AHEAD_FAILED bits}. */
#define RT_TEST_OPTION_NAME_BYTES 32
#define RT_TEST_OPT_BOOLEAN 1             /* any non-zero value stores 1 */
#define RT_TEST_OPT_UPLOAD 2              /* takes effect at the next rt_upload_scene */
#define RT_TEST_OPT_EXPERIMENT 4          /* a library without RT_EXPERIMENTS accepts 0 only */
#define RT_TEST_OPT_DROPS_PRIMARY 8       /* invalidates the primary tables */
#define RT_TEST_OPT_RESETS_TILES 16       /* resets the tile history */
#define RT_TEST_OPT_CLEARS_AHEAD_FAILED 32
#define RT_TEST_OPT_ONE_IS_AUTO 64        /* 1 is stored as -1 */
#define RT_TEST_OPT_NOT_ONE 128           /* 1 is refused inside the range */
int rt_test_option_table(uint32_t index, char name_out[RT_TEST_OPTION_NAME_BYTES], int32_t info_out[4]);
int rt_test_set_option(const char* name, int value, int32_t stored_out[2]);

/* One launch rule of csrc/host/launch_options.h (no device, no handle); option values go in as rt_test_set_option stored
 * them.  in / out per rule:
 *   VOTES    {vote_eighths, vote_patience, in a deferred-walk sequence, scene in global memory or many-mesh} -> {eighths, patience}
 *   ROUNDS   {pixels x frames of the launch, rays_per_pixel, internal nodes of the deferred mesh} -> {automatic rounds}
 *   VARIANT  {kernel_variant, persistent_blocks, tiles, frames of the batch (0: single frame), counters on} -> {variant}
 *   DEPTH    {pipeline, GPU_MAX_HW_QUEUES, world} -> {frames in flight}
 *   BATCH    {frames of the sequence, most frames per launch} -> {frames per launch}
 *   GRID     {LDS bytes per workgroup, persistent_blocks} -> {workgroups per CU, persistent grid}
 *   FRAME_GROUP {frames of the batch, tiles of the launch, resident waves, tile-major order, rounds planned,
 *                scene in global memory or many-mesh}
 *               -> {frames per work item, the compile-time cap RT_FRAME_GROUP}
 *   FRAME_GROUP_TAPERED the same inputs: the head of a launch that carries a taper table (frame_group_tapered_for)
 *               -> {frames per work item, the cap RT_FRAME_GROUP_TAPERED | the item floor RT_FRAME_GROUP_FLOOR_TAPERED << 16}
 *   FRAME_TAPER {frames of the batch, head group size G, resident waves, the order's max_cost, the cost floor, tiles,
 *                the address of a u32 array: the tiles' costs, then RT_TEST_TAPER_WORDS words that receive the table,
 *                alpha (0: the shipped constant)}
 *               -> {segments of the table, the alpha used}: frame_taper_table over the costs' histogram, on the host
 *   TERMINAL_SKIP {the address of a packed blob (rt_test_pack_scene's), the address of its 12 layout words, its n_items,
 *                the number of meshes, the scene is staged in LDS and walked by the few-mesh kernels, the launch takes
 *                SIMPLE, the launch counts tests, the address of three floats that receive terminal_c (zeros when refused)}
 *               -> {terminal_skip_ok, the mask of the dark meshes}: terminal_skip_scene and terminal_skip_for */
#define RT_TEST_RULE_VOTES 0
#define RT_TEST_RULE_ROUNDS 1
#define RT_TEST_RULE_VARIANT 2
#define RT_TEST_RULE_DEPTH 3
#define RT_TEST_RULE_BATCH 4
#define RT_TEST_RULE_GRID 5
#define RT_TEST_RULE_FRAME_GROUP 6
#define RT_TEST_RULE_FRAME_TAPER 7
#define RT_TEST_RULE_FRAME_GROUP_TAPERED 8
#define RT_TEST_TAPER_WORDS 28 /* {segments, items, frames of the batch, G}, then {first rank, group size, first item} x 8 */
#define RT_TEST_RULE_TERMINAL_SKIP 9
int rt_test_launch_rule(int which, const int64_t in[8], int64_t out[2]);

/* The terminal skip of a handle's render launches (RenderArgs::terminal_dark: path segments that cannot matter leave the
 * forest walk out).  on >= 0 switches it for the handle's later launches: 1, the default, lets the rule decide
 * (terminal_skip_for), 0 makes every launch walk everything; on < 0 changes nothing.  last_out (may be NULL), four
 * words: the dark-mesh mask the handle's last render launch ran with (0: it skipped nothing), then the bits of its
 * terminal_c. */
int rt_test_terminal_skip(rt_handle* h, int on, uint32_t last_out[4]);

/* The fixed switches (csrc/host/launch_options.h: FixedSwitches, fixed_switches_ok; the FIXED instantiations of the
 * persistent SIMPLE render kernels, grouped and ungrouped).  rt_test_fixed_switches: on >= 0 switches them for the handle's later launches -- 1, the default,
 * lets the rule decide, 0 makes every launch run the general kernels; on < 0 changes nothing.  last_out (may be NULL): 1 if the
 * handle's last render launch ran the FIXED instantiation (rt_last_launch out[3] bit 5).
 * rt_test_fixed_switches_rule (no device, no handle): the rule on a launch's values, in the order of FixedSwitchValues --
 * {stack_wide, forest_cull, roulette_skip, fast_miss, terminal_dark, pixel_cache, has a primary table, primary_complete,
 * skybox, rays_per_pixel, spp_reciprocal != 0, strip_world, batch_frames, batch_tile_major, frame_group} -> out[0] = the
 * rule's answer, bit 0 for a launch that takes the grouped kernel, bit 1 for one that takes the ungrouped kernel, out[1] = RT_FIXED_SWITCHES, out[2 ..]: the constants the kernel compiles in, in the same order (a switch that
 * is only tested against zero: 1 for "not zero"; frame_group: 1 for "more than one"). */
#define RT_TEST_FIXED_SWITCHES 15
int rt_test_fixed_switches(rt_handle* h, int on, uint32_t* last_out);
int rt_test_fixed_switches_rule(const int64_t in[RT_TEST_FIXED_SWITCHES], int64_t out[2 + RT_TEST_FIXED_SWITCHES]);

/* The frame groups of a handle's batches (RenderArgs::frame_group: the frames of a pixel that one lane renders back to
 * back).  force >= 0 sets the group size of the handle's later batches, with or without a taper table, 0 = the rules
 * decide (frame_group_for, and frame_group_tapered_for for a launch that carries a table); a
 * frame-major order, a deferred-walk sequence and a library built with -DRT_FRAME_GROUP=1 still render with 1.
 * force < 0 changes nothing.  last_out (may be NULL): the group size of the handle's last launch. */
int rt_test_frame_group(rt_handle* h, int force, uint32_t* last_out);

/* The taper of a handle's grouped batches (RenderArgs::frame_taper: the tile order cut into segments, each with a group
 * size of its own).  n_segments >= 1 forces the segments {first_rank[k], size[k]} -- first ranks ascending from 0, sizes
 * 1..64, at most 8 -- on the handle's later batches in place of the rule's table; a batch that takes no groups (see
 * rt_test_frame_group) ignores them.  0: the rule decides again; < 0 changes nothing.  table_out (may be NULL):
 * RT_TEST_TAPER_WORDS words, the table of the handle's last launch, zeros if it ran without one. */
int rt_test_frame_taper(rt_handle* h, int n_segments, const uint32_t* first_rank, const uint32_t* size, uint32_t* table_out);
/* The device's evaluation of the taper rule on n_tiles host-given costs (the kernel that runs behind a new tile order),
 * every input the caller's -- rule FRAME_TAPER of rt_test_launch_rule is the host's evaluation of the same function. */
int rt_test_frame_taper_rule(rt_handle* h, const uint32_t* cost, uint32_t n_tiles, uint32_t max_cost, uint32_t cost_floor,
                             uint32_t n_batch, uint32_t head, uint32_t waves, uint32_t alpha, uint32_t* table_out);

/* The rays per 8x8 tile that the handle's last cost-recording launch counted (option "tile_feedback": the first frame of
 * a batch, or a single frame): n_tiles counts in tile order, read after everything queued on the handle is done. */
int rt_test_tile_costs(rt_handle* h, uint32_t* out, uint32_t n_tiles);

/* The rules of a handle that keep state from call to call (csrc/host/launch_state.h), no device and no handle.  Each entry
 * point runs a whole sequence: it starts from a fresh state, takes n call records and fills n decision records.
 *
 * rt_test_tile_schedule: rt2::TileSchedule, the schedule of render launches' tile order, taper table and cost recording.
 * A call is a launch -- its shape, frames of the batch (0: a single frame), the head it would take with a taper table,
 * option tile_feedback_period, and flags: the handle has a taper buffer, the taper is compiled in, the step applies to the
 * launch (option tile_feedback on, no debug view, tiles within the tables, the persistent kernel), and RESET: the effect of
 * an option with RT_TEST_OPT_RESETS_TILES comes before the launch.  The decision, and the state behind it. */
#define RT_TEST_TILE_TAPER_BUFFER 1
#define RT_TEST_TILE_TAPER_COMPILED 2
#define RT_TEST_TILE_APPLIES 4
#define RT_TEST_TILE_RESET 8
typedef struct rt_test_tile_call {
    uint32_t width, height, rank, world;
    uint32_t n_batch, tapered_head;
    int32_t period;
    uint32_t flags;
} rt_test_tile_call;
typedef struct rt_test_tile_decision {
    uint32_t rewrite_order, order_from, write_taper, use_order, take_head, record_costs, record_into;
    uint32_t have_order, costs_ready, order_age, cost_slot, taper_head, taper_batch; /* the state after the launch */
} rt_test_tile_decision;
int rt_test_tile_schedule(const rt_test_tile_call* calls, uint32_t n, rt_test_tile_decision* out);

/* rt_test_ahead_sequence: rt2::AheadSequence driven the way render_single, render_impl and rt_set_option drive it, with the
 * device's part of each call replaced by the record's word.  kind FRAME: a one-frame call (params, rank, world) on a handle
 * whose option frame_ahead is `frame_ahead` (-1: automatic, the depth is rt2::ahead_depth's for a scene staged in LDS or
 * not, `texels` of the call's share and a host that waits or not); batch_fails: the batched launch the call would start
 * cannot be set up.  kind BATCHED: a launch of n_frames frames through the batched path (rt_render_frames).  kind BUMP:
 * something bumps the handle's generation (rt_set_camera with another camera, an upload ...).  kind SET_OPTION: option
 * frame_ahead is set (again): a bump, and the automatic depth may try again.
 * The decision: slot >= 0, the call blended that slot of the batch in flight; began, the frames of the batch it started
 * (0: none); plain, it rendered its own frame in a launch of its own; and behind the call: a batch is in flight, the ramp,
 * the automatic depth has failed once, and the frames asked for / speculative as rt_get_stats reports them. */
#define RT_TEST_AHEAD_FRAME 0
#define RT_TEST_AHEAD_BATCHED 1
#define RT_TEST_AHEAD_BUMP 2
#define RT_TEST_AHEAD_SET_OPTION 3
typedef struct rt_test_ahead_call {
    uint32_t kind;
    rt_params params;
    uint32_t rank, world;
    int32_t frame_ahead;
    uint32_t scene_in_lds, host_waits, batch_fails, n_frames;
    uint64_t texels;
} rt_test_ahead_call;
typedef struct rt_test_ahead_decision {
    int32_t slot;
    uint32_t continues, began, plain;
    uint32_t in_flight, ramp, failed_once;
    uint32_t frames, frames_speculative;
} rt_test_ahead_decision;
int rt_test_ahead_sequence(const rt_test_ahead_call* calls, uint32_t n, rt_test_ahead_decision* out);

/* rt_test_primary_choice: rt2::choose_primary, the primary table of a launch, on n rows of RT_TEST_PRIMARY_FACTS words
 * {primary_table, primary_hits, primary_per_slot (the options), the camera differs from the last sampled frame's, frames of
 * the batch, the launch is pipelined, pixel_cache, debug_flag, rays_per_pixel, counters on, then for the shared table and
 * for the slot's own: serves as it stands, large enough, may grow under the cap} -> RT_TEST_PRIMARY_CHOICE words {table: 0
 * none, 1 shared, 2 the slot's own; want_hits; rebuild; owed before a rebuild: 0 nothing, 1 the slot's stream is
 * synchronised, 2 every stream is drained; barrier_other is owed}. */
#define RT_TEST_PRIMARY_FACTS 16
#define RT_TEST_PRIMARY_CHOICE 5
int rt_test_primary_choice(const int32_t* facts, uint32_t n, uint32_t* out);

/* Test-only: the BVH builder's SAH plane search (find_best_split, bvh.rs:299-351) for host-given nodes, without a build
 * around it: device -1 runs the host search (csrc/host/bvh.cpp: make_host_level_search, no GPU needed), device >= 0 the
 * kernels of csrc/rt_bvh_search.hip (make_device_level_search).  tri9: nine floats per triangle (centroid, min, max; any
 * values, non-finite ones included); order: the n triangle ids in their current order; a query is a node -- positions
 * [start, start + count) of `order` and the node's box.  The queries are given level by level: level l has
 * level_counts[l] of them (0 allowed), consecutive in `queries`; all n_levels levels go, in turn, through ONE search
 * object (the device buffers a level outgrows are reallocated, as in a build).  out: one result per query.
 * RT_ERR_INVALID_ARGUMENT, before anything reaches the device, for a null array, an order entry >= n, count < 2 (the
 * builder never asks, and host and device answer differently) or start + count > n; a HIP error is RT_ERR_DEVICE.
 * Error text: rt_last_error(NULL). */
typedef struct rt_test_sah_query {
    uint32_t start, count;
    float aabb_min[3], aabb_max[3];
} rt_test_sah_query;
typedef struct rt_test_sah_result {
    int32_t axis;
    float pos, cost;
} rt_test_sah_result;
int rt_test_sah_search(int device, const float* tri9, uint64_t n, const uint32_t* order, const rt_test_sah_query* queries,
                       const uint32_t* level_counts, uint32_t n_levels, rt_test_sah_result* out);

#ifdef __cplusplus
}
#endif

#endif
