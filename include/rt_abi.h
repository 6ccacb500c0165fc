/*
 * rt_abi.h -- C ABI of librt2_mi355x.so, the MI355X-native replacement for the
 * per-pixel path-trace loop of addiswebb/ray_tracer_2.
 *
 * Everything in this header is plain C: fixed-layout POD structs, pointers and
 * sizes.  No torch, HIP or C++ types cross the boundary.  A Rust (or any other
 * FFI-capable) host binds exactly these symbols; INTEGRATION.md shows the
 * replacement `src/rendering/ray_tracer.rs` a maintainer would add.
 *
 * Section 1 reproduces, byte for byte, the `#[repr(C)]`/bytemuck structs the
 * reference uploads to its WGSL shader (citations are relative to the
 * reference checkout).  Section 2 is the device-side API that replaces
 * `RayTracer::{new, create_gpu_resources, load_scene_gpu_resources,
 * update_buffers, render}` (src/rendering/ray_tracer.rs:49,316,237,397,420).
 * Section 3 is the host-side scene pipeline (OBJ/MTL loader, SAH BVH builder,
 * built-in scene library) that feeds it, replacing `AssetManager::load_model`
 * (src/core/asset.rs:102), `BVH::build_per_mesh` (src/core/bvh.rs:152) and
 * `Scene::instantiate_scene` (src/scene/scene.rs:179).
 */
#ifndef RT_ABI_H
#define RT_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------ */
/* 1. Data contract (byte-exact with the reference)                          */
/* ------------------------------------------------------------------------ */

/* src/core/app.rs:27-40  <->  shaders/ray_tracer.wgsl:2-12 */
typedef struct rt_params {
    uint32_t width;
    uint32_t height;
    int32_t number_of_bounces; /* a path has number_of_bounces + 1 segments */
    int32_t rays_per_pixel;
    int32_t skybox;
    int32_t frames; /* the seed: -1 after a reset, 0 first frame, ... */
    int32_t accumulate;
    int32_t debug_flag; /* 0 = path trace, 1..7 = debug views */
    int32_t debug_scale;
    float _p1[3];
} rt_params;

/* src/scene/components/material.rs:3-18  <->  wgsl:14-27 */
typedef struct rt_material {
    float color[4];
    float emission_color[4];
    float specular_color[4];
    float absorption[4];
    float absorption_strength;
    float emission_strength;
    float smoothness;
    float specular;
    float ior;
    int32_t flag; /* RT_MATERIAL_* */
    int32_t diffuse_index;
    int32_t normal_index;
} rt_material;

enum { RT_MATERIAL_DEFAULT = 0, RT_MATERIAL_GLASS = 1, RT_MATERIAL_TEXTURE = 2 };

/* src/scene/components/geometry/sphere.rs:4-10  <->  wgsl:29-33 */
typedef struct rt_sphere {
    float pos[3];
    float radius;
    rt_material material;
} rt_sphere;

/* src/scene/components/geometry/mesh.rs:52-62  <->  wgsl:35-42.
 * Matrices are column-major ([col][row]), as glam's to_cols_array_2d. */
typedef struct rt_mesh_uniform {
    float world_to_model[4][4];
    float model_to_world[4][4];
    uint32_t node_offset;
    uint32_t triangles;
    uint32_t triangle_offset;
    float _p1;
    rt_material material;
} rt_mesh_uniform;

/* src/core/bvh.rs:55-66  <->  wgsl:60-67.  left/right are mesh-local node
 * indices, first is a mesh-local triangle index, count > 0 marks a leaf. */
typedef struct rt_node {
    uint32_t left;
    uint32_t right;
    uint32_t first;
    uint32_t count;
    float aabb_min[3];
    float _p1;
    float aabb_max[3];
    float _p2;
} rt_node;

/* src/core/bvh.rs:19-34  <->  wgsl:69-82 */
typedef struct rt_packed_triangle {
    float v1[3];
    float uv10;
    float v2[3];
    float uv11;
    float v3[3];
    float uv20;
    float n1[3];
    float uv21;
    float n2[3];
    float uv30;
    float n3[3];
    float uv31;
} rt_packed_triangle;

/* src/scene/camera.rs:15-22  <->  wgsl:44-49 (84 bytes on the host) */
typedef struct rt_camera_uniform {
    float cam_to_world[4][4];
    float view_params[3]; /* plane_width, plane_height, focus_dist */
    float defocus_strength;
    float diverge_strength;
} rt_camera_uniform;

/* src/scene/scene.rs:1016-1026  <->  wgsl:51-58.  The host layout is kept
 * as is, including `nodes` at offset 100 (the shader never reads it). */
typedef struct rt_scene_uniform {
    uint32_t spheres;
    uint32_t n_vertices;
    uint32_t n_indices;
    uint32_t meshes;
    rt_camera_uniform camera;
    uint32_t nodes;
    float padding[6];
} rt_scene_uniform;

/* One RGBA8 sRGB texture as the reference uploads it
 * (src/rendering/ray_tracer.rs:237-275): tightly packed rows, already
 * flipped horizontally by the loader (src/core/asset.rs:77). */
typedef struct rt_texture_desc {
    const uint8_t* rgba8;
    uint32_t width;
    uint32_t height;
} rt_texture_desc;

/* Capacity limits the reference's fixed-size buffers impose
 * (src/rendering/ray_tracer.rs:15-19, src/core/bvh.rs:140); kept as input
 * validation. */
#define RT_MAX_MESHES 400u
#define RT_MAX_SPHERES 500u
#define RT_MAX_TRIANGLES 1375000u
#define RT_MAX_NODES 2600000u
#define RT_MAX_TEXTURES 64u
#define RT_BVH_STACK 32u /* wgsl:297 */

/* status codes: 0 = ok, negative = error (text via rt_last_error) */
enum {
    RT_OK = 0,
    RT_ERR_INVALID_ARGUMENT = -1,
    RT_ERR_CAPACITY = -2,
    RT_ERR_DEVICE = -3,
    RT_ERR_NO_SCENE = -4,
    RT_ERR_BVH_DEPTH = -5,
    RT_ERR_IO = -6,
    RT_ERR_PARSE = -7,
    RT_ERR_OUT_OF_MEMORY = -8,
    RT_ERR_INDEX_RANGE = -9
};

/* ------------------------------------------------------------------------ */
/* 2. Device side: replaces RayTracer (src/rendering/ray_tracer.rs)          */
/* ------------------------------------------------------------------------ */

typedef struct rt_handle rt_handle;

/* Counters accumulated over the rt_render* calls since the last
 * rt_reset_timing (device-side atomics, one add per wave).  `segments` counts
 * calculate_ray_collions calls (wgsl:353) = rays. */
typedef struct rt_stats {
    uint64_t segments;
    uint64_t paths;
    uint64_t node_tests;     /* AABB tests, as wgsl:322 counts them */
    uint64_t triangle_tests; /* as wgsl:307 counts them */
    float kernel_ms;         /* sum of the hipEvent times of `launches` render launches (pipelined single frames --
                              * option "pipeline" -- overlap: their sum then exceeds the wall time) */
    uint32_t launches;       /* render launches since the last rt_reset_timing */
    uint32_t frames;         /* frames the host asked for since the last rt_reset_timing (rt_render_frames: several per launch) */
    uint64_t segments_reused; /* of `segments`: primary segments whose hit was taken from the per-pixel memo
                               * (same ray as the pixel's first sample: no traversal ran); segments -
                               * segments_reused rays were traversed */
    uint32_t frames_speculative; /* frames rendered AHEAD of the host's calls (option "frame_ahead") that no call has asked for
                               * (yet): the launches, rays and times above include them; a sequence that ends mid-batch
                               * leaves them here */
    uint32_t _reserved;
} rt_stats;

/* ≙ RayTracer::new + create_gpu_resources (ray_tracer.rs:49,316): picks the
 * device, creates the stream and the RGBA32F accumulation image of up to
 * max_width x max_height texels (engine.rs:142-158). */
int rt_create(int device_ordinal, uint32_t max_width, uint32_t max_height, rt_handle** out);

/* ≙ RayTracer::update_buffers (ray_tracer.rs:397-419), to be called when the
 * scene changes instead of every frame.  All arrays are copied before return.
 * Validates capacities and BVH indices (ranges, cycles).  A BVH of height >= 32 --
 * the shader's 32-entry stack (wgsl:297) can overflow on it -- is accepted and traversed
 * with the shader's literal push/pop and index clamping, so it renders exactly as the
 * shader would. */
int rt_upload_scene(rt_handle* h, const rt_scene_uniform* scene, const rt_sphere* spheres,
                    uint32_t n_spheres, const rt_mesh_uniform* meshes, uint32_t n_meshes,
                    const rt_packed_triangle* triangles, uint32_t n_triangles,
                    const rt_node* nodes, uint32_t n_nodes);

/* The per-instance part of update_buffers: new SceneUniform, spheres and mesh uniforms for the scene of the
 * last successful rt_upload_scene / rt_upload_built_scene.  Triangles and BVH nodes stay those of that upload.
 * n_meshes and, per mesh, node_offset / triangle_offset / triangles must equal the uploaded ones; transforms,
 * materials, the camera and every sphere (count included, <= 500) may change.  The handle afterwards is exactly
 * what rt_upload_scene with the same arrays and the uploaded triangles / nodes would leave: same blob bytes, same
 * kernel choice, same images.  Only the blob's head (everything before the BVH / triangle records) is rebuilt and
 * sent: in place when its size is unchanged, else into a new allocation with the old tail copied device to device.
 * Like rt_upload_scene it waits for the launches already enqueued, drops frames rendered ahead and invalidates the
 * primary tables.  Errors: RT_ERR_NO_SCENE (nothing uploaded), RT_ERR_INVALID_ARGUMENT (a changed mesh count or
 * mesh offsets -- rt_last_error names the mesh --, counts that disagree with the SceneUniform, null arrays with
 * non-zero counts), RT_ERR_CAPACITY (more than 500 spheres), RT_ERR_OUT_OF_MEMORY (no room for a resized blob).
 * On any error nothing changes.  DESIGN.md section 2.8. */
int rt_update_instances(rt_handle* h, const rt_scene_uniform* scene, const rt_sphere* spheres, uint32_t n_spheres,
                        const rt_mesh_uniform* meshes, uint32_t n_meshes);

/* BVH refit: moved vertices, same topology.
 *
 * rt_refit_bvh (host only, no device needed) recomputes in place the node boxes of every mesh it selects: the meshes
 * whose leaf range [tri_lo, tri_hi) -- the triangles their leaves reference -- meets [first, first + n).  Other meshes
 * keep their nodes bit for bit (their boxes may be looser than a refit would make them, as in a foreign BVH), and the
 * topology fields (left, right, first, count) never change.  The box rule, which the device reproduces bit for bit
 * (csrc/rt_refit.h):
 *   - min(a, b) / max(a, b) of two floats: the smaller / larger of two ordered values; of two equal ones -0 / +0 when
 *     they are zeros of both signs; of a NaN and another value the other value (NaN only when both are NaN).  (Not libm
 *     fmin: the sign of its zero results differs between compilers, so the builder's own boxes are only defined up to
 *     the sign of zero, and a refit of unchanged vertices gives them back value for value, == on every float.)
 *   - a leaf's box: a fold over its triangles in array order, from (+FLT_MAX, -FLT_MAX), each triangle contributing
 *     min(v1, min(v2, v3)) and max(v1, max(v2, v3)) per axis (the builder's fit_bounds);
 *   - an internal node's box: min(left, right) / max(left, right), element by element.
 * No box holds a NaN; a leaf whose vertices are all NaN keeps the empty box (+FLT_MAX, -FLT_MAX).
 * Refused with RT_ERR_INVALID_ARGUMENT, nothing changed, rt_last_error(NULL) naming the mesh: a selected mesh whose leaf
 * range is not inside [first, first + n) (a mesh is refitted whole: its leaf boxes need every vertex), a selected mesh
 * whose node interval [node_offset, highest node its root reaches] overlaps that of a mesh with another triangle_offset
 * (no single node array could then describe the result), a range past n_triangles.  Invalid BVH indices give
 * RT_ERR_INDEX_RANGE as rt_upload_scene does. */
int rt_refit_bvh(const rt_mesh_uniform* meshes, uint32_t n_meshes, const rt_packed_triangle* triangles, uint32_t n_triangles,
                 rt_node* nodes, uint32_t n_nodes, uint32_t first, uint32_t n);

/* rt_refit_triangles replaces the uploaded triangles [first, first + n) and refits the uploaded BVH on the device.  The
 * handle afterwards is exactly what rt_upload_scene would leave for the uniform, spheres and meshes of the last upload or
 * update, the uploaded triangles with that range replaced, and the uploaded nodes passed through
 * rt_refit_bvh(..., first, n): the same blob bytes, SceneLayout, kernel choice (rt_last_launch), images and ray-query
 * results.  `triangles` holds n rt_packed_triangle records: device pointers on the handle's device (16-byte aligned),
 * read in order on the handle's stream like rt_intersect_rays, unless flags has RT_REFIT_HOST_MEMORY (host pointers).
 * The kernels rewrite the triangle records of the range and recompute the selected meshes' boxes bottom-up; the
 * per-mesh root facts (root box, containment, proper hierarchy) are the only thing read back -- the call returns after
 * that one small readback --, and the host then reruns the instance phase (top-level trees, forests, mesh records) and
 * commits the head as rt_update_instances does: after the launches already enqueued, dropping frames rendered ahead and
 * the primary tables; in place, or in a new allocation when the head's size changes.  Device scratch (about 72 bytes
 * per BVH record of the selected meshes, and n x 96 bytes of staging for host input) is held only during the call and
 * counts against option "max_device_mb".  Errors, all checked before anything is written, leaving the scene as it was:
 * those of rt_refit_bvh, RT_ERR_NO_SCENE, RT_ERR_INVALID_ARGUMENT (null or misaligned triangles with n > 0, unknown
 * flags, the experiments build), RT_ERR_OUT_OF_MEMORY (the cap or the device has no room for the scratch or a resized
 * blob). */
enum { RT_REFIT_HOST_MEMORY = 1 };
int rt_refit_triangles(rt_handle* h, const rt_packed_triangle* triangles, uint32_t first, uint32_t n, int flags);

/* ≙ RayTracer::load_scene_gpu_resources (ray_tracer.rs:237-315). n <= 64. */
int rt_upload_textures(rt_handle* h, const rt_texture_desc* descs, uint32_t n);

/* The cheap per-frame part of update_buffers: only the camera changed. */
int rt_set_camera(rt_handle* h, const rt_camera_uniform* camera);

/* ≙ RayTracer::render (ray_tracer.rs:420-434): one frame of wgsl `main` over
 * params->width x params->height; accumulates into the device image when
 * params->frames >= 1 (wgsl:154-161).  Asynchronous on the handle's stream. */
int rt_render(rt_handle* h, const rt_params* params);

/* n_frames consecutive frames of RayTracer::render with Params.frames advancing by one per frame, as
 * App::update does while accumulating (app.rs:44-53, 160-162): the image afterwards is bit-identical to
 * n_frames calls of rt_render with frames, frames + 1, ...  The only dependency between frames is the
 * per-texel blend (wgsl:154-161), so the frames of a batch (option "batch_frames", default 32, at most
 * 64) are sampled by ONE persistent launch over (frame, tile) work items -- the waves never drain
 * between frames -- into scratch images, and a dense second kernel blends them in frame order with
 * the shader's two operations.  Intermediate frames of a batch are not observable. */
int rt_render_frames(rt_handle* h, const rt_params* params, uint32_t n_frames);

/* Multi-GPU tile split: renders only the 8-row strips s with
 * s % world == rank into the compact local image (strip-major).  Seeds use
 * the full-frame pixel index, so the stitched image equals rt_render's. */
int rt_render_strips(rt_handle* h, const rt_params* params, uint32_t rank, uint32_t world);

/* rt_render_frames for one rank's strips. */
int rt_render_strips_frames(rt_handle* h, const rt_params* params, uint32_t n_frames, uint32_t rank,
                            uint32_t world);

/* Number of texels rt_render_strips(rank, world) writes. */
uint64_t rt_strip_texels(uint32_t width, uint32_t height, uint32_t rank, uint32_t world);

/* Scatter a gathered [world][max_local_texels][4] float device buffer
 * (rank-major, each rank padded to rt_strip_texels(.., 0, world)) into the
 * handle's full-frame image. */
int rt_assemble_strips(rt_handle* h, const void* gathered_device, uint32_t width, uint32_t height,
                       uint32_t world);

/* Single-process multi-GPU frame: per_gpu[r] (one handle per device, same scene
 * uploaded to each) renders the strips of rank r, per_gpu[0]'s device gathers them
 * device-to-device over xGMI and assembles the frame; if rgba32f_out is not NULL the
 * full frame (width*height RGBA32F) is copied there (blocking).  Every handle keeps
 * its own strip accumulation across frames.  The frame is bit-identical to rt_render's. */
int rt_render_multi(rt_handle** per_gpu, int n_gpus, const rt_params* params, float* rgba32f_out);
/* The same for n_frames consecutive frames (rt_render_strips_frames on every GPU), ONE gather at the
 * end.  Transport of the gather: RCCL (grouped ncclSend/ncclRecv, every peer on its own xGMI link to the
 * root; librccl is loaded on first use) between distinct devices, device-to-device copies (peer access
 * enabled where the devices allow it) between handles that share a device or when option "multi_rccl"
 * of per_gpu[0] is 0.  Non-blocking when rgba32f_out is NULL: a later call may follow at once (each
 * rank's next render waits for the root's copy of its previous strips). */
int rt_render_multi_frames(rt_handle** per_gpu, int n_gpus, const rt_params* params, uint32_t n_frames,
                           float* rgba32f_out);
/* Blocking read of the frame the last rt_render_multi* call assembled on the root. */
int rt_read_multi_frame(rt_handle* root, float* rgba32f_out, size_t bytes);

/* ≙ copy_texture_to_buffer in save_render_to_file (app.rs:341-407): blocking
 * copy of width*height RGBA32F texels (row 0 = bottom of the view). */
int rt_read_image(rt_handle* h, float* rgba32f_out, size_t bytes);
/* The two halves of rt_read_image for a host that shows every frame (the reference blits the storage texture every
 * redraw, src/rendering/renderer.rs): rt_snapshot_image keeps the first `bytes` of the image as it is after the calls
 * made so far -- a device-to-device copy in stream order, it does not block --, rt_read_snapshot brings that copy to the
 * host on a stream of its own and blocks until it has arrived, NOT until later frames are rendered:
 *     rt_render(k); rt_snapshot_image(h, n); rt_render(k + 1); rt_read_snapshot(h, out, n);   // frame k, while k + 1 renders
 * costs max(render, read) per frame instead of their sum (config 2: 1.13 + 0.59 ms). */
int rt_snapshot_image(rt_handle* h, size_t bytes);
int rt_read_snapshot(rt_handle* h, float* rgba32f_out, size_t bytes);
/* Restore a previously read accumulation image (checkpoint/resume). */
int rt_write_image(rt_handle* h, const float* rgba32f_in, size_t bytes);

int rt_synchronize(rt_handle* h);
int rt_get_stats(rt_handle* h, rt_stats* out);
/* Shape of the last render launch (what a profile summary needs next to the code object's static resources):
 * out[0] = dynamic LDS bytes per workgroup, out[1] = workgroups of the render kernel, out[2] = 1 when the scene blob
 * was staged into LDS, out[3] = bit 0: many-mesh kernels, bit 1: specialised instantiation, bit 2: one-wave-per-tile
 * variant, bit 3: a deferred-walk sequence ran, bit 4: a wavefront sequence ran (then out[0] / out[1] are the walk kernel's), bit 5: the
 * instantiation with the default launch's fixed switches compiled in ran (csrc/host/launch_options.h: FixedSwitches);
 * out[4] = MiB of device memory the handle holds on its own initiative right now (batch and pipeline scratch images, primary
 * tables, global-memory memos, park queues, snapshot: what option "max_device_mb" bounds), out[5] = that cap (0 = none). */
int rt_last_launch(rt_handle* h, uint32_t out[6]);
/* Zero the counters and forget the recorded launch times. */
int rt_reset_timing(rt_handle* h);
/* Run this handle's work on a caller-owned HIP stream (e.g. the stream a
 * collective library orders its transfers on) so render -> gather -> assemble
 * need no host synchronisation; NULL restores the internal stream. */
int rt_set_stream(rt_handle* h, void* hip_stream);
/* Render into caller-owned device memory of `texels` RGBA32F texels (e.g. a
 * buffer a collective library will send); NULL restores the internal image. */
int rt_bind_image(rt_handle* h, void* device_ptr, uint64_t texels);
/* Tuning knobs.  The image, the ray count and the test counters never depend on any option but "cross_prune" (see its
 * row); every option is swept by the parity tests.  They choose between schedules and data placements.  Unknown names and
 * out-of-range values return RT_ERR_INVALID_ARGUMENT.  "(upload)" = takes effect at the next rt_upload_scene.
 *
 *   name                  values (default)        meaning
 *   --------------------  ----------------------  ---------------------------------------------------------------
 *   kernel_variant        -1 / 0 / 1 (-1)         -1 automatic; 0 persistent waves with active-lane refill; 1 one wave
 *                                                 per 8x8 tile (chosen automatically at <= 1.25 tiles per resident wave)
 *   persistent_blocks     >= 1 (CUs x 5)          grid of variant 0 (256-thread workgroups)
 *   specialise            0 / 1 (1)               1: scenes without spheres, glass and textured materials, rendered by a
 *                                                 camera without jitter, run kernels with those branches compiled out
 *   lds_scene             0 / 1 (1)               0: never stage the scene blob into LDS
 *   pixel_cache           0 / 1 / 2 (1)           per-pixel memo of the primary ray and its hit: off / in LDS when it
 *                                                 fits (else global memory) / always in global memory
 *   primary_table         0 / 1 (1)               0: compute the memoised primary ray per pixel in the render kernel
 *                                                 instead of once per (camera, frame size)
 *   primary_hits          0 / 1 (1)               the primary table also holds every pixel's primary HIT (once per camera, frame
 *                                                 size, strip layout and scene): while the camera stands still no primary ray is
 *                                                 traversed at all; 0: a pixel's first sample of every frame traverses it again
 *   max_device_mb         >= 0 (0)                upper bound (MiB) on the device memory the library takes on its OWN initiative: batch
 *                                                 and pipeline scratch images (64 x 33 MB for a 1080p batch), primary tables (133 MB),
 *                                                 global-memory memos, the park queues of deferred walks (up to half of the free
 *                                                 memory), the snapshot; not the image, the scene and the textures.  What does not
 *                                                 fit runs the plainer path -- smaller batches, no pipeline, no table, no deferred
 *                                                 walks: same image, other frame time; rt_last_launch reports what is held.  0 = no cap
 *   memo_in_table         0 / 1 (1)               kernels whose memo has no room in LDS read it in place from a complete primary
 *                                                 table instead of copying it into a buffer in global memory (round 5: that copy
 *                                                 was 96 % of what those kernels wrote to memory); 0: the copy
 *   vote_eighths          -1 / 0..8 (-1)          intersection vote: traverse when wanting lanes x 8 >= lanes x this
 *   vote_patience         -1 / >= 0 (-1)          ... or when some lane has waited this many iterations; -1: by the kind of
 *                                                 launch (6 and 3 for a scene in LDS on the few-mesh kernels, 7 and 16 for
 *                                                 the others, 8 and 16 inside a deferred-walk sequence)
 *   tile_feedback         0 / 1 (1)               order the tiles by an earlier frame's rays per tile, heaviest first
 *   tile_feedback_period  >= 1 (8)                frames an order is kept before it is refreshed
 *   pipeline              -1 / 0 / 2 .. 8 (-1)    frames in flight: consecutive rt_render calls sample into that many scratch images,
 *                                                 each on an internal stream of its own, and are blended in frame order on the
 *                                                 handle's stream: frame k + 1's launch takes the CUs frame k's draining waves free;
 *                                                 every frame stays observable (config 2: 1.51 / 1.27 / 1.23 / 1.20 ms per frame at
 *                                                 0 / 2 / 3 / 4, config 3 stand-in 7.26 / 6.83 at 3 / 4).  Needs a hardware queue per
 *                                                 stream: -1 (and 1) = four frames when the host has set GPU_MAX_HW_QUEUES >= 5, three
 *                                                 otherwise; seven for a rank of a strip split of 4 ranks and more when there are
 *                                                 12 queues (the library never touches the environment)
 *   pipeline_when_idle    0 / 1 (0)               1 = also pipeline a frame that finds the handle's stream idle; by default such a
 *                                                 frame -- a host that renders, reads, renders: nothing to overlap with -- takes the
 *                                                 plain in-place launch (no scratch image, no blend kernel)
 *   primary_per_slot      0 / 1 (1)               a pipelined frame whose camera is not the shared primary table's builds a table
 *                                                 of its own pipeline slot on its own stream instead of rewriting the shared one
 *                                                 behind a barrier (the frames right after a camera has stopped; while it MOVES --
 *                                                 the camera differs from the previous frame's -- frames render without a table)
 *   frame_ahead           -1 / 0 / 2..64 (-1)     one-frame calls (rt_render, rt_render_strips, rt_render_multi) that continue an
 *                                                 accumulation (same parameters, camera, scene and options, frames = f, f + 1, ...):
 *                                                 the call for frame f renders frames f .. f + d - 1 in one batched launch and blends
 *                                                 frame f; the next d - 1 calls only blend theirs (the image after every call is
 *                                                 bit-identical; a call that does not continue the sequence drops the rest).  -1 =
 *                                                 automatic: ONLY for a host that runs ahead of the device (the call finds the
 *                                                 handle's stream busy) -- a host that renders, waits and renders again never has a
 *                                                 frame held back behind frames it has not asked for (round 5; before, its longest
 *                                                 wait grew from 1.5 to 8 ms) and opts in with an explicit depth --, and then for an
 *                                                 LDS-resident scene and a share too small for a launch of its own to keep the lanes
 *                                                 full (batches of about 4 ms: 28 / 14 / 7 frames for a strip share of 8 / 4 / 2 ranks
 *                                                 of config 2, none for the whole frame), reached by doubling from 2 so that a
 *                                                 sequence of n frames renders at most n in vain; never for a scene read from global
 *                                                 memory (rays of unknown cost: a host asks for batches there itself -- frame_ahead = 8:
 *                                                 config 5's geometry 4.43 -> 3.40 ms per call); 0 = off; 2 .. 64 = that many frames per batch whatever
 *                                                 the host does (the first call of a batch returns its frame after the whole batch).
 *                                                 rt_get_stats: `frames` counts the frames asked for, `frames_speculative` the ones
 *                                                 rendered ahead that no call has asked for (yet); rays and times include both
 *   cross_prune           0 / 1 (0)               many-mesh kernels: boxes and meshes whose entry distance lies beyond a bound derived
 *                                                 from the closest hit so far (error budget + 12.5 % slack) are not
 *                                                 entered; never in the counter / debug kernels.  OFF by default since round 5: exact
 *                                                 on every random ray ever compared (102 G), but a ray that grazes a far triangle at
 *                                                 about 1e-6 rad from an origin within about 1e-4 of that triangle's plane, in a
 *                                                 generic orientation, gets a t from the shader's own arithmetic that the 12.5 % do
 *                                                 not cover (tests/test_gpu_prune_directed.py: 1 texel in 2 M such rays).  1 = take
 *                                                 the 35-45 % shorter many-mesh frames and that risk
 *   batch_frames          1..64 (32)              frames per launch of rt_render_frames
 *   batch_tile_major      0 / 1 (1)               a batch's work items in (tile, frame) order instead of (frame, tile)
 *   forest                0 / 1 (1)  (upload)     BVH meshes of one local space walked per lane back to back
 *   flat2                 0 / 1 (1)  (upload)     meshes whose BVH is a root with two leaves run as straight-line code
 *   stack_wide            -1 / 0 / 1 (-1)         BVH stack entries: automatic / one dword when legal / two dwords
 *   tlas                  0 / 1 (1)  (upload)     top-level trees over the root boxes of many meshes in one local space
 *   tlas_min              >= 2 (8)   (upload)     smallest run of meshes that gets a top-level tree
 *   cull_roots            -1 / 0 / 1 (-1)         results-preserving root-box culling in the mesh loop (-1: from 16 meshes)
 *   sort_rounds           -1 / 0 / 1..64 (-1)     deferred walks (one big mesh among a few): park pixels in front of the
 *                                                 mesh, walk it for all parked rays in a kernel of its own, resume --
 *                                                 for that many rounds; -1: by the work of the launch and the mesh's size,
 *                                                 and only while both park queues fit half of the free memory
 *   defer_min_nodes       >= 1 (1024) (upload)    smallest BVH (internal nodes) whose mesh may be the deferred one
 *   fast_miss             0 / 1 (1)               a memoised primary ray that leaves the scene ends its pixel in one step: the
 *                                                 remaining samples are that segment again and their light is added in order
 *   roulette_skip         0 / 1 (1)               the samples of a pixel that die at the russian roulette of their memoised
 *                                                 primary hit (a plain material: no glass, no texture) are found from the RNG
 *                                                 state alone and not shaded: their light is added in order, the RNG jumps
 *                                                 their 12 draws, their segment is counted as served from the memo; no texel changes
 *   park_levels           0 / 1 (1)               a parking launch runs the deferred walk's first two levels inline and parks
 *                                                 only the rays that reach a grandchild box (0: every ray that can hit the root box)
 *   multi_rccl            0 / 1 / 2 (1)           gather of rt_render_multi: device-to-device copies / RCCL between
 *                                                 distinct devices, copies otherwise (falls back to copies when librccl
 *                                                 cannot be loaded) / RCCL or an error
 *
 * Only in a library built with -DRT_EXPERIMENTS=1 (tools/build_variant.sh exp -DRT_EXPERIMENTS=1; rt_version() then ends in
 * "+experiments") -- features that were built, parity-tested and measured slower than what ships; the product library
 * accepts 0 for them and rejects anything else with RT_ERR_INVALID_ARGUMENT:
 *
 *   lds_top               -1 / 0 / N (0)          wide BVH records of the biggest mesh staged into LDS when the scene is read
 *                                                 from global memory: what fits at full occupancy / none / N (<= 2048)
 *   lds_tlas              0 / 1 / 2 (0)           top-level tree records staged into LDS when the scene is read from global
 *                                                 memory: none / the top levels that fit at full occupancy / the whole tree
 *                                                 (measured slower both ways)
 *   hybrid                0 / 1 (0)               the parking launches of a deferred-walk sequence stage everything but the big
 *                                                 mesh into LDS (measured no faster: DESIGN.md section 5.4)
 *   wavefront             0 / 1 (0)               wavefront sequences (many-mesh scenes): path state in memory slots, a shading
 *                                                 kernel and a ray-walk kernel with per-lane refill alternate (measured slower
 *                                                 than the inline kernels: sponza-sized stand-in 10.65 -> 11.3 ms per frame,
 *                                                 200-mesh stand-in 5.0 -> 7.4)
 */
int rt_set_option(rt_handle* h, const char* name, int value);
/* Enable/disable the optional per-ray counters (node/triangle tests). */
int rt_set_counters(rt_handle* h, int enabled);
/* Raw device pointer of the image / stream, for zero-copy interop
 * (torch.distributed gathers over RCCL operate on this memory). */
void* rt_device_image(rt_handle* h);
void* rt_stream(rt_handle* h);

/* Ray queries against the uploaded scene.  Each ray is intersected exactly as a render's walk
 * does it (calculate_ray_collions, wgsl:353-396): the same instantiation, the same literal stack for BVH heights >= 32,
 * the same tie-break by mesh index.  Queries leave the image, the primary table, a frame_ahead batch in flight, the
 * pipeline slots, rt_get_stats and rt_last_launch as they are, and ignore rt_set_counters. */
typedef struct rt_ray {            /* 32 bytes */
    float origin[3];
    float tmax;                    /* world distance; +INF = unbounded; must be > 0 */
    float dir[3];                  /* any finite non-zero length; normalised by the library with the kernels' normalize3 */
    uint32_t _p0;                  /* must be 0 */
} rt_ray;

typedef struct rt_hit {            /* 64 bytes */
    float t;                       /* world distance (Hit.dst); +INF on a miss */
    uint32_t object;               /* mesh index, or n_meshes + sphere index (the material numbering); 0xffffffff on a miss */
    uint32_t primitive;            /* index into the triangle array given to rt_upload_scene; the sphere index for a sphere;
                                    * 0xffffffff on a miss */
    uint32_t flags;                /* RT_HIT_* */
    float point[3];                /* world hit point */
    float bary_u;                  /* barycentrics (u, v) of the triangle test (wgsl:258-290); w = (1 - u) - v; 0 for spheres */
    float normal[3];               /* the shading normal the render uses */
    float bary_v;
    float tex_u, tex_v;            /* Hit.u / Hit.v: texture coordinates */
    float _p1[2];
} rt_hit;
/* A miss record: t = +INF, object = primitive = 0xffffffff, everything else 0. */

enum { RT_HIT_HIT = 1, RT_HIT_BACKFACE = 2 };
enum { RT_QUERY_HOST_MEMORY = 1, RT_QUERY_PRUNE_TMAX = 2 };

/* Closest hit of n rays.  A hit with t >= tmax is reported as a miss (a filter after the walk: exact).
 * Without RT_QUERY_HOST_MEMORY `rays` and `hits` are device pointers on the handle's device (16-byte aligned) and the
 * call is asynchronous, ordered on the handle's stream after every earlier call on the handle and before every later
 * one.  With it they are host pointers: the rays are staged through temporary device buffers of at most 64 MB per
 * chunk, counted against option "max_device_mb" while held (RT_ERR_OUT_OF_MEMORY when not even one ray fits), and the
 * call returns when the hits are on the host.  A ray with a non-finite component, a direction whose normalisation is
 * not finite and non-zero, tmax <= 0 or NaN, or _p0 != 0 gets a miss record on both paths (never an error).
 * n = 0 is a no-op; n > 2^31 - 1 gives RT_ERR_CAPACITY.  Flags: RT_QUERY_HOST_MEMORY only. */
int rt_intersect_rays(rt_handle* h, const rt_ray* rays, uint64_t n, rt_hit* hits, int flags);
/* Occlusion: occluded[i] = 1 when the scene holds a hit closer than tmax, else 0 (invalid rays: 0).  The same walk in the
 * same order that stops at the first candidate whose world distance is < tmax, so occluded == (closest hit && t < tmax)
 * except for rays with some hit within a few ulps of tmax.  RT_QUERY_PRUNE_TMAX also skips boxes entered beyond a
 * local-space bound for tmax: the fast path for short shadow rays, but not exact -- it
 * rests on the same hypothesis as option "cross_prune".  Memory, ordering and limits as rt_intersect_rays
 * (occluded: 4-byte aligned). */
int rt_occluded_rays(rt_handle* h, const rt_ray* rays, uint64_t n, uint32_t* occluded, int flags);
/* The closest hit of the ray the debug views trace for texel (x, y) of a params->width x params->height frame (row 0 is
 * the bottom, no jitter, the camera currently set).  Synchronous; hit is host memory.  x or y out of range:
 * RT_ERR_INVALID_ARGUMENT; no scene: RT_ERR_NO_SCENE. */
int rt_pick(rt_handle* h, const rt_params* params, uint32_t x, uint32_t y, rt_hit* hit);

/* First-hit buffers of a whole frame (the G-buffer a denoiser is guided by, an id mask, depth and normal maps; DESIGN.md
 * section 2.10): for every texel of a params->width x params->height frame and the camera currently set, the closest hit
 * of the ray the debug views and rt_pick trace for it (wgsl:502-515: no jitter), in ONE launch, into planes the caller
 * owns.  Planes are row-major, tightly packed, row 0 = bottom of the view (as the image).  A NULL plane is not produced
 * and costs nothing.  For every channel rt_hit also has, a texel holds the bits rt_pick(h, params, x, y, &hit) returns
 * for it; a miss (and a texel whose ray rt_intersect_rays would call invalid, e.g. width == 1: x / (width - 1)) gets
 * +INF, 0xffffffff and zeros -- `dir` is written all the same.
 * Only width and height of `params` matter; the frame need not fit the handle's max_width x max_height (the image is
 * not touched); width * height <= 2^31 - 1 (else RT_ERR_CAPACITY).
 * Memory and ordering as rt_intersect_rays.  Without RT_GBUFFER_HOST_MEMORY the planes are device pointers on the
 * handle's device (4-byte aligned; 16 for albedo / emission; 1 for flags) and the call is asynchronous on the handle's
 * stream, after every earlier call on the handle and before every later one.  With it they are host pointers: the frame
 * is produced in bands of whole rows through temporary device buffers of at most 64 MB, counted against option
 * "max_device_mb" while held (RT_ERR_OUT_OF_MEMORY when not even one row fits), and the call returns when the data is
 * on the host.
 * Errors, nothing written: RT_ERR_INVALID_ARGUMENT (null handle / params / out, struct_bytes != sizeof(rt_gbuffer),
 * _p0 != 0, unknown flags, zero width or height, misaligned device planes), RT_ERR_CAPACITY, RT_ERR_NO_SCENE.  All
 * planes NULL: a no-op.
 * Like the ray queries the call leaves the image, the primary tables, a frame_ahead batch in flight, the pipeline slots,
 * rt_get_stats and rt_last_launch as they are, and ignores rt_set_counters. */
typedef struct rt_gbuffer {
    uint32_t  struct_bytes; /* = sizeof(rt_gbuffer): channels can be appended without writing past an older caller's struct */
    uint32_t  _p0;          /* must be 0 */
    float*    depth;        /* [h][w]     rt_hit.t: Hit.dst, world distance; +INF on a miss                        */
    float*    dir;          /* [h][w][3]  the normalised ray direction (the origin is cam_to_world[3])             */
    float*    point;        /* [h][w][3]  rt_hit.point                                                             */
    float*    normal;       /* [h][w][3]  rt_hit.normal (the shading normal the render uses)                       */
    float*    bary;         /* [h][w][2]  rt_hit.bary_u, bary_v                                                    */
    float*    texcoord;     /* [h][w][2]  rt_hit.tex_u, tex_v                                                      */
    float*    albedo;       /* [h][w][4]  `color` of wgsl:453-458: the diffuse texture's sample at Hit.uv when flag ==
                             *            RT_MATERIAL_TEXTURE and diffuse_index != -1, else material.color (glass too);
                             *            zeros on a miss                                                          */
    float*    emission;     /* [h][w][4]  emission_color * emission_strength (wgsl:450), one multiply per component;
                             *            zeros on a miss                                                          */
    uint32_t* object;       /* [h][w]     rt_hit.object; 0xffffffff on a miss                                      */
    uint32_t* primitive;    /* [h][w]     rt_hit.primitive; 0xffffffff on a miss                                   */
    uint8_t*  flags;        /* [h][w]     RT_HIT_HIT | RT_HIT_BACKFACE                                             */
} rt_gbuffer;
enum { RT_GBUFFER_HOST_MEMORY = 1 };
int rt_render_gbuffer(rt_handle* h, const rt_params* params, const rt_gbuffer* out, int flags);

/* Radiance along rays the caller supplies: the path tracer (`trace`, wgsl:398-471) for rays that
 * need not come from the library's pinhole camera -- light probes, lightmap texels, panoramic / fisheye / orthographic /
 * cube-map cameras, re-sampling chosen pixels.  For ray i the call runs `frag`'s sample loop (wgsl:486-498) with the ray
 * held fixed, bit for bit:
 *     state = seed;
 *     for each of params->rays_per_pixel samples: four draws of the generator (the ones `frag` spends on the camera
 *         jitter, wgsl:488-492), then total += trace(ray, &state) -- `trace` normalises dir (wgsl:400);
 *     out[i] = total / f32(rays_per_pixel), all four components.
 * So a ray with origin = cam_to_world[3], dir = texel (x, y) of rt_render_gbuffer's `dir` plane and
 * seed = y * width + x + |frames| * 719393 (u32 arithmetic) gets the bits rt_render writes to that texel for
 * frames <= 0 under a camera without jitter (both strengths +0, no component of the camera origin or of the texel's
 * focus point being -0).
 * Of `params` only number_of_bounces (>= 0), rays_per_pixel (>= 1) and skybox matter (other values of the first two:
 * RT_ERR_INVALID_ARGUMENT); width, height, frames, accumulate and the debug fields are ignored.  The handle's camera,
 * image, primary tables and options do not enter the result (the options that choose the scene's instantiation and
 * placement at upload apply and, as for a render, never change a bit).
 * A ray with a non-finite component, a direction whose normalisation is not finite and non-zero, or _p0 != 0 gets
 * (0, 0, 0, 0) (never an error).
 * Memory, ordering and limits as rt_intersect_rays: without RT_RADIANCE_HOST_MEMORY `rays` and `rgba32f_out` are device
 * pointers on the handle's device (16-byte aligned) and the call is asynchronous on the handle's stream, after every
 * earlier call on the handle and before every later one; with it they are host pointers, staged through a temporary
 * device buffer of at most 64 MB per chunk (48 bytes per ray), counted against option "max_device_mb" while held
 * (RT_ERR_OUT_OF_MEMORY when not even one ray fits), and the call returns when the results are on the host.
 * n = 0 is a no-op; n > 2^31 - 1 gives RT_ERR_CAPACITY; no scene: RT_ERR_NO_SCENE; null handle / params / rays / out,
 * unknown flags or misaligned device pointers: RT_ERR_INVALID_ARGUMENT.  On any error nothing is written.
 * Like the ray queries the call leaves the image, the primary tables, a frame_ahead batch in flight, the pipeline slots,
 * rt_get_stats and rt_last_launch as they are, and ignores rt_set_counters. */
typedef struct rt_path_ray {       /* 32 bytes, two 16-byte loads */
    float origin[3];
    uint32_t seed;                 /* the ray's RNG state before its first sample (wgsl:475 for a pixel) */
    float dir[3];                  /* any finite non-zero length */
    uint32_t _p0;                  /* must be 0 */
} rt_path_ray;
enum { RT_RADIANCE_HOST_MEMORY = 1 };
int rt_radiance_rays(rt_handle* h, const rt_params* params, const rt_path_ray* rays, uint64_t n,
                     float* rgba32f_out /* [n][4] */, int flags);

/* G-buffer-guided denoising of a rendered frame: the edge-avoiding a-trous filter of Dammertz et
 * al. 2010 with its three edge terms in one exponent, guided by the planes rt_render_gbuffer writes.  The frame is
 * width x height, row 0 = bottom, every plane tightly packed as the G-buffer's.  In binary32, unfused, in this order:
 *   k_c = 1 / (sigma_color * sigma_color) (+INF gives 0), k_n and k_x likewise from sigma_normal and sigma_point;
 *   pass i of `iterations` has step s = 2^i and k_c,i = k_c * 4^i (sigma_color halves per pass).
 *   Texel p is FILTERABLE when some component of normal(p) is non-zero, every component of normal(p), point(p) and
 *   color(p).rgb is finite, and emission is NULL or emission(p).rgb are all zero.  Every other texel (a miss, a lamp, a
 *   non-finite sample) copies color(p) to out(p) bit for bit and is never a tap.
 *   a'(p) = albedo(p) > 2^-10 ? albedo(p) : 2^-10 per component (1 with a NULL albedo);  c_0(p) = color(p).rgb / a'(p).
 *   Pass i, for filterable p: over dy = -2..2 (outer), dx = -2..2 (inner), q = p + s (dx, dy) inside the frame and
 *   filterable, with d2(a) = ((a0 a0 + a1 a1) + a2 a2) of the componentwise difference of the values at p and q:
 *       e = (d2(c_i) k_c,i + d2(normal) k_n) + d2(point) k_x,   w = (h[dx] h[dy]) exp_(-e),  h = {1/16, 1/4, 3/8, 1/4, 1/16}
 *       (exp_: csrc/rt_transc.h); a tap with w > 0 adds w c_i(q) to sum and w to wsum;   c_{i+1}(p) = sum / wsum.
 *   out(p).rgb = c_n(p) a'(p), out(p).a = color(p).a.
 *   The centre tap has e = 0 and adds 9/64, so wsum > 0 -- unless a finite colour overflows in the division by a' (3e38 /
 *   0.5): then c_0(p) is infinite, the centre difference is inf - inf = NaN, every tap of p is skipped and out(p).rgb is
 *   the NaN of 0 / 0.  Such a texel is still filterable by the rule above; a host that may hold colours near FLT_MAX over
 *   albedos below 1 clamps them first.
 * sigma_color is in units of demodulated radiance (colour divided by albedo), sigma_point in world units, sigma_normal in
 * units of the difference of two unit normals (0 .. 2).
 * rt_denoise_host (section 3) is this definition over host pointers, without a device; rt_denoise computes the same bits
 * on the device.  Without RT_DENOISE_HOST_MEMORY the planes are device pointers on the handle's device (4-byte aligned;
 * 16 for color, albedo, emission and out), `color` may be NULL for the handle's current image (rt_device_image or a
 * bound image; width * height texels of it), `out` may be `color` or that image, and the call is asynchronous on the
 * handle's stream, after every earlier call on the handle and before every later one.  With it they are host pointers,
 * staged WHOLE through one temporary device buffer -- 40 to 72 bytes per texel, 149 MB for 1920 x 1080 with every plane:
 * the one host-memory call that does not keep to chunks of 64 MB, because a pass reads up to 256 rows away and the frame
 * cannot be cut into bands -- counted against option "max_device_mb" while held, and the call returns when `out` is on
 * the host.  `out` may be the same pointer as `color`; any other overlap is undefined.
 * The handle keeps 64 bytes of scratch per texel (a packed guide record and two colour images), allocated on first use,
 * grown on demand, counted by rt_last_launch out[4] and bounded by option "max_device_mb" (RT_ERR_OUT_OF_MEMORY).
 * Errors, nothing written: RT_ERR_INVALID_ARGUMENT (null handle / desc / normal / point / out, null color on the host or
 * with the flag, struct_bytes != sizeof(rt_denoise_desc), _p0 != 0, unknown flags, zero width or height, iterations
 * outside 1 .. 8, a sigma that is NaN or <= 0, an infinite sigma_normal or sigma_point, misaligned device planes),
 * RT_ERR_CAPACITY (width * height > 2^31 - 1, or more texels than the image has with a NULL color),
 * RT_ERR_OUT_OF_MEMORY.  No scene is needed.
 * Like the ray queries the call leaves the image (unless `out` is the image), the primary tables, a frame_ahead batch
 * in flight, the pipeline slots, rt_get_stats and the launch words of rt_last_launch as they are. */
typedef struct rt_denoise_desc {
    uint32_t     struct_bytes;  /* = sizeof(rt_denoise_desc) */
    uint32_t     _p0;           /* must be 0 */
    uint32_t     width, height;
    uint32_t     iterations;    /* n: 1 .. 8 passes, steps 1, 2, .. 2^(n-1) */
    float        sigma_color;   /* > 0, may be +INF (no colour term) */
    float        sigma_normal;  /* > 0, finite */
    float        sigma_point;   /* > 0, finite */
    const float* color;         /* [h][w][4] */
    const float* normal;        /* [h][w][3] */
    const float* point;         /* [h][w][3] */
    const float* albedo;        /* [h][w][4] or NULL */
    const float* emission;      /* [h][w][4] or NULL */
    float*       out;           /* [h][w][4] */
} rt_denoise_desc;
enum { RT_DENOISE_HOST_MEMORY = 1 };
int rt_denoise(rt_handle* h, const rt_denoise_desc* desc, int flags);

/* Temporal accumulation across a camera move: the shader's per-texel accumulation (wgsl:154-161)
 * with the history fetched from where each texel's hit point lay in the PREVIOUS frame.  Inputs: the current frame's
 * colour and G-buffer planes (point, normal, optionally object: rt_render_gbuffer's), the previous frame's accumulated
 * colour, a per-texel history length and its G-buffer planes, and the camera those were produced under.  Frames are
 * width x height, row 0 = bottom, every plane tightly packed.  The scene itself is taken not to have moved.
 * Everything is binary32 and unfused, in this order.
 *   Once per call, on the host: V = mat4_inverse(prev_camera.cam_to_world) (glam's scalar cofactor inverse, csrc/host/
 *   glam_math.h); pw, ph, fd = prev_camera.view_params.
 *   Texel p = (x, y) is REPROJECTABLE when some component of normal(p) is non-zero, every component of normal(p) and
 *   point(p) is finite, and object is NULL or object(p) != 0xffffffff.  A texel that is not (a miss, a NaN) gets
 *   out(p) = color(p) bit for bit, out_history(p) = 1 and motion(p) = two quiet NaNs (0x7fc00000).
 *   Projection, with X = point(p):  l_k = ((V[0][k] X0 + V[1][k] X1) + V[2][k] X2) + V[3][k] for k = 0, 1, 2 (column-major,
 *   [col][row]);  ux = ((l0 / l2) * fd) / pw + 0.5;  uy = ((l1 / l2) * fd) / ph + 0.5;  fx = ux * (f32(W) - 1);
 *   fy = uy * (f32(H) - 1) -- the inverse of the texel's focus point (wgsl:479-482).
 *   ON SCREEN: l2 > 0, -1 < fx < W and -1 < fy < H (all false for NaN).  A texel that is not on screen takes the "no
 *   history" result below, with motion = the two NaNs.
 *   Snap, per axis: x0 = floor(fx) as an integer, tx = fx - f32(x0); with S = 1/64: if tx <= S then tx = 0, otherwise if
 *   tx >= 1 - S then x0 += 1 and tx = 0.  A position within 1/64 texel of a texel centre takes that texel alone: a camera
 *   that has not moved resamples nothing.   motion(p) = ((f32(x0) + tx) - f32(x), (f32(y0) + ty) - f32(y)).
 *   Taps, in the order (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1), with weights b = (1-tx)(1-ty), tx(1-ty), (1-tx)ty,
 *   tx ty.  Tap q is VALID when b > 0; q is inside the frame; some component of prev_normal(q) is non-zero; prev_normal(q),
 *   prev_point(q), all four components of prev_color(q) and prev_history(q) are finite; prev_history(q) >= 1; when both
 *   object planes are given, prev_object(q) == object(p); with a = prev_point(q) - X and n = normal(p),
 *   |(a0 n0 + a1 n1) + a2 n2| <= point_tolerance * l2; and with m = prev_normal(q), ((n0 m0 + n1 m1) + n2 m2) >= normal_cos.
 *   A valid tap adds b * prev_color(q) (four components) to sum, b * prev_history(q) to hsum and b to wsum, in tap order,
 *   all three from +0.
 *   Blend.  If wsum > 0: prev = sum / wsum; n = hsum / wsum; n_c = n < max_history ? n : max_history; w = 1 / (n_c + 1);
 *   out(p) = prev * (1 - w) + color(p) * w on all four components (two products, then the sum: wgsl:156-157);
 *   out_history(p) = n_c + 1 -- but if some component of color(p) is not finite the sample is dropped: out(p) = prev and
 *   out_history(p) = n_c.  If wsum is not > 0 there is no history: out(p) = color(p) bit for bit, out_history(p) = 1.
 * Consequence: under an unmoved camera, with the same G-buffer on both sides, prev_history == k everywhere and `color` the
 * raw sample of seed k (rt_render with frames = -k), every reprojectable texel takes one tap of weight 1 and `out` is what
 * rt_render with frames = k leaves in the image, bit for bit, alpha included.
 * Rigidly or affinely moved meshes and moved or resized spheres keep their history through rt_temporal_accumulate_moving
 * (below), and a mesh whose vertices moved (rt_refit_triangles) keeps it through rt_temporal_accumulate_deforming (below
 * that).  Still out of scope: a mesh whose topology changed and the sky -- their texels fail the plane test or are misses,
 * and restart at history 1.
 * point_tolerance is the distance from the current texel's tangent plane that a tap's hit point may have, per unit of view
 * depth (the footprint of a texel grows with depth); normal_cos the least cosine between the two normals.
 * rt_temporal_accumulate_host (section 3) is this definition over host pointers, without a device;
 * rt_temporal_accumulate computes the same bits on the device.  Without RT_TEMPORAL_HOST_MEMORY the planes are device
 * pointers on the handle's device (4-byte aligned; 16 for color, prev_color and out; 8 for motion), `color` may be NULL
 * for the handle's current image (width * height texels of it), `out` may be `color` or that image, and the call is
 * asynchronous on the handle's stream, after every earlier call on the handle and before every later one.  With the flag
 * they are host pointers, staged WHOLE through one temporary device buffer (a gather can reach any row: no bands; 88 to
 * 104 bytes per texel, `out` in the colour's place) that is counted against option "max_device_mb" while held (RT_ERR_OUT_OF_MEMORY past the cap), and
 * the call returns when the outputs are on the host.
 * `out` may be the same pointer as `color`.  out, out_history and motion must not overlap any prev_* plane, nor each
 * other, nor any other input: undefined.  The call keeps no scratch between calls.
 * Errors, nothing written: RT_ERR_INVALID_ARGUMENT (null handle or desc; a null plane other than object, prev_object,
 * motion, and color on the device path; struct_bytes != sizeof(rt_temporal_desc); _p0 != 0; unknown flags; zero width or
 * height; max_history NaN or below 1; point_tolerance NaN, <= 0 or infinite; normal_cos NaN or outside [-1, 1];
 * misaligned device planes), RT_ERR_CAPACITY (width * height > 2^31 - 1, or more texels than the image has with a NULL
 * color), RT_ERR_OUT_OF_MEMORY.  No scene is needed.
 * Like the ray queries the call leaves the image (unless `out` is the image), the primary tables, a frame_ahead batch in
 * flight, the pipeline slots, rt_get_stats and the launch words of rt_last_launch as they are. */
typedef struct rt_temporal_desc {
    uint32_t          struct_bytes;     /* = sizeof(rt_temporal_desc) */
    uint32_t          _p0;              /* must be 0 */
    uint32_t          width, height;
    rt_camera_uniform prev_camera;      /* the camera the prev_* planes were produced under */
    float             max_history;      /* >= 1, may be +INF: cap of the history length */
    float             point_tolerance;  /* > 0, finite: plane distance allowed per unit of view depth */
    float             normal_cos;       /* finite, in [-1, 1]: least dot product of the two normals */
    const float*      color;            /* [h][w][4] current frame; device path: NULL = the handle's image */
    const float*      point;            /* [h][w][3] current */
    const float*      normal;           /* [h][w][3] current */
    const uint32_t*   object;           /* [h][w] current, or NULL */
    const float*      prev_color;       /* [h][w][4] accumulated history */
    const float*      prev_history;     /* [h][w]    frames accumulated in prev_color, as a float >= 1 */
    const float*      prev_point;       /* [h][w][3] */
    const float*      prev_normal;      /* [h][w][3] */
    const uint32_t*   prev_object;      /* [h][w] or NULL */
    float*            out;              /* [h][w][4]; may be `color` */
    float*            out_history;      /* [h][w] */
    float*            motion;           /* [h][w][2] or NULL */
} rt_temporal_desc;
enum { RT_TEMPORAL_HOST_MEMORY = 1 };
int rt_temporal_accumulate(rt_handle* h, const rt_temporal_desc* desc, int flags);

/* Temporal accumulation across moving objects: rt_temporal_accumulate with a table that says, per
 * object word of the G-buffer (a mesh's index, or n_meshes + a sphere's index), how a point of the object in the CURRENT
 * frame's world is carried to where the same surface point lay in the PREVIOUS frame's world.  rt_object_motions (section 3)
 * fills the table from two scene states.  Everything is binary32 and unfused, in this order; what is not restated here is
 * rt_temporal_accumulate's definition above, word for word.
 *   `object` is required.  For a REPROJECTABLE texel p (so object(p) != 0xffffffff) with k = object(p):
 *   k >= n_objects: the "no history" result -- out(p) = color(p) bit for bit, out_history(p) = 1, motion(p) = two quiet NaNs.
 *   motions[k].moved == 0: the record's matrices are not read and the texel is worked exactly as by
 *   rt_temporal_accumulate, with X = point(p) and n = normal(p) as they are.
 *   Otherwise, with d = motions[k].d, nt = motions[k].nt, X = point(p), n = normal(p), for r = 0, 1, 2:
 *     X'_r = ((d[0][r] X0 + d[1][r] X1) + d[2][r] X2) + d[3][r]
 *     m_r  = (nt[0][r] n0 + nt[1][r] n1) + nt[2][r] n2
 *     len  = sqrt((m0 m0 + m1 m1) + m2 m2)    (the correctly rounded square root)
 *     n'_r = m_r / len                        (three divisions)
 *   If some component of X' or n' is not finite (a zero len gives NaN or infinity): the "no history" result.  Otherwise the
 *   texel is worked as by rt_temporal_accumulate with X' in the place of X and n' in the place of n throughout: the
 *   projection and the on-screen test, the snap, motion(p), each tap's plane distance |(prev_point(q) - X') . n'| <=
 *   point_tolerance * l2 and normal cosine n' . prev_normal(q), the object match (when prev_object is given) and the blend.
 *   motion(p) is then the screen offset that the camera's and the object's move produce together.
 * Consequence: with a table whose records all have moved == 0 (and every object word below n_objects) every output plane
 * is rt_temporal_accumulate's bit for bit, for any camera move.
 * What this keeps is an object's OWN history, not the lighting: a turning object's faces change their illumination, shadows
 * and reflections move over surfaces that stand still, and the history lags behind them; max_history bounds the lag
 * everywhere at the price of noise everywhere, and rt_temporal_rectify (below) cuts it where the new frame contradicts the
 * history.
 * A second call with the luminance moments as color / prev_color and the same table accumulates the moments that
 * rt_denoise_variance takes for a moving object.
 * Memory, asynchrony, aliasing and side effects are rt_temporal_accumulate's.  `motions` is on the side of the planes: a
 * device pointer (16-byte aligned) without RT_TEMPORAL_HOST_MEMORY; with it a host pointer whose n_objects * 96 bytes are
 * staged with the planes and counted against option "max_device_mb" with them.
 * Errors, nothing written: rt_temporal_accumulate's (struct_bytes != sizeof(rt_temporal_motion_desc)), and
 * RT_ERR_INVALID_ARGUMENT for a null motions, n_objects == 0, _p1 != 0, a null object plane, a misaligned device table. */
typedef struct rt_object_motion {
    float    d[4][3];    /* current world -> previous world, column-major [col][row]: X' = d * (X, 1) */
    float    nt[3][3];   /* [col][row]: m = nt * n is the previous-world normal before normalisation */
    uint32_t moved;      /* 0: the object stands still, the record's matrices are not read; 2: DEFORMED for
                            rt_temporal_accumulate_deforming (any non-zero value is "moved" to rt_temporal_accumulate_moving) */
    uint32_t _p[2];      /* 0 */
} rt_object_motion;      /* 96 bytes */
typedef struct rt_temporal_motion_desc {
    uint32_t          struct_bytes;     /* = sizeof(rt_temporal_motion_desc) */
    uint32_t          _p0;              /* must be 0 */
    uint32_t          width, height;
    rt_camera_uniform prev_camera;
    float             max_history;
    float             point_tolerance;
    float             normal_cos;
    const float*      color;
    const float*      point;
    const float*      normal;
    const uint32_t*   object;           /* [h][w] current: required */
    const float*      prev_color;
    const float*      prev_history;
    const float*      prev_point;
    const float*      prev_normal;
    const uint32_t*   prev_object;      /* [h][w] or NULL */
    float*            out;
    float*            out_history;
    float*            motion;           /* [h][w][2] or NULL */
    const rt_object_motion* motions;    /* [n_objects], indexed by the object word */
    uint32_t          n_objects;        /* >= 1 */
    uint32_t          _p1;              /* must be 0 */
} rt_temporal_motion_desc;              /* rt_temporal_desc's fields in their order, then the table */
int rt_temporal_accumulate_moving(rt_handle* h, const rt_temporal_motion_desc* desc, int flags);

/* Temporal accumulation across deforming meshes: rt_temporal_accumulate_moving with a third kind
 * of record.  A mesh whose vertices moved (rt_refit_triangles) has no one map from the current world to the previous one,
 * but the G-buffer says which triangle of the uploaded array each texel hit and where (primitive, bary, flags:
 * rt_render_gbuffer's), and the caller still holds the triangles that rt_refit_triangles replaced: the previous-world
 * position of a texel's surface point is the barycentric interpolation of the PREVIOUS triangle's vertices under the
 * previous model_to_world.  rt_object_motions_deforming (section 3) fills the table.  Everything is binary32 and unfused,
 * in this order; what is not restated here is rt_temporal_accumulate_moving's definition above, word for word.
 *   motions[k].moved is read three ways: 0 -- the object stands still; 2 -- DEFORMED, below; any other value -- carried
 *   rigidly, exactly as by rt_temporal_accumulate_moving.  (The two calls above take every non-zero value as moved.)
 *   For a REPROJECTABLE texel p with k = object(p) < n_objects and motions[k].moved == 2, with t = primitive(p) and
 *   (u, v) = bary(p):
 *   t < tri_first, or t - tri_first >= n_prev_triangles, or u or v not finite: the "no history" result -- out(p) =
 *   color(p) bit for bit, out_history(p) = 1, motion(p) = two quiet NaNs.  prev_triangles is read only after this test.
 *   Otherwise, with T = prev_triangles[t - tri_first], d = motions[k].d, nt = motions[k].nt and w = (1 - u) - v, for
 *   r = 0, 1, 2:
 *     Xm_r = (T.v1_r * w + T.v2_r * u) + T.v3_r * v      (the order of the render kernel's normal interpolation)
 *     X'_r = ((d[0][r] Xm0 + d[1][r] Xm1) + d[2][r] Xm2) + d[3][r]
 *     g_r  = (T.n1_r * w + T.n2_r * u) + T.n3_r * v
 *     m_r  = (nt[0][r] g0 + nt[1][r] g1) + nt[2][r] g2
 *     len  = sqrt((m0 m0 + m1 m1) + m2 m2)               (the correctly rounded square root)
 *     s    = (flags(p) & RT_HIT_BACKFACE) ? -1 : 1
 *     n'_r = (m_r / len) * s
 *   One normalisation, where the shader has two (of g, then of the transformed normal: wgsl:386): n' only feeds the
 *   normal cosine and the plane distance, whose thresholds are far wider than the few ulp between the two.  The render
 *   kernel's RT_HIT_BACKFACE on a triangle is exactly the factor -1 on its interpolated normal, hence s.
 *   If some component of X' or n' is not finite (a degenerate previous triangle whose normals interpolate to zero length
 *   gives NaN): the "no history" result.  Otherwise the texel is worked as by rt_temporal_accumulate with X' in the place
 *   of X and n' in the place of n throughout: the projection and the on-screen test, the snap, motion(p), each tap's plane
 *   distance and normal cosine, the object match and the blend.
 *   A mesh that deforms and also moves rigidly needs nothing more: d is its previous model_to_world.
 * Consequences: (a) with a table that has no record of moved == 2 every output plane is rt_temporal_accumulate_moving's bit
 * for bit, whatever primitive, bary, flags and prev_triangles hold.  (b) With prev_triangles = the current triangles, an
 * unmoved camera and the same G-buffer on both sides every deformed texel's X' lies within a few ulp of point(p), far
 * inside the 1/64-texel snap; it takes its own texel as its one tap, motion(p) = (0, 0), and every output plane is
 * rt_temporal_accumulate's bit for bit -- and so rt_render's own accumulation.
 * What still lags or restarts: the lighting around a deforming object lags as it does around a moving one (max_history
 * bounds it, rt_temporal_rectify cuts it where the new frame contradicts the history); a change of topology restarts (the primitive word then names another triangle or none); the sky restarts;
 * a sphere given moved == 2 by a hand-made table restarts or fetches a wrong triangle's history -- its primitive word is
 * read as a triangle index -- which rt_object_motions_deforming never produces.
 * A second call with the luminance moments as color / prev_color and the same arguments accumulates the moments that
 * rt_denoise_variance takes for a deforming object.
 * Memory, asynchrony, aliasing and side effects are rt_temporal_accumulate_moving's.  primitive, bary, flags and
 * prev_triangles are on the side of the planes: device pointers without RT_TEMPORAL_HOST_MEMORY (primitive and bary 4-byte
 * aligned, flags 1, prev_triangles 16); with it host pointers, the three planes and the n_prev_triangles * 96 bytes staged
 * with the rest and counted against option "max_device_mb" with them.  The call never reads the uploaded scene: no scene
 * is needed.
 * Errors, nothing written: rt_temporal_accumulate_moving's (struct_bytes != sizeof(rt_temporal_deform_desc)), and
 * RT_ERR_INVALID_ARGUMENT for a null primitive, bary, flags or prev_triangles, n_prev_triangles == 0, tri_first +
 * n_prev_triangles past 2^32, a misaligned device plane or triangle array. */
typedef struct rt_temporal_deform_desc {
    uint32_t          struct_bytes;     /* = sizeof(rt_temporal_deform_desc) */
    uint32_t          _p0;              /* must be 0 */
    uint32_t          width, height;
    rt_camera_uniform prev_camera;
    float             max_history;
    float             point_tolerance;
    float             normal_cos;
    const float*      color;
    const float*      point;
    const float*      normal;
    const uint32_t*   object;           /* [h][w] current: required */
    const float*      prev_color;
    const float*      prev_history;
    const float*      prev_point;
    const float*      prev_normal;
    const uint32_t*   prev_object;      /* [h][w] or NULL */
    float*            out;
    float*            out_history;
    float*            motion;           /* [h][w][2] or NULL */
    const rt_object_motion* motions;    /* [n_objects], indexed by the object word */
    uint32_t          n_objects;        /* >= 1 */
    uint32_t          _p1;              /* must be 0 */
    const uint32_t*   primitive;        /* [h][w]    current G-buffer: required */
    const float*      bary;             /* [h][w][2] current G-buffer: required */
    const uint8_t*    flags;            /* [h][w]    current G-buffer: required */
    const rt_packed_triangle* prev_triangles;   /* [n_prev_triangles]: triangles [tri_first, tri_first + n) of the uploaded
                                                   array as they were in the PREVIOUS frame */
    uint32_t          tri_first, n_prev_triangles;   /* n >= 1 */
} rt_temporal_deform_desc;              /* rt_temporal_motion_desc's fields in their order, then the triangle side */
int rt_temporal_accumulate_deforming(rt_handle* h, const rt_temporal_deform_desc* desc, int flags);

/* Variance-guided denoising: the variance half of SVGF (Schied et al. 2017, sections 4.2 - 4.4)
 * over rt_denoise's guides.  rt_luminance_moments writes the per-frame sample of the luminance moments;
 * rt_denoise_variance estimates each texel's variance -- from moments accumulated over a history (a second
 * rt_temporal_accumulate call whose color / prev_color are the moments planes), or from a 7 x 7 window where the history is
 * short -- and runs an a-trous filter whose luminance edge-stopping is measured in units of the local standard deviation,
 * filtering the variance along with the colour so that later passes narrow as the earlier ones remove noise.  The frame is
 * width x height, row 0 = bottom, every plane tightly packed.  In binary32, unfused, in this order:
 *   FILTERABLE, a'(p), c_0(p) = color(p).rgb / a'(p), d2, h, k_n and k_x: exactly rt_denoise's (above).  A texel that is not
 *   filterable copies color(p) to out(p) bit for bit, gets out_variance(p) = 0, and is never a tap of anything below.
 *   l(c) = (0.2126f c0 + 0.7152f c1) + 0.0722f c2.
 *   rt_luminance_moments: with l = l(c_0(p)), out(p) = (l, l l, 0, 0) for a filterable texel and (0, 0, 0, 0) otherwise
 *   (iterations, the sigmas, min_history, moments, history and out_variance are not examined).
 *   VARIANCE OF THE INPUT, var_0(p), for filterable p.
 *     Temporal, when `moments` is given, history(p) is finite and >= min_history, and m1 = moments(p).x and
 *     m2 = moments(p).y are finite:  v = (m2 - m1 m1) / history(p)  (the history is a true mean: the variance of the mean
 *     falls with its length).
 *     Spatial, otherwise: over dy = -3..3 (outer), dx = -3..3 (inner), q = p + (dx, dy) inside the frame and filterable,
 *     u = exp_(-(d2(normal) k_n + d2(point) k_x)); a tap with u > 0 adds u l_q to s1, u (l_q l_q) to s2 and u to sw, all
 *     from +0, with l_q = l(c_0(q));  m1 = s1 / sw, m2 = s2 / sw, v = m2 - m1 m1.
 *     In both: var_0(p) = v > 0 ? v : 0 (a NaN gives 0).
 *   PASS i, step s = 2^i, for filterable p.
 *     Prefilter: over dy = -1..1 (outer), dx = -1..1 (inner), q = p + (dx, dy) inside the frame and filterable, with
 *     g = {1/4, 1/2, 1/4}: gs += (g[dx] g[dy]) var_i(q), gw += g[dx] g[dy], from +0;  G = gs / gw;
 *     D = sigma_luminance sqrt_(G) + 2^-30.
 *     Taps: rt_denoise's 25, in its order, q = p + s (dx, dy) inside the frame and filterable, l_p = l(c_i(p)), l_q = l(c_i(q)):
 *       e = (abs_(l_p - l_q) / D + d2(normal) k_n) + d2(point) k_x,   w = (h[dx] h[dy]) exp_(-e);
 *       a tap with w > 0 adds w c_i(q) to sum, (w w) var_i(q) to vsum and w to wsum, from +0;
 *       c_{i+1}(p) = sum / wsum,  var_{i+1}(p) = vsum / (wsum wsum).
 *     sigma_luminance is the same in every pass; the variance is what changes.
 *   out(p).rgb = c_n(p) a'(p), out(p).a = color(p).a, out_variance(p) = var_n(p).
 * Consequence: where var_0 is 0 over a texel's neighbourhood, D = 2^-30 and every tap whose luminance differs is refused:
 * out equals color up to the roundings of / a' * a' and (w c) / w.
 * Memory, ordering, alignment (16 bytes for color, albedo, emission, moments and out, 4 otherwise), a NULL `color` for the
 * handle's image, `out` being `color` or the image, the whole-frame staging of the host-memory path (44 to 100 bytes per
 * texel, counted against option "max_device_mb") and the side effects are rt_denoise's.  The scratch is rt_denoise's own 64
 * bytes per texel, shared: the variance rides in the fourth component of the colour images, and calls of the two may be
 * interleaved on one handle.
 * Errors, nothing written: rt_denoise's (with sigma_luminance, which must be finite, in sigma_color's place), `moments`
 * without `history` or the reverse, a min_history that is NaN, infinite or below 1, _p1 != 0. */
typedef struct rt_vdenoise_desc {
    uint32_t     struct_bytes;    /* = sizeof(rt_vdenoise_desc) */
    uint32_t     _p0;             /* must be 0 */
    uint32_t     width, height;
    uint32_t     iterations;      /* 1 .. 8; ignored by rt_luminance_moments */
    float        sigma_luminance; /* > 0, finite: luminance differences in units of the local standard deviation */
    float        sigma_normal;    /* > 0, finite */
    float        sigma_point;     /* > 0, finite */
    float        min_history;     /* >= 1, finite: below it the variance is estimated spatially */
    uint32_t     _p1;             /* must be 0 */
    const float* color;           /* [h][w][4]; device path: NULL = the handle's image */
    const float* normal;          /* [h][w][3] */
    const float* point;           /* [h][w][3] */
    const float* albedo;          /* [h][w][4] or NULL */
    const float* emission;        /* [h][w][4] or NULL */
    const float* moments;         /* [h][w][4] or NULL: .x, .y = accumulated first and second moment of the demodulated luminance */
    const float* history;         /* [h][w] or NULL: frames accumulated in `moments`; given exactly when `moments` is */
    float*       out;             /* [h][w][4] */
    float*       out_variance;    /* [h][w] or NULL; ignored by rt_luminance_moments */
} rt_vdenoise_desc;
enum { RT_VDENOISE_HOST_MEMORY = 1 };
int rt_denoise_variance(rt_handle* h, const rt_vdenoise_desc* desc, int flags);
int rt_luminance_moments(rt_handle* h, const rt_vdenoise_desc* desc, int flags);

/* Adaptive sampling: the link from rt_denoise_variance's out_variance back to the sampler.
 * rt_adaptive_plan apportions a budget of rays over the texels of a frame in proportion to their standard deviation and
 * writes the chosen texels' rays as one compacted rt_path_ray list; rt_radiance_rays traces that list; rt_adaptive_merge
 * blends the traced samples into the accumulation.  Frames are width x height, row 0 = bottom, tightly packed; texel
 * p = (x, y) has index y * width + x, "row-major order" below.
 *
 * rt_adaptive_plan.  Everything after the quantisation is integer arithmetic; the one float step is binary32, unfused.
 *   M = the largest variance(p) over the texels whose variance is finite and > 0 (as floats, which for these values is
 *   the order of their bit patterns as u32).
 *   q(p) = (u32)((sqrt_(variance(p)) / sqrt_(M)) * 1048576.0f), truncating, for a texel with a finite variance > 0, and
 *   0 for every other texel (0, negative, NaN, infinite) -- all of them when there is no M.  sqrt_ and the division are
 *   correctly rounded (csrc/rt_transc.h), so q <= 2^20.
 *   C(p) = the exclusive prefix sum of q in row-major order (u64); S = the sum of all q;
 *   R = budget - min_samples * width * height;  F(c) = floor(c * R / S) exactly (a 128-bit product: mul_div_floor of
 *   csrc/rt_adaptive.h);  e(p) = F(C(p) + q(p)) - F(C(p)), and 0 when S = 0;  n(p) = min(min_samples + e(p), max_samples).
 *   That is largest-remainder apportionment with the rounding error carried along the scan order: before the clamp the
 *   e(p) sum to R exactly (to 0 when S = 0).  What max_samples removes stays unspent (it is not redistributed).
 *   counts(p) = n(p);  offsets(p) = the exclusive row-major prefix sum of n;
 *   totals = { sum of n (<= budget), texels with n > min_samples, texels with min_samples + e > max_samples, 0 }.
 *   For k < n(p), rays[offsets(p) + k] = { origin, seed = (y * width + x) + (first_frame + k) * 719393 in u32 arithmetic
 *   (the seed of pixel p in frame first_frame + k, wgsl:475), dir(p) bit for bit, _p0 = 0 }.
 *   rays[totals[0] .. budget) are 32 zero bytes each: rt_radiance_rays answers a zero direction with (0, 0, 0, 0) and no
 *   work, so a caller traces `budget` rays without reading the total back.
 * Errors, nothing written: RT_ERR_INVALID_ARGUMENT (null handle / desc / plane, struct_bytes, _p0 or _p1 != 0, unknown
 * flags, zero width or height, budget outside 1 .. 2^31 - 1, max_samples outside 1 .. 65535, min_samples > max_samples,
 * min_samples * width * height > budget, misaligned device planes), RT_ERR_CAPACITY (width * height > 2^31 - 1),
 * RT_ERR_OUT_OF_MEMORY.
 *
 * rt_adaptive_merge.  One texel at a time, binary32, unfused, two products and then the sum (wgsl:156-157):
 *   acc = color(p) (four components), hl = history(p), m = moments(p).  If hl is not finite, hl < 1, or some component of
 *   color(p) is not finite there is no prior: hl = 0.
 *   For k = 0 .. counts(p) - 1 in order, with c = radiance[offsets(p) + k] (a record at or past `budget` ends the texel's
 *   samples: no read leaves the list) and, with moments, l = l(c.rgb / a'(p)) (rt_denoise_variance's l, rt_denoise's a';
 *   a' = 1 with a NULL albedo):
 *     some component of c not finite: the sample is dropped;
 *     otherwise, hl = 0:  acc = c bit for bit, m = (l, l l, 0, 0), hl = 1;
 *     otherwise:  n_c = hl < max_history ? hl : max_history;  w = 1 / (n_c + 1);  acc = acc * (1 - w) + c * w and
 *     m = m * (1 - w) + (l, l l, 0, 0) * w on four components each;  hl = n_c + 1.
 *   out(p) = acc, out_history(p) = hl, out_moments(p) = m -- and with hl still 0 (no prior and no valid sample)
 *   out(p) = color(p) bit for bit, out_history(p) = 0, out_moments(p) = moments(p).
 * A ray record is one unit of history whatever rays_per_pixel traced it with, as a frame is for rt_render.
 * Consequence: with min_samples = max_samples = N, budget = N * width * height, first_frame = 0, history 0,
 * max_history = +INF and a camera without jitter, plan -> rt_radiance_rays -> merge leaves what rt_render leaves after
 * frames 0 .. N - 1, bit for bit, alpha included.
 * Errors, nothing written: RT_ERR_INVALID_ARGUMENT (null handle / desc / radiance / counts / offsets / history / out /
 * out_history, a null color on the host or with the flag, moments without out_moments or the reverse, struct_bytes,
 * _p0 != 0, unknown flags, zero width or height, budget outside 1 .. 2^31 - 1, max_history NaN or below 1, misaligned
 * device planes), RT_ERR_CAPACITY (width * height > 2^31 - 1, or more texels than the image has with a NULL color),
 * RT_ERR_OUT_OF_MEMORY.
 *
 * Both: the _host forms (section 3) are these definitions over host pointers, without a device; the device calls compute
 * the same bits.  Without the HOST_MEMORY flag the planes are device pointers on the handle's device (4-byte aligned; 16
 * for rays, radiance, color, albedo, moments, out and out_moments) and the call is asynchronous on the handle's stream,
 * after every earlier call on the handle and before every later one; merge's `color` may be NULL for the handle's image,
 * and out / out_history / out_moments may be color / history / moments (or `out` the image); any other overlap is
 * undefined.  With the flag they are host pointers, staged whole through one temporary device buffer that is counted
 * against option "max_device_mb" while held, and the call returns when the outputs are on the host.  The plan keeps 32
 * bytes of scratch per 1024 texels (the block sums of its two scans) on the handle, grown on demand, counted by
 * rt_last_launch out[4] and bounded by "max_device_mb".  No scene is needed.  Like the denoisers the calls leave the image
 * (unless `out` is the image), the primary tables, a frame_ahead batch in flight, the pipeline slots, rt_get_stats and
 * the launch words of rt_last_launch as they are. */
typedef struct rt_adaptive_plan_desc {
    uint32_t        struct_bytes;   /* = sizeof(rt_adaptive_plan_desc) */
    uint32_t        _p0;            /* must be 0 */
    uint32_t        width, height;
    uint32_t        budget;         /* 1 .. 2^31 - 1: the number of records in `rays` */
    uint32_t        min_samples;    /* <= max_samples */
    uint32_t        max_samples;    /* 1 .. 65535 */
    uint32_t        first_frame;    /* the seed frame of a texel's sample 0 */
    float           origin[3];      /* the origin of every ray */
    uint32_t        _p1;            /* must be 0 */
    const float*    variance;       /* [h][w] */
    const float*    dir;            /* [h][w][3]: rt_render_gbuffer's `dir` plane */
    uint32_t*       counts;         /* [h][w] out */
    uint32_t*       offsets;        /* [h][w] out */
    rt_path_ray*    rays;           /* [budget] out */
    uint32_t*       totals;         /* [4] out */
} rt_adaptive_plan_desc;
typedef struct rt_adaptive_merge_desc {
    uint32_t        struct_bytes;   /* = sizeof(rt_adaptive_merge_desc) */
    uint32_t        _p0;            /* must be 0 */
    uint32_t        width, height;
    uint32_t        budget;         /* 1 .. 2^31 - 1: the number of records in `radiance` */
    float           max_history;    /* >= 1, may be +INF */
    const float*    radiance;       /* [budget][4]: what rt_radiance_rays wrote for the plan's rays */
    const uint32_t* counts;         /* [h][w] the plan's */
    const uint32_t* offsets;        /* [h][w] the plan's */
    const float*    color;          /* [h][w][4]; device path: NULL = the handle's image */
    const float*    history;        /* [h][w] */
    const float*    albedo;         /* [h][w][4] or NULL */
    const float*    moments;        /* [h][w][4] or NULL */
    float*          out;            /* [h][w][4]; may be `color` */
    float*          out_history;    /* [h][w]; may be `history` */
    float*          out_moments;    /* [h][w][4], given exactly when `moments` is; may be `moments` */
} rt_adaptive_merge_desc;
enum { RT_ADAPTIVE_HOST_MEMORY = 1 };
int rt_adaptive_plan(rt_handle* h, const rt_adaptive_plan_desc* desc, int flags);
int rt_adaptive_merge(rt_handle* h, const rt_adaptive_merge_desc* desc, int flags);

/* The test-only entry points (rt_test_*: the kernels' arithmetic building blocks evaluated element-wise on the device, raw
 * copies of sequence buffers, the RCCL gather against a stub, the frame_ahead policy) are NOT exported by the product
 * library: include/rt_test_abi.h declares them and ray_tracer_2_amd/librt2_mi355x_test.so -- the same sources compiled
 * with -DRT_TEST_ENTRIES=1 -- exports them beside everything declared here (round 5). */

const char* rt_last_error(rt_handle* h);
void rt_destroy(rt_handle* h);

/* Library-level queries (no device needed). */
const char* rt_version(void);
int rt_device_count(void);
/* sizeof() of every struct above, for FFI self-checks:
 * params, material, sphere, mesh, node, triangle, camera, scene. */
void rt_abi_sizes(uint32_t out[8]);

/* ------------------------------------------------------------------------ */
/* 3. Host side: scene pipeline (no device needed)                           */
/* ------------------------------------------------------------------------ */

typedef struct rt_scene rt_scene;

/* ≙ Scene::from_name + Scene::instantiate_scene (scene.rs:1003,179).
 * name: "cornell_box", "room", "room_2", "metal", "balls", "sponza",
 * "texture_test", "obj_test", "random_balls" / "random_balls:<seed>" (the reference draws this
 * scene from an OS-seeded generator, scene.rs:403, so its own runs never agree; this build makes
 * the same draws from a seeded one: a documented divergence).  assets_dir ≙ CARGO_MANIFEST_DIR/assets (asset.rs:50,108). */
int rt_scene_load_builtin(const char* name, const char* assets_dir, rt_scene** out);

/* Scene-definition API ≙ SceneDefinition::{set_camera, add_mesh, add_sphere}
 * (scene.rs:75-99). */
typedef struct rt_transform {
    float pos[3];
    float rot[4]; /* quaternion x, y, z, w */
    float scale[3];
} rt_transform;

typedef struct rt_camera_desc { /* ≙ CameraDescriptor (camera.rs:38-66) */
    rt_transform transform;
    float fov;
    float aspect;
    float near_plane;
    float far_plane;
    float focus_dist;
    float defocus_strength;
    float diverge_strength;
} rt_camera_desc;

int rt_scene_create(rt_scene** out);
int rt_scene_set_camera(rt_scene* s, const rt_camera_desc* cam);
/* ≙ Transform::cam (transform.rs:13-19): look-at camera transform. */
void rt_transform_cam(const float origin[3], const float look_at[3], rt_transform* out);
int rt_scene_add_sphere(rt_scene* s, const float centre[3], float radius, const rt_material* m);
/* MeshDefinition::FromFile (mesh.rs:33-36) */
int rt_scene_add_obj(rt_scene* s, const char* assets_dir, const char* path,
                     const rt_transform* t, int use_mtl, const rt_material* m);
/* MeshDefinition::FromData: n_vertices x (pos[3], normal[3], uv[2]) floats */
int rt_scene_add_mesh_data(rt_scene* s, const float* vertices8, uint32_t n_vertices,
                           const uint32_t* indices, uint32_t n_indices,
                           const rt_transform* t, const rt_material* m);
/* Texture registration for material.diffuse_index; returns the index or <0. */
int rt_scene_add_texture_rgba8(rt_scene* s, const uint8_t* rgba8, uint32_t w, uint32_t h);
/* ≙ BVH::build_per_mesh(meshes, Quality::High) (bvh.rs:152-207);
 * quality: 0 = Low, 1 = High, 2 = Disabled (bvh.rs:126-131). */
int rt_scene_build(rt_scene* s, int quality);
/* The same build with the SAH plane searches (find_best_split, src/core/bvh.rs:299-351: the
 * O(150 n)-per-level part) of meshes with at least `min_triangles` triangles (0 = default 16384)
 * done on GPU `device`; nodes, node order and triangle order are bit-identical to rt_scene_build's
 * (evaluate_sah is order-independent: minima, maxima and integer counts).  device = -1 runs the
 * same level-wise build with the searches on the host (validation).  SURVEY 8(f)-4. */
int rt_scene_build_device(rt_scene* s, int quality, int device, uint32_t min_triangles);

/* Accessors: pointers stay valid until the scene is modified or destroyed. */
int rt_scene_get_uniform(const rt_scene* s, rt_scene_uniform* out); /* ≙ Scene::to_uniform */
uint32_t rt_scene_num_spheres(const rt_scene* s);
uint32_t rt_scene_num_meshes(const rt_scene* s);
uint32_t rt_scene_num_triangles(const rt_scene* s);
uint32_t rt_scene_num_nodes(const rt_scene* s);
uint32_t rt_scene_num_textures(const rt_scene* s);
const rt_sphere* rt_scene_spheres(const rt_scene* s);
const rt_mesh_uniform* rt_scene_meshes(const rt_scene* s);
const rt_packed_triangle* rt_scene_triangles(const rt_scene* s);
const rt_node* rt_scene_nodes(const rt_scene* s);
int rt_scene_get_texture(const rt_scene* s, uint32_t i, rt_texture_desc* out);
const char* rt_scene_mesh_label(const rt_scene* s, uint32_t i);
/* Raw (pre-BVH) geometry of mesh instance i, in file order: n_vertices x
 * (pos[3], normal[3], uv[2]) floats and the index list (≙ MeshData,
 * geometry/mesh.rs:8-12).  Pass NULL outputs to query the counts. */
int rt_scene_mesh_data(const rt_scene* s, uint32_t i, float* vertices8, uint32_t* n_vertices,
                       uint32_t* indices, uint32_t* n_indices, rt_transform* transform,
                       rt_material* material);
uint32_t rt_scene_num_mesh_instances(const rt_scene* s);
const char* rt_scene_last_error(const rt_scene* s);
void rt_scene_destroy(rt_scene* s);

/* Convenience: upload everything a built scene holds to a device handle
 * (≙ load_scene_gpu_resources + update_buffers). */
int rt_upload_built_scene(rt_handle* h, const rt_scene* s);
/* rt_update_instances from a built rt_scene whose geometry is the one uploaded (after the setters below). */
int rt_update_built_scene(rt_handle* h, const rt_scene* s);
/* rt_refit_triangles with the packed triangles of mesh instances [first_mesh, first_mesh + n_meshes) of a built rt_scene
 * whose topology is the one uploaded (after rt_scene_set_mesh_vertices), from host memory. */
int rt_refit_built_scene(rt_handle* h, const rt_scene* s, uint32_t first_mesh, uint32_t n_meshes);

/* Inspector edits of a scene (≙ the egui drag widgets, src/rendering/egui.rs:240-330).  i is a mesh instance
 * (rt_scene_num_mesh_instances) / a sphere index.  On a built scene the instance's rt_mesh_uniform is rewritten the
 * way rt_scene_build makes it (Transform::to_matrix and its inverse, the material); the BVH is not rebuilt and the
 * scene stays built, so rt_update_built_scene sends the change.  A bad index or a null pointer gives
 * RT_ERR_INVALID_ARGUMENT (rt_scene_last_error says which). */
int rt_scene_set_mesh_transform(rt_scene* s, uint32_t i, const rt_transform* t);
int rt_scene_set_mesh_material(rt_scene* s, uint32_t i, const rt_material* m);
int rt_scene_set_sphere(rt_scene* s, uint32_t i, const float centre[3], float radius, const rt_material* m);
/* Moved vertices of mesh instance i: n_vertices x (pos[3], normal[3], uv[2]) floats, as rt_scene_add_mesh_data takes
 * them; n_vertices must equal the instance's count, and its index list stays.  Copy-on-write when the instance shares
 * its mesh data with others (they keep the old vertices).  On a built scene the instance's packed triangles are repacked
 * in BVH order and its nodes refitted (rt_refit_bvh): the scene stays built and rt_refit_built_scene sends the change.
 * Refused (RT_ERR_INVALID_ARGUMENT, nothing changed) for another vertex count or a scene built with quality Disabled,
 * which has no packed triangles. */
int rt_scene_set_mesh_vertices(rt_scene* s, uint32_t i, const float* vertices8, uint32_t n_vertices);
/* The BVH order of a built scene's mesh instance i: out[k] (rt_mesh_uniform.triangles entries) is the source triangle, in
 * its index list, of packed triangle triangle_offset + k -- what a host needs to pack moved triangles itself, e.g. on the
 * device.  RT_ERR_INVALID_ARGUMENT on an unbuilt scene. */
int rt_scene_triangle_order(rt_scene* s, uint32_t i, uint32_t* out);

/* Uniform n x n barycentric split of every triangle of every mesh added so
 * far (SURVEY 8d stand-in for the missing Dragon_80K / dragon_large assets). */
int rt_scene_subdivide_meshes(rt_scene* s, uint32_t n);

/* ≙ the pixel loop of save_render_to_file (app.rs:408-460): gamma 1/2.2,
 * clamp, truncating u8, net vertical flip.  out: width*height*4 bytes. */
int rt_export_rgba8(const float* rgba32f, uint32_t width, uint32_t height, uint8_t* out);

/* The denoiser's definition (section 2: rt_denoise) in executable form: plain C++ over host pointers, no device.  `color`
 * is required; `out` may be `color`.  The same argument errors as rt_denoise (no handle, no flags, no alignment rule),
 * nothing written on an error, the reason in rt_last_error(NULL); RT_ERR_OUT_OF_MEMORY when the host has no room for the
 * 64 bytes per texel of working memory. */
int rt_denoise_host(const rt_denoise_desc* desc);

/* Temporal accumulation's definition (section 2: rt_temporal_accumulate) in executable form: plain C++ over host
 * pointers, no device, no working memory.  `color` is required; `out` may be `color`.  The same argument errors as
 * rt_temporal_accumulate (no handle, no flags, no alignment rule), nothing written on an error, the reason in
 * rt_last_error(NULL). */
int rt_temporal_accumulate_host(const rt_temporal_desc* desc);
/* The same for rt_temporal_accumulate_moving: `motions` is a host pointer. */
int rt_temporal_accumulate_moving_host(const rt_temporal_motion_desc* desc);
/* The same for rt_temporal_accumulate_deforming: motions, primitive, bary, flags and prev_triangles are host pointers. */
int rt_temporal_accumulate_deforming_host(const rt_temporal_deform_desc* desc);

/* The motion table of rt_temporal_accumulate_moving from two states of one scene (the arrays rt_update_instances takes,
 * before and after the edit): out[0, n_meshes + n_spheres), meshes first.  Plain C++, no device.  Binary32, unfused.
 * With the product of two column-major matrices as glam's Mat4 * Mat4 (csrc/host/glam_math.h: mat4_mul),
 *   (A B)[c][r] = ((A[0][r] B[c][0] + A[1][r] B[c][1]) + A[2][r] B[c][2]) + A[3][r] B[c][3]:
 * Mesh k:  moved = the 128 bytes of world_to_model and model_to_world differ between prev_meshes[k] and meshes[k];
 *   D = prev.model_to_world * cur.world_to_model and d[c][r] = D[c][r] (r < 3);
 *   N = cur.model_to_world * prev.world_to_model and nt[c][r] = N[r][c] (c, r < 3) -- the transpose of N's 3 x 3, which is
 *   the inverse transpose of d's linear part without an inversion.
 * Sphere j, record n_meshes + j:  moved = the 16 bytes of pos and radius differ;  s = prev.radius / cur.radius;
 *   d[c][r] = (c == r ? s : 0) for c < 3;  d[3][r] = prev.pos[r] - s * cur.pos[r];  nt = the identity.
 * The matrices are filled whether or not `moved` is set; _p is 0.  An array may be NULL when its count is 0.
 * RT_ERR_INVALID_ARGUMENT, nothing written: a null `out` with a non-zero total, a null array with a non-zero count. */
int rt_object_motions(const rt_mesh_uniform* prev_meshes, const rt_mesh_uniform* meshes, uint32_t n_meshes,
                      const rt_sphere* prev_spheres, const rt_sphere* spheres, uint32_t n_spheres, rt_object_motion* out);
/* The table of rt_temporal_accumulate_deforming: rt_object_motions' arguments and, per mesh, whether its vertices moved
 * between the two states (deformed[k] != 0).  Such a mesh's record has moved = 2, d[c][r] = prev_meshes[k].
 * model_to_world[c][r] (c < 4, r < 3) -- the previous triangle's model-space point goes straight to the previous world --
 * and nt[c][r] = prev_meshes[k].model_to_world[c][r] (c, r < 3): the shader carries normals by model_to_world as
 * directions (wgsl:386), not by the inverse transpose.  Every other record is rt_object_motions' byte for byte.
 * RT_ERR_INVALID_ARGUMENT, nothing written: rt_object_motions', and a null `deformed` with n_meshes > 0. */
int rt_object_motions_deforming(const rt_mesh_uniform* prev_meshes, const rt_mesh_uniform* meshes, uint32_t n_meshes,
                                const rt_sphere* prev_spheres, const rt_sphere* spheres, uint32_t n_spheres,
                                const uint8_t* deformed /* [n_meshes] */, rt_object_motion* out);

/* The variance-guided denoiser's definition (section 2: rt_denoise_variance, rt_luminance_moments) in executable form:
 * plain C++ over host pointers, no device.  `color` is required; `out` may be `color`.  The same argument errors as the
 * device entry points (no handle, no flags, no alignment rule), nothing written on an error, the reason in
 * rt_last_error(NULL); RT_ERR_OUT_OF_MEMORY when the host has no room for the working memory. */
int rt_denoise_variance_host(const rt_vdenoise_desc* desc);
int rt_luminance_moments_host(const rt_vdenoise_desc* desc);

/* Adaptive sampling's definitions (section 2: rt_adaptive_plan, rt_adaptive_merge) in executable form: plain C++ over host
 * pointers, no device, no working memory.  merge's `color` is required.  The same argument errors as the device entry
 * points (no handle, no flags, no alignment rule), nothing written on an error, the reason in rt_last_error(NULL). */
int rt_adaptive_plan_host(const rt_adaptive_plan_desc* desc);
int rt_adaptive_merge_host(const rt_adaptive_merge_desc* desc);

/* Guided upsampling: a frame traced at a LOW resolution carried onto the G-buffer of a HIGH one by
 * a joint bilateral filter -- bilinear taps of the low frame, each validated against the high texel's own first hit as
 * rt_temporal_accumulate validates its history taps.  The low frame is w x h (lo_width x lo_height), the high frame W x H
 * (width x height); both have row 0 at the bottom, every plane tightly packed, and both were produced under the SAME
 * camera: lo_point, lo_normal and lo_object are rt_render_gbuffer's planes at w x h, depth .. emission its planes at
 * W x H.  Any pair of sizes is allowed, equal and downscaling ones included.  Everything is binary32 and unfused, in this
 * order.
 *   Once per call, on the host: rx = (f32(w) - 1) / (f32(W) - 1), or 0 when W == 1; ry likewise from h and H.  Texel x of a
 *   frame n wide looks through u = x / (n - 1) (wgsl:479), so high texel P = (X, Y) lies at the low position
 *   fx = f32(X) * rx, fy = f32(Y) * ry.
 *   Snap, per axis, rt_temporal_accumulate's (S = 1/64): x0 = floor(fx), tx = fx - f32(x0); if tx <= S then tx = 0,
 *   otherwise if tx >= 1 - S then x0 += 1 and tx = 0.  Likewise (y0, ty).
 *   P is GUIDED when some component of normal(P) is non-zero; normal(P) and point(P) are finite; depth(P) is finite and
 *   > 0; object(P) != 0xffffffff; and `emission` is NULL or the first three components of emission(P) are all zero.
 *   Every other texel (a miss, a lamp, a NaN) is PLAIN.
 *   A low tap q with weight b is VALID when b > 0; q is inside the low frame; all four components of lo_color(q) are
 *   finite; and lo_object(q) == object(P) (a miss matches a miss, a lamp its own lamp).  For a GUIDED P also: some
 *   component of lo_normal(q) is non-zero; lo_normal(q) and lo_point(q) are finite; with a = lo_point(q) - point(P) and
 *   n = normal(P), |(a0 n0 + a1 n1) + a2 n2| <= point_tolerance * depth(P); and with m = lo_normal(q),
 *   ((n0 m0 + n1 m1) + n2 m2) >= normal_cos.
 *   c(q) = lo_color(q) -- but when P is GUIDED and both albedo planes are given, components k = 0 .. 2 are
 *   lo_color(q)_k / a'(lo_albedo(q)_k) with a' rt_denoise's floor at 2^-10; alpha as it is.
 *   A valid tap adds b * c(q) (four components) to sum and b to wsum, both from +0, in tap order.
 *   RING 1: rt_temporal_accumulate's four taps (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1) with its weights
 *   (1-tx)(1-ty), tx(1-ty), (1-tx)ty, tx ty.  If wsum > 0: v = sum / wsum and coverage(P) = 2.
 *   RING 2, only when ring 1 left wsum not > 0: sum and wsum from +0 again over the sixteen taps (x0 + i, y0 + j),
 *   j = -1 .. 2 (outer), i = -1 .. 2 (inner), b = kx * ky with kx = 1 - |f32(i) - tx| * 0.5 and ky = 1 - |f32(j) - ty| * 0.5
 *   (a tent of half-width two low texels).  If wsum > 0: v = sum / wsum and coverage(P) = 1.
 *   HOLE, when both rings fail: v = c(q) of the nearest low texel q = (x0 + (tx > 0.5), y0 + (ty > 0.5)), each coordinate
 *   clamped into the low frame, whatever that texel holds; coverage(P) = 0.
 *   Result: out(P) = (v0 * albedo(P)_0, v1 * albedo(P)_1, v2 * albedo(P)_2, v3) when P is GUIDED and both albedo planes are
 *   given (albedo(P) as it is, not floored), and out(P) = v otherwise.
 * Consequences.  (1) With w == W, h == H, the low planes being the high planes themselves, no albedo planes and
 * normal_cos <= 0.99, every texel whose colour is finite takes one tap of weight 1 and `out` is `color` bit for bit (a
 * component that is -0 comes out +0).  (2) With W == 2w - 1 and H == 2h - 1, rx and ry are exactly 0.5 and the texels with
 * X and Y even are looked through by the very rays of the low texels (X/2, Y/2): with both G-buffers from
 * rt_render_gbuffer and no albedo planes, out(X, Y) == lo_color(X/2, Y/2) bit for bit there, wherever that colour is
 * finite.  (3) rt_upsample and rt_upsample_host give the same bits for every input.
 * `coverage` (optional, one byte per high texel) says which rule produced the texel.  A caller can re-trace its zeros with
 * rt_radiance_rays from the high G-buffer's `dir` plane and the pixel's seeds; the library has no helper that does.
 * point_tolerance and normal_cos are rt_temporal_accumulate's, with depth(P) in the place of the view depth.
 * Without RT_UPSAMPLE_HOST_MEMORY the planes are device pointers on the handle's device (4-byte aligned; 16 for lo_color,
 * lo_albedo, albedo, emission and out; 1 for coverage), `lo_color` may be NULL for the handle's current image (w * h texels
 * of it), and the call is asynchronous on the handle's stream, after every earlier call on the handle and before every
 * later one.  With the flag they are host pointers, staged WHOLE through one temporary device buffer (44 to 60 bytes per
 * low texel, 48 to 81 per high texel, `out` in a place of its own) that is counted against option "max_device_mb" while
 * held (RT_ERR_OUT_OF_MEMORY past the cap), and the call returns when the outputs are on the host.
 * out and coverage must not overlap any input, nor each other: undefined.  The call keeps no scratch between calls.
 * Errors, nothing written: RT_ERR_INVALID_ARGUMENT (null handle or desc; a null plane other than lo_albedo, albedo,
 * emission, coverage, and lo_color on the device path; one albedo plane without the other; struct_bytes !=
 * sizeof(rt_upsample_desc); _p0 != 0; unknown flags; a zero width or height on either side; point_tolerance NaN, <= 0 or
 * infinite; normal_cos NaN or outside [-1, 1]; misaligned device planes), RT_ERR_CAPACITY (w * h or W * H > 2^31 - 1, or
 * more low texels than the image has with a NULL lo_color), RT_ERR_OUT_OF_MEMORY.  No scene is needed.
 * Like the ray queries the call leaves the image (unless `out` is the image), the primary tables, a frame_ahead batch in
 * flight, the pipeline slots, rt_get_stats and the launch words of rt_last_launch as they are. */
typedef struct rt_upsample_desc {
    uint32_t        struct_bytes;     /* = sizeof(rt_upsample_desc) */
    uint32_t        _p0;              /* must be 0 */
    uint32_t        lo_width, lo_height;
    uint32_t        width, height;
    float           point_tolerance;  /* > 0, finite: plane distance allowed per unit of depth(P) */
    float           normal_cos;       /* finite, in [-1, 1]: least dot product of the two normals */
    const float*    lo_color;         /* [h][w][4]; device path: NULL = the handle's image */
    const float*    lo_point;         /* [h][w][3] */
    const float*    lo_normal;        /* [h][w][3] */
    const uint32_t* lo_object;        /* [h][w] */
    const float*    lo_albedo;        /* [h][w][4] or NULL (with albedo, or not at all) */
    const float*    depth;            /* [H][W] */
    const float*    point;            /* [H][W][3] */
    const float*    normal;           /* [H][W][3] */
    const uint32_t* object;           /* [H][W] */
    const float*    albedo;           /* [H][W][4] or NULL */
    const float*    emission;         /* [H][W][4] or NULL */
    float*          out;              /* [H][W][4] */
    uint8_t*        coverage;         /* [H][W] or NULL: 2 = ring 1, 1 = ring 2, 0 = hole */
} rt_upsample_desc;
enum { RT_UPSAMPLE_HOST_MEMORY = 1 };
int rt_upsample(rt_handle* h, const rt_upsample_desc* desc, int flags);
/* The definition above in executable form: plain C++ over host pointers, no device, no working memory.  `lo_color` is
 * required.  The same argument errors as rt_upsample (no handle, no flags, no alignment rule), nothing written on an
 * error, the reason in rt_last_error(NULL). */
int rt_upsample_host(const rt_upsample_desc* desc);

/* ---- display frames: 8-bit output, tone mapping, auto exposure ----
 * rt_display turns the RGBA32F frame `color` (width x height, row 0 at the bottom, tightly packed) into four bytes per
 * texel: what the reference's window shows (shaders/renderer.wgsl onto a Bgra8UnormSrgb surface), with an exposure and a
 * tone curve in front for frames that leave [0, 1].  Everything is binary32, every operation rounded once, nothing fused,
 * and no transcendental function is evaluated.
 *   Exposure, once per call: e = exposure, or exposure * *exposure_scale (one product) when the pointer is given; a scale
 *   that is not finite and > 0 counts as 1 (e = exposure).
 *   Input, k = 0 .. 2: v = color_k * e; m = v >= 0 ? min(v, 2^64) : 0 (NaN and negatives become 0, +inf 2^64).
 *   Tone CLAMP: t = m.  Tone REINHARD: t = (m * (1 + m / (white * white))) / (1 + m), white * white rounded once per call;
 *   white = +inf gives m / (1 + m).  (A white so small that its square underflows makes t +inf, or NaN at m = 0, which the
 *   transfers below take as 1 and 0.)
 *   Transfer SRGB: byte = the number of k in 1 .. 255 with t >= T[k], where T[k] is the smallest binary32 whose exact sRGB
 *   encoding is >= (k - 1/2) / 255 -- the IEC 61966-2-1 decode (c <= 0.04045 ? c / 12.92 : ((c + 0.055) / 1.055)^2.4) of
 *   (k - 1/2) / 255 in exact arithmetic, rounded up to binary32 (csrc/rt_srgb_encode_lut.h, generated by
 *   tools/micro/gen_srgb_encode_lut.py).  This is round(255 srgb(clamp(t))) as a step function of 255 steps; NaN gives 0.
 *   Transfer LINEAR (for a surface that encodes): l = t > 0 ? min(t, 1) : 0 (NaN: 0); byte = (uint32)(l * 255 + 0.5).
 *   Alpha: the LINEAR rule on color_3 as it is -- no exposure, no tone.
 *   Layout: bytes (r, g, b, a), with bit 0 (RT_DISPLAY_LAYOUT_BGRA) (b, g, r, a); input row y goes to output row y, with bit
 *   1 (RT_DISPLAY_LAYOUT_TOP_FIRST) to row height - 1 - y: the top of the view first.
 * Consequences.  (1) CLAMP, SRGB, layout = RT_DISPLAY_LAYOUT_BGRA, exposure 1 and no scale pointer give the reference's
 * window byte for byte.  (2) Every value of rt_srgb_lut.h -- the decode table of the textures -- returns to its byte.
 * (3) rt_display and rt_display_host give the same bytes for every input.
 * Without RT_DISPLAY_HOST_MEMORY the planes are device pointers on the handle's device (color 16-byte aligned, out and
 * exposure_scale 4), `color` may be NULL for the handle's current image (width * height texels of it), and the call is
 * asynchronous on the handle's stream, after every earlier call on the handle and before every later one: an
 * exposure_scale that rt_auto_exposure wrote there is read in stream order, with no host round trip.  With the flag they
 * are host pointers, staged WHOLE through one temporary device buffer (20 bytes per texel) that is counted against option
 * "max_device_mb" while held (RT_ERR_OUT_OF_MEMORY past the cap), and the call returns when `out` is on the host.
 * out must not overlap color or exposure_scale: undefined.  The call keeps no scratch between calls.
 * Errors, nothing written: RT_ERR_INVALID_ARGUMENT (null handle or desc; null out; null color except on the device path;
 * struct_bytes != sizeof(rt_display_desc); _p0 or _p1 != 0; unknown tone, transfer, layout bits or flags; a zero width or
 * height; exposure NaN, <= 0 or infinite; with REINHARD a white that is NaN or <= 0; misaligned device planes),
 * RT_ERR_CAPACITY (width * height > 2^31 - 1, or more texels than the image has with a NULL color), RT_ERR_OUT_OF_MEMORY.
 * No scene is needed.  Like rt_upsample the call leaves the image, the primary tables, a frame_ahead batch in flight, the
 * pipeline slots, rt_get_stats and the launch words of rt_last_launch as they are. */
enum { RT_DISPLAY_TONE_CLAMP = 0, RT_DISPLAY_TONE_REINHARD = 1 };
enum { RT_DISPLAY_SRGB = 0, RT_DISPLAY_LINEAR = 1 };
enum { RT_DISPLAY_LAYOUT_BGRA = 1, RT_DISPLAY_LAYOUT_TOP_FIRST = 2 };
typedef struct rt_display_desc {
    uint32_t     struct_bytes;     /* = sizeof(rt_display_desc) */
    uint32_t     _p0;              /* must be 0 */
    uint32_t     width, height;
    uint32_t     tone;             /* RT_DISPLAY_TONE_CLAMP | RT_DISPLAY_TONE_REINHARD */
    uint32_t     transfer;         /* RT_DISPLAY_SRGB | RT_DISPLAY_LINEAR */
    uint32_t     layout;           /* bit 0: B,G,R,A instead of R,G,B,A; bit 1: top row first */
    uint32_t     _p1;              /* must be 0 */
    float        exposure;         /* finite, > 0 */
    float        white;            /* REINHARD: > 0, +inf allowed; ignored by CLAMP */
    const float* color;            /* [h][w][4]; device path: NULL = the handle's image */
    const float* exposure_scale;   /* one float or NULL: what rt_auto_exposure wrote */
    uint8_t*     out;              /* [h][w][4] */
} rt_display_desc;
enum { RT_DISPLAY_HOST_MEMORY = 1 };
int rt_display(rt_handle* h, const rt_display_desc* desc, int flags);
/* The definition above in executable form: plain C++ over host pointers, no device, no working memory.  `color` is
 * required.  The same argument errors as rt_display (no handle, no flags, no alignment rule), nothing written on an error,
 * the reason in rt_last_error(NULL). */
int rt_display_host(const rt_display_desc* desc);

/* rt_auto_exposure meters the frame `color` and writes one float, *scale, that rt_display takes as exposure_scale: the
 * factor that brings the frame's trimmed mean log-luminance to `key`.  It is all integers until the last operations, so no
 * order of summation exists.
 *   Luminance of a texel: Y = (0.2126 c0 + 0.7152 c1) + 0.0722 c2 (rt_denoise_variance's).
 *   Counting: a texel whose Y is NaN, <= 0 or +inf is not counted; any other falls into bin
 *   clamp((bits(Y) >> 20) - 888, 0, 255) -- the exponent and the top three mantissa bits: eight bins per octave over
 *   2^-16 .. 2^16, a piecewise-linear logarithm.  n_b is the number of texels in bin b.
 *   Trimming: N = sum n_b, lo = floor(N * low_permille / 1000), hi = floor(N * high_permille / 1000) in 64 bits.  Of the
 *   texels ranked in ascending bin order the ranks [lo, hi) are kept: k_b is the overlap of bin b's rank interval with it,
 *   N' = sum k_b, S = sum k_b * b.
 *   Mean: mbar = f32(S) / f32(N') (each conversion rounded to nearest); Ybar = as_float((uint32)((mbar + 888.5f) *
 *   1048576.0f)), the same map run backwards through a bin's midpoint; target = min(max(key / Ybar, min_scale), max_scale).
 *   With N' = 0, target = 1.
 *   Result: *scale = target; with a prev_scale that is finite and > 0, *scale = prev + (target - prev) * rate (every
 *   operation rounded).  `histogram`, where given, receives n_b untrimmed.
 * Device memory (no RT_AUTO_EXPOSURE_HOST_MEMORY): color 16-byte aligned (NULL: the handle's image), the others 4; the
 * call is asynchronous on the handle's stream, and `scale` may be prev_scale.  The handle keeps 1 KiB of scratch for the
 * global bins, counted against option "max_device_mb" like rt_adaptive_plan's.  Host memory: staged whole (16 bytes per
 * texel and three small planes) within the cap; returns when the outputs are on the host.
 * Errors, nothing written: RT_ERR_INVALID_ARGUMENT (null handle, desc or scale; null color except on the device path;
 * struct_bytes; _p0 != 0; unknown flags; a zero width or height; not 0 <= low_permille < high_permille <= 1000; key,
 * min_scale or max_scale NaN, <= 0 or infinite, or min_scale > max_scale; rate NaN or outside (0, 1]; misaligned device
 * planes), RT_ERR_CAPACITY (as rt_display), RT_ERR_OUT_OF_MEMORY.  No scene is needed; side effects as rt_display.
 * rt_auto_exposure and rt_auto_exposure_host give the same bits for every input. */
typedef struct rt_auto_exposure_desc {
    uint32_t     struct_bytes;                  /* = sizeof(rt_auto_exposure_desc) */
    uint32_t     _p0;                           /* must be 0 */
    uint32_t     width, height;
    uint32_t     low_permille, high_permille;   /* 0 <= low < high <= 1000: the ranks kept */
    float        key;                           /* finite, > 0: the luminance the mean is brought to (0.18) */
    float        min_scale, max_scale;          /* finite, 0 < min <= max */
    float        rate;                          /* in (0, 1]; used with prev_scale */
    const float* color;                         /* [h][w][4]; device path: NULL = the handle's image */
    const float* prev_scale;                    /* one float or NULL */
    uint32_t*    histogram;                     /* [256] or NULL */
    float*       scale;                         /* one float, required */
} rt_auto_exposure_desc;
enum { RT_AUTO_EXPOSURE_HOST_MEMORY = 1 };
int rt_auto_exposure(rt_handle* h, const rt_auto_exposure_desc* desc, int flags);
int rt_auto_exposure_host(const rt_auto_exposure_desc* desc);

/* The picture to the host: rt_snapshot_image / rt_read_snapshot's protocol with the display pass in the place of the
 * device-to-device copy.  rt_snapshot_display encodes the first width * height texels of the image, as they are after the
 * calls made so far, into a buffer of the handle's own (width * height * 4 bytes; desc->color and desc->out must be NULL;
 * desc->exposure_scale, if given, is a device pointer read in stream order) and does not block; rt_read_display_snapshot
 * brings the first `bytes` of that picture to the host on the copy stream and returns when they are there, without waiting
 * for frames rendered since.  The float pair keeps its buffer and its bits, and the two pairs may be interleaved.  The
 * buffer is allocated on first use (or growth), counted in rt_last_launch's out[4] and against option "max_device_mb":
 * RT_ERR_OUT_OF_MEMORY when it does not fit.  Errors otherwise as rt_display; RT_ERR_CAPACITY for more texels than the image
 * has; rt_read_display_snapshot: RT_ERR_INVALID_ARGUMENT before any snapshot or for more bytes than the last one has. */
int rt_snapshot_display(rt_handle* h, const rt_display_desc* desc);
int rt_read_display_snapshot(rt_handle* h, uint8_t* out, size_t bytes);

/* ---- history rectification: clip the reprojected history to the new frame ----
 * rt_temporal_accumulate and its _moving and _deforming forms keep a texel's history across camera moves, moving objects
 * and deforming meshes, but not across a change of the lighting: a history of n frames takes the new frame in at 1 / (n + 1)
 * and stays wrong for about n frames.  rt_temporal_rectify is the blend of those calls with variance clipping in front:
 * the REPROJECTED history is clamped, per colour channel, into mean +- clip_sigma standard deviations of the new frame's
 * colours around the texel, and a texel that had to be clamped has its history length cut to clip_history, so that new
 * samples take over quickly.
 * The reprojected history is what any of the three calls returns for a `color` plane of quiet NaNs: they drop a non-finite
 * sample (out = the reprojected prev_color, out_history = the reprojected, capped history length; a texel without
 * history gets out = NaN, out_history = 1).  `history` and `history_length` are those two planes, `color` is the frame the
 * NaNs stood in for; the moments of rt_denoise_variance go through a reprojection of their own and are `history_moments`.
 * Frames are width x height, row 0 at the bottom, every plane tightly packed.  Everything is binary32 and unfused, in this
 * order, r = radius, g = clip_sigma.
 *   NO HISTORY.  Texel p has no history when some component of history(p) is not finite, or history_length(p) is not finite
 *   or below 1.  Then out(p) = color(p) bit for bit, out_history(p) = 1, out_moments(p) = moments(p), out_clipped(p) = 0.
 *   WINDOW, for every other texel.  Taps q = p + (dx, dy) over dy = -r .. r (outer), dx = -r .. r (inner).  A tap COUNTS
 *   when q is inside the frame, the first three components of color(q) are finite, and `object` is NULL or
 *   object(q) == object(p).  A counted tap adds color(q)_k to s1_k and color(q)_k * color(q)_k to s2_k, k = 0 .. 2, all from
 *   +0, and 1 to the integer count c.
 *   BOX, with c >= 2 and g < +INF, per k = 0 .. 2: mu = s1_k / f32(c); m2 = s2_k / f32(c); v = m2 - mu * mu; v = v > 0 ? v : 0;
 *   sd = the correctly rounded square root of v; lo = mu - g * sd; hi = mu + g * sd; with h = history(p)_k,
 *   h' = h < lo ? lo : (h > hi ? hi : h).  The texel is CLIPPED when some h'_k differs in bits from h_k.  With c < 2 or
 *   g = +INF no box is formed, h' = h and the texel is not clipped.  Alpha is never clipped: h'_3 = h_3.
 *   LENGTH AND BLEND.  n = history_length(p); n' = (CLIPPED and clip_history < n) ? clip_history : n; w = 1 / (n' + 1);
 *   rest = 1 - w; out(p)_k = h'_k * rest + color(p)_k * w, k = 0 .. 3 (two products and a sum, rt_temporal_accumulate's
 *   blend); out_history(p) = n' + 1.  A color(p) with a component that is not finite is dropped: out(p) = h',
 *   out_history(p) = n'.  out_clipped(p) = 2 when CLIPPED, 1 otherwise.
 *   MOMENTS (the three planes come together or not at all) are blended with the same w and never clipped:
 *   out_moments(p)_k = history_moments(p)_k * rest + moments(p)_k * w; a history_moments(p) with a component that is not
 *   finite gives out_moments(p) = moments(p), and otherwise a moments(p) that is not finite gives history_moments(p).
 * Consequences.  (1) With clip_sigma = +INF, rt_temporal_rectify on the reprojected history (a call of
 * rt_temporal_accumulate, _moving or _deforming with NaNs for color) gives `out` and `out_history` of that call on `color`
 * itself, bit for bit -- for all three forms, any camera move, finite and non-finite samples.  (2) Under an unmoved
 * camera that is rt_render's own accumulation, bit for bit (rt_temporal_accumulate's consequence).  (3) Where the counted
 * colours of a window are all equal, to a value whose first c multiples and those of its square are exact in binary32 (a
 * colour of few mantissa bits: 0.5, 0.75, 3), mu is that colour, sd is 0 and a clipped history becomes that colour exactly;
 * for any other equal colours it comes within the sums' rounding of it.  (4) At a texel that is not clipped, any clip_sigma gives consequence 1's bits.  (5) rt_temporal_rectify and
 * rt_temporal_rectify_host give the same bits for every input.
 * What it does not do: a lamp that gets BRIGHTER widens the new frame's box with its own noise, the old, darker history
 * lies inside it and is not clipped -- the method reacts to a change that leaves the noise box, not to every change; the
 * window's statistics are taken on the raw colour, not the demodulated one, so texture detail widens the box; and a channel
 * is clamped on its own, which can shift a hue.
 * Unlike rt_temporal_accumulate's, this pass's lanes read their neighbours' `color`: out must not overlap color (an error,
 * below), object or moments (undefined).  out may be history, out_history may be history_length and out_moments may be
 * history_moments: each is touched at the texel's own place only, after it was read.
 * Without RT_RECTIFY_HOST_MEMORY the planes are device pointers on the handle's device (16-byte aligned for the [4] planes,
 * 4 for the others, 1 for out_clipped), `color` may be NULL for the handle's current image (width * height texels of it,
 * read only: an `out` that overlaps them is then an error), and the call is asynchronous on the handle's stream, after
 * every earlier call on the handle and before every later one.  With the flag they are host pointers, staged WHOLE through
 * one temporary device buffer (36 to 73 bytes per texel: out takes history's place, out_history history_length's,
 * out_moments history_moments') that is counted against option "max_device_mb" while held (RT_ERR_OUT_OF_MEMORY past the
 * cap), and the call returns when the outputs are on the host.  The call keeps no scratch between calls.
 * Errors, nothing written: RT_ERR_INVALID_ARGUMENT (null handle or desc; null history, history_length, out or out_history;
 * null color except on the device path; one or two of moments, history_moments and out_moments without the rest;
 * struct_bytes != sizeof(rt_rectify_desc); _p0 or _p1 != 0; unknown flags; a zero width or height; radius outside 1 .. 3;
 * clip_sigma NaN or < 0; clip_history NaN or < 1; out overlapping color; misaligned device planes), RT_ERR_CAPACITY
 * (width * height > 2^31 - 1, or more texels than the image has with a NULL color), RT_ERR_OUT_OF_MEMORY.  No scene is
 * needed.  Like rt_upsample the call leaves the image (unless `out` is in it), the primary tables, a frame_ahead batch in
 * flight, the pipeline slots, rt_get_stats and the launch words of rt_last_launch as they are. */
typedef struct rt_rectify_desc {
    uint32_t        struct_bytes;      /* = sizeof(rt_rectify_desc) */
    uint32_t        _p0;               /* must be 0 */
    uint32_t        width, height;
    uint32_t        radius;            /* 1, 2 or 3: the window is (2 r + 1)^2 texels */
    float           clip_sigma;        /* >= 0, +INF allowed (no clipping): the box's half-width in standard deviations */
    float           clip_history;      /* >= 1, +INF allowed (no cut): the history length a clipped texel keeps at most */
    uint32_t        _p1;               /* must be 0 */
    const float*    color;             /* [h][w][4] this frame's sample; device path: NULL = the handle's image */
    const float*    history;           /* [h][w][4] the reprojected history */
    const float*    history_length;    /* [h][w] its length */
    const uint32_t* object;            /* [h][w] or NULL: the G-buffer's object word */
    const float*    moments;           /* [h][w][4] or NULL: this frame's luminance moments */
    const float*    history_moments;   /* [h][w][4] or NULL: the reprojected moments */
    float*          out;               /* [h][w][4] */
    float*          out_history;       /* [h][w] */
    float*          out_moments;       /* [h][w][4] or NULL */
    uint8_t*        out_clipped;       /* [h][w] or NULL: 0 = no history, 1 = kept, 2 = clipped */
} rt_rectify_desc;
enum { RT_RECTIFY_HOST_MEMORY = 1 };
int rt_temporal_rectify(rt_handle* h, const rt_rectify_desc* desc, int flags);
/* The definition above in executable form: plain C++ over host pointers, no device, no working memory.  `color` is
 * required.  The same argument errors as rt_temporal_rectify (no handle, no flags, no alignment rule), nothing written on
 * an error, the reason in rt_last_error(NULL). */
int rt_temporal_rectify_host(const rt_rectify_desc* desc);

#ifdef __cplusplus
}
#endif

#endif /* RT_ABI_H */
