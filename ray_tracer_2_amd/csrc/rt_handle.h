// rt_handle.h -- what the four units of the device-side C ABI share (rt_api.hip: lifecycle, scene, options, the render
// path, image I/O; rt_api_queries.hip: caller-supplied rays; rt_api_frames.hip: the passes over a rendered frame;
// rt_api_test.hip: the test library's entry points): the launch declarations, the handle, and the few helpers that a second
// unit calls.  Private: not installed, not under include/.  A helper goes in here only when a second unit calls it; what
// one unit uses stays in that unit.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "host/launch_options.h"
#include "host/launch_state.h"
#include "host/scene_pack.h"
#include "rt_device.h"

// The launches' argument structs that the handle does not hold: a unit includes the header of what it launches (rt_refit.h,
// rt_*_api.h).
namespace rt2 {
enum class TemporalKind;
}
namespace rtd {
struct RefitArgs;
struct DenoiseArgs;
struct TemporalArgs;
struct VDenoiseArgs;
struct AdaptivePlanArgs;
struct AdaptiveMergeArgs;
struct UpsampleArgs;
struct RectifyArgs;
struct DisplayArgs;
struct AutoExposureArgs;
}  // namespace rtd

namespace rtd {
hipError_t launch_render(const RenderArgs& a, hipStream_t stream, bool fixed_allowed);
bool render_takes_simple(const RenderArgs& a);
bool render_takes_fixed(const RenderArgs& a);
size_t render_lds_bytes(const RenderArgs& a);
hipError_t launch_tile_order(const uint32_t* cost, uint32_t n_tiles, uint32_t max_cost, uint32_t* order,
                             hipStream_t stream);
hipError_t launch_frame_taper(const uint32_t* cost, uint32_t n_tiles, uint32_t max_cost, uint32_t cost_floor, uint32_t n_batch,
                              uint32_t head, uint32_t waves, uint32_t alpha, uint32_t* table, hipStream_t stream);
hipError_t launch_primary(const RenderArgs& a, void* table, bool with_hits, hipStream_t stream);
hipError_t launch_blend_frames(const BlendArgs& b, hipStream_t stream);
hipError_t launch_walk(const RenderArgs& a, uint32_t compute_units, hipStream_t stream);
hipError_t launch_query(const RenderArgs& a, const void* rays, unsigned long long n, void* out, bool any, bool prune_tmax,
                        uint32_t blocks, uint32_t compute_units, hipStream_t stream);
hipError_t launch_pick_ray(const RenderArgs& a, uint32_t x, uint32_t y, float4* ray, hipStream_t stream);
hipError_t launch_gbuffer(const RenderArgs& a, const GBufferArgs& g, hipStream_t stream);
hipError_t launch_radiance(const RenderArgs& a, const void* rays, uint32_t n, void* out, uint32_t* next_ray, uint32_t compute_units,
                           hipStream_t stream);
hipError_t launch_wf_shade(const RenderArgs& a, uint32_t blocks, hipStream_t stream);
hipError_t launch_wf_walk(const RenderArgs& a, uint32_t blocks, hipStream_t stream);
size_t wf_walk_lds_bytes(const RenderArgs& a);
hipError_t launch_refit_fit(const RefitArgs& a, hipStream_t stream);
hipError_t launch_refit_write(const RefitArgs& a, hipStream_t stream);
hipError_t launch_denoise(const DenoiseArgs& a, hipStream_t stream);
hipError_t launch_temporal(const TemporalArgs& a, rt2::TemporalKind kind, hipStream_t stream);
hipError_t launch_vdenoise(const VDenoiseArgs& a, hipStream_t stream);
hipError_t launch_luminance_moments(const VDenoiseArgs& a, hipStream_t stream);
hipError_t launch_adaptive_plan(const AdaptivePlanArgs& a, hipStream_t stream);
hipError_t launch_adaptive_merge(const AdaptiveMergeArgs& a, hipStream_t stream);
hipError_t launch_upsample(const UpsampleArgs& a, hipStream_t stream);
hipError_t launch_rectify(const RectifyArgs& a, hipStream_t stream);
hipError_t launch_display(const DisplayArgs& a, hipStream_t stream);
hipError_t launch_auto_exposure(const AutoExposureArgs& a, hipStream_t stream);
hipError_t launch_assemble(const float4* gathered, float4* image, uint32_t width, uint32_t height,
                           uint32_t world, unsigned long long pad_texels, hipStream_t stream);
#if defined(RT_DIAG) || defined(RT_DIAGT)
hipError_t diag_read(unsigned long long* out, bool reset);
#endif
#if defined(RT_DIAG) || defined(RT_WAVE_TIMES)
hipError_t diag_wave_times(unsigned long long* out);
#endif
}  // namespace rtd

using namespace rtd;

// The host packer (host/scene_pack.h): the facts of an uploaded scene that the handle keeps.
using rt2::InstanceFacts, rt2::MeshGeom, rt2::SceneGeom;

// The frame layout a buffer, a table or a history was made for (host/launch_state.h).
using rt2::FrameShape;

// primary table (rt_primary_kernel): every pixel's memo -- its constant primary ray and (option "primary_hits") that
// ray's hit -- valid for (camera, width, height, strip layout, scene, with / without hits); 64 B per pixel
struct PrimaryTable {
    void* table = nullptr;
    size_t texels = 0;
    bool valid = false, with_hits = false;  // (valid: cleared by whatever changes the scene or the walk that found the hits)
    rt_camera_uniform camera{};
    FrameShape shape;
};

// a fresh tile counter per launch: a ring of 64, zeroed in one go each time it wraps (launches on
// one stream are ordered, so every earlier user of the ring is done by then)
struct CounterRing {
    uint32_t* mem = nullptr;
    uint32_t slot = 0;
    hipError_t create(hipStream_t stream) {
        const hipError_t e = hipMalloc((void**)&mem, 64 * sizeof(uint32_t));
        slot = 0;
        return e != hipSuccess ? e : hipMemsetAsync(mem, 0, 64 * sizeof(uint32_t), stream);
    }
    hipError_t next(hipStream_t stream, uint32_t*& counter) {
        slot = (slot + 1) & 63u;
        counter = mem + slot;
        return slot == 0u ? hipMemsetAsync(mem, 0, 64 * sizeof(uint32_t), stream) : hipSuccess;
    }
};

// One frame in flight of the pipelined single frames (option "pipeline"): what is per slot.
struct PipeSlot {
    hipStream_t stream = nullptr;
    hipEvent_t sampled = nullptr;     // frame sampled into `scratch` (recorded on `stream`)
    hipEvent_t blended = nullptr;     // ... and blended out of it (recorded on the handle's stream)
    bool sampled_set = false, blended_set = false;
    float4* scratch = nullptr;        // (rt_handle::pipe_scratch_texels texels)
    FrameShape zeroed;                // the frame layout the scratch image's padding rows were zeroed for
    CounterRing work;                 // a ring of launch counters per pipe stream
    uint32_t* memo = nullptr;         // further global-memory primary-ray memos (pixel_cache == 2)
    size_t memo_words = 0;
    // A pipelined frame whose camera (or shape) is not the shared table's builds a table of its OWN pipeline slot on its own
    // stream -- ordered behind that slot's previous frame and read by nobody else, so no frame in flight has to finish
    // first: the frames of a moving camera overlap like those of a standing one (option "primary_per_slot", default 1).
    PrimaryTable primary;
};

struct rt_handle {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;  // created by rt_create; `stream` may be rebound (rt_set_stream)
    // one (start, stop) event pair per launch since the last rt_reset_timing
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    size_t ev_used = 0;
    // launches whose event pairs were harvested when the pool wrapped (rt_get_stats adds the live ones)
    double ev_ms_harvested = 0.0;
    unsigned long long launches_total = 0;             // since rt_reset_timing (the frames: ahead.frames_asked, .frames_speculative)
    // frame batches (rt_render_frames): scratch images of the frames in flight
    float4* batch_scratch = nullptr;
    size_t batch_scratch_texels = 0;
    // deferred walks (RenderArgs::park; the deferred mesh found at upload: inst.have_defer): the two park queues, their counters
#if RT_WALK2
    float4* walk2 = nullptr;           // experiment: two-level records of the deferred mesh (rt_device.h)
    uint32_t walk2_base = 0;
#endif
    float4* wf_state = nullptr;
    float4* wf_hit = nullptr;
    uint32_t* wf_lists = nullptr;     // two lists of wf_capacity slots
    uint32_t* wf_counts = nullptr;
    size_t wf_capacity = 0, wf_counts_capacity = 0;
    rt2::Options opt;                                  // what rt_set_option sets (host/launch_options.h)
    // Frames rendered ahead (option "frame_ahead", include/rt_abi.h; the depth: rt2::ahead_depth): which one-frame call
    // starts a batch in the batch scratch images and which calls only blend their slot of it (render_single asks, acts and
    // reports back), and the frames asked for / rendered ahead that rt_get_stats reports.
    rt2::AheadSequence ahead;
    uint64_t generation = 0;                           // bumped by everything that changes what a frame looks like
    // rt_snapshot_image / rt_read_snapshot: a copy of the image taken in stream order (device to device), read back on a
    // stream of its own while the handle's stream renders the next frames
    float4* snapshot = nullptr;
    size_t snapshot_capacity = 0, snapshot_bytes = 0;  // bytes allocated / bytes of the last snapshot
    // rt_denoise: per texel a guide record of two float4 and two colour images of one float4 each (64 B), kept between calls
    float4* denoise_scratch = nullptr;
    size_t denoise_scratch_bytes = 0;
    // rt_adaptive_plan: the block sums of its two scans and a few words (rt_adaptive_api.h), kept between calls
    void* adaptive_scratch = nullptr;
    size_t adaptive_scratch_bytes = 0;
    // rt_auto_exposure: the 256 global bins of its histogram (1 KiB), kept between calls
    uint32_t* exposure_scratch = nullptr;
    size_t exposure_scratch_bytes = 0;
    // rt_snapshot_display / rt_read_display_snapshot: the float pair's protocol on a buffer of four bytes per texel that the
    // display kernel fills (0 bytes until first used)
    uint8_t* display_snapshot = nullptr;
    size_t display_snapshot_capacity = 0, display_snapshot_bytes = 0;
    hipEvent_t display_taken = nullptr, display_read = nullptr;
    bool display_read_pending = false;
    hipStream_t copy_stream = nullptr;
    hipEvent_t snapshot_taken = nullptr, snapshot_read = nullptr;
    bool snapshot_read_pending = false;                // a read of the staging buffer was queued since the last snapshot
    PipeSlot pipe[rt2::PIPE_MAX];
    hipEvent_t pipe_book = nullptr;                    // the last tile-order / primary-table rebuild (recorded on a pipe stream)
    hipEvent_t pipe_main = nullptr;                    // the last launch that was not pipelined (recorded on the handle's stream)
    bool pipe_book_set = false, pipe_main_set = false;
    bool pipe_main_need = true;                        // pipelined frames have to wait for pipe_main before they sample (render_impl)
    size_t pipe_scratch_texels = 0;                    // texels of every slot's scratch image
    uint32_t pipe_seq = 0;
    float4* small_blob = nullptr;
    SceneLayout small_lay{};
    uint32_t small_stack_entries = 1;
    bool small_ok = false;
    float4* park_queue[2] = {nullptr, nullptr};
    size_t park_capacity = 0;  // records per queue
    uint32_t* park_counts = nullptr;
    // rt_render_multi: what the root's stream has to finish before this handle's image may be overwritten
    // (owned by THIS handle, created on the root's device -- an event is recorded on a stream of its own device --,
    // so that destroying the root first leaves nothing dangling)
    hipEvent_t multi_copied = nullptr;
    int multi_copied_device = -1;
    bool multi_copy_pending = false;
    // batch scratch: the frame layout its padding rows were zeroed for
    FrameShape batch_zeroed;
    // root side of rt_render_multi
    std::vector<void*> multi_comms;       // ncclComm_t per rank
    std::vector<int> multi_comm_devices;  // the device list the communicators were made for
    std::set<int> multi_peers_enabled;
    uint32_t top_available = 0;  // breadth-first numbered top records of the biggest mesh's BVH (from geom.top_mesh_base on)
    float4* own_image = nullptr;  // allocated by rt_create; `image` may be rebound
    float4* multi_gathered = nullptr;  // rt_render_multi root: [world][pad_texels]
    float4* multi_frame = nullptr;     // rt_render_multi root: assembled full frame
    size_t multi_gathered_texels = 0, multi_frame_texels = 0;
    hipEvent_t multi_event = nullptr;
    size_t image_texels = 0;
    unsigned long long paths_total = 0;  // camera paths started since rt_reset_timing
    uint32_t max_width = 0, max_height = 0;
    float4* image = nullptr;
    Counters* counters = nullptr;
    CounterRing work;  // ring of per-launch tile counters (launches on the handle's stream)
    uint32_t* pixel_cache_mem = nullptr;  // primary-ray cache when LDS has no room (persistent kernel)
    size_t pixel_cache_words = 0;
    // tile-cost feedback: rays per tile of the previous frame order the next frame's tiles
    uint32_t* tile_cost[2] = {nullptr, nullptr};
    uint32_t* tile_order = nullptr;
    // The taper of the grouped launches (RenderArgs::frame_taper): two tables of rt2::TAPER_WORDS words -- the one that
    // rt_frame_taper_kernel wrote behind the last tile order (tiles.taper_batch, .taper_head say what for), and the one a
    // test forces (rt_test_frame_taper: its segments' first ranks and group sizes).
    uint32_t* frame_taper = nullptr;
    const uint32_t* last_taper = nullptr;  // the table of the last launch (null: it ran untapered)
    std::vector<uint32_t> taper_forced;
    uint32_t tile_capacity = 0;
    rt2::TileSchedule tiles;  // when the order is rewritten and the costs are recorded, and into which table (tile_feedback)
    PrimaryTable primary;  // the shared table (every stream's frames read it); the slots' own: PipeSlot::primary
    // The camera of the last sampled frame: a frame whose camera is another one (the camera is MOVING) renders without a
    // table (rt2::choose_primary) -- every pixel computes its own memo, its primary ray is traversed once, by its first sample.
    rt2::SampledCamera last_sampled;
    uint32_t compute_units = 1;  // of the device (rt_create); sizes the walk kernel's grid whatever "persistent_blocks" says
    float* srgb_lut = nullptr;
    // scene
    bool have_scene = false;
    float4* blob = nullptr;  // the scene, see rt_scene_format.h
    SceneGeom geom;          // the geometry phase's facts of the uploaded scene (rt_update_instances)
    InstanceFacts inst;      // the instance phase's decisions of the last upload / update: layout, items, trees, deferred mesh
    std::vector<rt_mesh_uniform> inst_meshes;  // the instance phase's inputs of the last upload / update (rt_refit_triangles
    std::vector<rt_sphere> inst_spheres;       // reruns it)
    bool lds_scene = false;  // the scene fits the LDS beside the stacks (commit_scene; option "lds_scene" = 0 overrides)
    DTexture* textures = nullptr;
    std::vector<uint8_t*> texture_data;
    uint32_t n_textures = 0;
    uint32_t stack_entries = 1;
    bool stack_wide = false, stack_must_wide = false;
    rt_camera_uniform camera{};
    int count_tests = 0;
    uint32_t last_launch[4] = {0, 0, 0, 0};  // rt_last_launch (entries 4 and 5 are computed when asked)
    uint32_t frame_group_forced = 0, last_frame_group = 1;  // rt_test_frame_group (0: rt2::frame_group_for decides)
    // The terminal skip (RenderArgs::terminal_dark): what rt2::terminal_skip_scene said of the head of the last upload /
    // update / refit, the switch (rt_test_terminal_skip: the test library's) and the mask of the last render launch.
    rt2::TerminalScene terminal;
    bool terminal_skip_on = true;
    uint32_t last_terminal_dark = 0;
    bool fixed_switches_on = true;           // rt_test_fixed_switches (the test library's): false keeps every launch on the general kernels
    bool queues_noted = false;               // the note about GPU_MAX_HW_QUEUES has been left in `err` once
    std::string err;
};

// The helpers that cross a unit boundary.  Defined in rt_api.hip, beside what they work on (query_args: rt_api_queries.hip);
// their comments are there.
namespace rth {
int fail(rt_handle* h, int code, const std::string& msg);  // (keeps `msg` for rt_last_error: the handle's, and the thread's)
bool fits_cap(const rt_handle* h, size_t extra, size_t freed = 0);
int replace_dev(rt_handle* h, void** p, size_t& have, size_t need, size_t each);
int wait_pending_copy(rt_handle* h);
int drain_streams(rt_handle* h);
void scene_args(const rt_handle* h, RenderArgs& a);
RenderArgs query_args(const rt_handle* h, const rt_params* params);
size_t staging_room(const rt_handle* h);

#define HIP_TRY(h, expr)                                                                   \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return fail(h, RT_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

template <typename T>
void free_dev(T*& p) {
    if (p) {
        (void)hipFree(p);
        p = nullptr;
    }
}

// Grow a device buffer that only the launches on `reader` read: synchronise them, then replace it.
template <typename T>
int regrow(rt_handle* h, T*& p, size_t& have, size_t need, hipStream_t reader) {
    if (have >= need) return RT_OK;
    HIP_TRY(h, hipStreamSynchronize(reader));
    return replace_dev(h, (void**)&p, have, need, sizeof(T));
}

template <typename T>
int upload(rt_handle* h, T*& dst, const T* src, size_t n) {
    size_t bytes = (n ? n : 1) * sizeof(T);
    HIP_TRY(h, hipMalloc((void**)&dst, bytes));
    if (n) HIP_TRY(h, hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyHostToDevice, h->stream));
    return RT_OK;
}

// The loop of a host-memory call (the ray queries, rt_render_gbuffer, rt_radiance_rays): one temporary device buffer of
// `bytes` (what_for: its name in the out-of-memory message), then step(buf, i0, m, what) for the chunks [i0, i0 + m) of the
// call's n items.  A step queues its chunk's copies and launch on the handle's stream; when one of them fails it names it in
// `what` and returns its error.  The stream is drained after every chunk -- the buffer is used again, and the results are on
// the host when the call returns -- and before the buffer is freed, whatever happened.
template <class Step>
static int staged_chunks(rt_handle* h, size_t bytes, uint64_t n, uint64_t chunk, const char* what_for, Step&& step) {
    auto hip_fail = [&](const char* what, hipError_t e) { return fail(h, RT_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e)); };
    uint8_t* buf = nullptr;
    hipError_t e = hipMalloc((void**)&buf, bytes);
    if (e != hipSuccess)
        return e == hipErrorOutOfMemory ? fail(h, RT_ERR_OUT_OF_MEMORY, std::string("no device memory for ") + what_for) : hip_fail("hipMalloc", e);
    int rc = RT_OK;
    for (uint64_t i0 = 0; rc == RT_OK && i0 < n; i0 += chunk) {
        const char* what = "hipStreamSynchronize";
        e = step(buf, i0, std::min<uint64_t>(chunk, n - i0), what);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) rc = hip_fail(what, e);
    }
    if (rc != RT_OK) (void)hipStreamSynchronize(h->stream);  // (nothing may still use the buffer when it is freed)
    free_dev(buf);
    return rc;
}
}  // namespace rth

using namespace rth;
