// rt_api.hip -- section 2 of include/rt_abi.h: the device-side C ABI that
// replaces RayTracer (src/rendering/ray_tracer.rs) of the reference.
//
// Ownership and threading follow the reference's use of RayTracer: one handle
// per device, calls from one thread at a time, inputs are borrowed and copied
// before the call returns, errors are integer codes (never exceptions or
// aborts across the boundary).
#include <hip/hip_runtime.h>


#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <set>
#include <string>
#include <vector>

#include "host/bvh.h"  // (rt2::refit_select / refit_bvh: the selection rule shared with the host refit)
#include "host/launch_options.h"  // (the option table and the launch rules: plain C++, tested on the CPU)
#include "host/launch_state.h"  // (the rules that keep state from call to call: tile schedule, frames rendered ahead, primary table)
#include "host/scene_pack.h"  // (the host packer: scene arrays -> blob)
#include "rt_device.h"
#include "rt_refit.h"
#include "rt_denoise_api.h"  // (the denoiser: its argument rules and host restatement, host/denoise.cpp; its launch, rt_denoise.hip)
#include "rt_upsample_api.h"  // (guided upsampling: its argument rules and host restatement, host/upsample.cpp; its launch, rt_upsample.hip)
#include "rt_display_api.h"  // (the display pass and the exposure meter: their argument rules and host restatements, host/display.cpp; their launches, rt_display.hip)
#include "rt_temporal_api.h"  // (temporal accumulation: its argument rules and host restatement, host/temporal.cpp; its launch, rt_temporal.hip)
#include "rt_vdenoise_api.h"  // (the variance-guided denoiser: its argument rules and host restatement, host/vdenoise.cpp; its launches, rt_vdenoise.hip)
#include "rt_adaptive_api.h"  // (adaptive sampling: its argument rules and host restatement, host/adaptive.cpp; its launches, rt_adaptive.hip)
#include "rt_rccl.h"  // (types of <rccl/rccl.h>; the library itself is loaded on first multi-device use)
#ifndef RT_TEST_ENTRIES
#define RT_TEST_ENTRIES 0
#endif
#if RT_TEST_ENTRIES
#include "../../include/rt_test_abi.h"
#endif
#include "rt_srgb_lut.h"

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
#if RT_TEST_ENTRIES
hipError_t launch_units(int fn, const float* x, const float* y, float* out, unsigned long long n, hipStream_t stream);
hipError_t launch_sweep(int which, unsigned long long* out, hipStream_t stream);
hipError_t launch_test_intersect(const RenderArgs& a, const float* ro, const float* rd, const uint8_t* active,
                                 unsigned long long n, bool simple, bool stats, uint32_t* out, hipStream_t stream);
hipError_t launch_units_texture(const uint8_t* rgba8, uint32_t width, uint32_t height, const float* srgb_lut, const float* uv,
                                float* out, unsigned long long n, hipStream_t stream);
hipError_t launch_test_shade(const RenderArgs& a, int which, const uint32_t* cases, const uint8_t* active, unsigned long long n,
                             bool simple, bool fast_miss, bool total_lds, uint32_t* out, hipStream_t stream);
#endif
hipError_t launch_refit_fit(const RefitArgs& a, hipStream_t stream);
hipError_t launch_refit_write(const RefitArgs& a, hipStream_t stream);
hipError_t launch_denoise(const DenoiseArgs& a, hipStream_t stream);
hipError_t launch_temporal(const TemporalArgs& a, rt2::TemporalKind kind, hipStream_t stream);
hipError_t launch_vdenoise(const VDenoiseArgs& a, hipStream_t stream);
hipError_t launch_luminance_moments(const VDenoiseArgs& a, hipStream_t stream);
hipError_t launch_adaptive_plan(const AdaptivePlanArgs& a, hipStream_t stream);
hipError_t launch_adaptive_merge(const AdaptiveMergeArgs& a, hipStream_t stream);
hipError_t launch_upsample(const UpsampleArgs& a, hipStream_t stream);
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

namespace {

// GPU_MAX_HW_QUEUES as the host set it (rt2::pipeline_depth says why it matters).  The variable is read ONCE, when
// the first handle is created -- the HIP runtime reads it once too, at initialisation: a host that changes it later would
// otherwise be given a depth for queues it does not have, ADVICE round 4.
int hw_queues_requested() {
    static const int queues = [] {
        const char* v = getenv("GPU_MAX_HW_QUEUES");
        const int q = v ? atoi(v) : 4;
        return q > 0 ? q : 4;
    }();
    return queues;
}
thread_local std::string g_err;

int fail(rt_handle* h, int code, const std::string& msg) {
    if (h) h->err = msg;
    g_err = msg;
    return code;
}

// bytes of device memory the handle holds on its own initiative (what option "max_device_mb" bounds)
size_t optional_bytes(const rt_handle* h) {
    size_t b = h->batch_scratch_texels * sizeof(float4) + h->pixel_cache_words * sizeof(uint32_t) + h->primary.texels * 64u +
               2u * (((h->park_capacity + 63) / 64) * (size_t)PARK_PLANES * 64u * sizeof(float4)) + h->snapshot_capacity +
               h->denoise_scratch_bytes + h->adaptive_scratch_bytes + h->exposure_scratch_bytes + h->display_snapshot_capacity;
    for (const PipeSlot& ps : h->pipe) {
        if (ps.scratch) b += h->pipe_scratch_texels * sizeof(float4);
        b += ps.memo_words * sizeof(uint32_t) + ps.primary.texels * 64u;
    }
    return b;
}
// may the handle take `extra` more bytes (after giving back `freed` of what it holds)?
bool fits_cap(const rt_handle* h, size_t extra, size_t freed = 0) {
    if (h->opt.max_device_mb == 0) return true;
    const size_t held = optional_bytes(h);
    return (held > freed ? held - freed : 0) + extra <= h->opt.max_device_bytes();
}

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

// A device buffer of `have` elements of `each` bytes is replaced by one of `need`: free, hipMalloc, record the size (0
// while there is no buffer).  Whoever may still read the old buffer has been synchronised by the caller.
int replace_dev(rt_handle* h, void** p, size_t& have, size_t need, size_t each) {
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    have = 0;
    HIP_TRY(h, hipMalloc(p, need * each));
    have = need;
    return RT_OK;
}
// Grow a device buffer that only the launches on `reader` read: synchronise them, then replace it.
template <typename T>
int regrow(rt_handle* h, T*& p, size_t& have, size_t need, hipStream_t reader) {
    if (have >= need) return RT_OK;
    HIP_TRY(h, hipStreamSynchronize(reader));
    return replace_dev(h, (void**)&p, have, need, sizeof(T));
}

// (host/launch_options.h repeats these figures of rt_device.h)
static_assert(rt2::BLOCKS_PER_CU == BLOCKS_PER_CU && rt2::WAVES_PER_BLOCK == WAVES_PER_BLOCK && rt2::MAX_BATCH_FRAMES == RT_MAX_BATCH_FRAMES, "");

// The blend weight pair of frame `frames` (wgsl:157-158): two separate IEEE operations, as the shader rounds them
// (i32 arithmetic wraps in the shader; frames = -1 gives +inf there too)
void blend_weights(int32_t frames, float& weight, float& rest) {
    volatile float w = 1.0f / (float)(int32_t)((uint32_t)frames + 1u);
    volatile float r = 1.0f - w;
    weight = w;
    rest = r;
}

// whatever the tables hold (the primary hits: a function of the scene and of the walk that found them) is stale
void invalidate_primary_tables(rt_handle* h) {
    h->primary.valid = false;
    for (PipeSlot& ps : h->pipe) ps.primary.valid = false;
}

// A pipeline slot's stream, events and counter ring (its scratch image, memo and table are made when a frame needs them)
int pipe_slot_create(rt_handle* h, PipeSlot& ps) {
    if (!ps.stream) HIP_TRY(h, hipStreamCreateWithFlags(&ps.stream, hipStreamNonBlocking));
    if (!ps.sampled) HIP_TRY(h, hipEventCreateWithFlags(&ps.sampled, hipEventDisableTiming));
    if (!ps.blended) HIP_TRY(h, hipEventCreateWithFlags(&ps.blended, hipEventDisableTiming));
    if (!ps.work.mem) HIP_TRY(h, ps.work.create(ps.stream));
    return RT_OK;
}
void pipe_slot_destroy(PipeSlot& ps) {
    if (ps.stream) {
        (void)hipStreamSynchronize(ps.stream);
        (void)hipStreamDestroy(ps.stream);
    }
    if (ps.sampled) (void)hipEventDestroy(ps.sampled);
    if (ps.blended) (void)hipEventDestroy(ps.blended);
    free_dev(ps.scratch);
    free_dev(ps.work.mem);
    free_dev(ps.memo);
    free_dev(ps.primary.table);
}

void free_scene(rt_handle* h) {
    free_dev(h->blob);
    free_dev(h->small_blob);
    h->small_ok = false;
    h->have_scene = false;
}

void free_textures(rt_handle* h) {
    for (uint8_t*& p : h->texture_data) free_dev(p);
    h->texture_data.clear();
    free_dev(h->textures);
    h->n_textures = 0;
}

template <typename T>
int upload(rt_handle* h, T*& dst, const T* src, size_t n) {
    size_t bytes = (n ? n : 1) * sizeof(T);
    HIP_TRY(h, hipMalloc((void**)&dst, bytes));
    if (n) HIP_TRY(h, hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyHostToDevice, h->stream));
    return RT_OK;
}

}  // namespace

namespace {
RcclApi g_rccl;

// (abort: the communicators' last group failed -- ncclCommAbort where the library has it)
void multi_drop_comms(rt_handle* root, bool abort = false) {
    if (g_rccl.lib)
        for (void* c : root->multi_comms) {
            if (abort) g_rccl.drop((ncclComm_t)c);
            else (void)g_rccl.CommDestroy((ncclComm_t)c);
        }
    root->multi_comms.clear();
    root->multi_comm_devices.clear();
}
}  // namespace

extern "C" {

const char* rt_version(void) { return RT_EXPERIMENTS ? "ray_tracer_2_amd 0.1 (gfx950) +experiments" : "ray_tracer_2_amd 0.1 (gfx950)"; }

int rt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void rt_abi_sizes(uint32_t out[8]) {
    out[0] = sizeof(rt_params);
    out[1] = sizeof(rt_material);
    out[2] = sizeof(rt_sphere);
    out[3] = sizeof(rt_mesh_uniform);
    out[4] = sizeof(rt_node);
    out[5] = sizeof(rt_packed_triangle);
    out[6] = sizeof(rt_camera_uniform);
    out[7] = sizeof(rt_scene_uniform);
}

const char* rt_last_error(rt_handle* h) { return h ? h->err.c_str() : g_err.c_str(); }

int rt_create(int device_ordinal, uint32_t max_width, uint32_t max_height, rt_handle** out) {
    if (!out || max_width == 0 || max_height == 0) return fail(nullptr, RT_ERR_INVALID_ARGUMENT, "bad arguments");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(nullptr, RT_ERR_DEVICE, "no HIP device available (this library has no CPU fallback)");
    if (device_ordinal < 0 || device_ordinal >= n) return fail(nullptr, RT_ERR_INVALID_ARGUMENT, "device ordinal out of range");
    rt_handle* h = new (std::nothrow) rt_handle();
    if (!h) return fail(nullptr, RT_ERR_OUT_OF_MEMORY, "out of host memory");
    h->device = device_ordinal;
    h->max_width = max_width;
    h->max_height = max_height;
    *out = h;
    (void)hw_queues_requested();   // (GPU_MAX_HW_QUEUES as the runtime is about to see it)
    HIP_TRY(h, hipSetDevice(device_ordinal));
    HIP_TRY(h, hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    h->stream = h->own_stream;
    size_t texels = (size_t)max_width * max_height;
    HIP_TRY(h, hipMalloc((void**)&h->own_image, texels * sizeof(float4)));
    h->image = h->own_image;
    h->image_texels = texels;
    HIP_TRY(h, hipMemsetAsync(h->image, 0, texels * sizeof(float4), h->stream));
    HIP_TRY(h, hipMalloc((void**)&h->counters, sizeof(Counters)));
    HIP_TRY(h, hipMemsetAsync(h->counters, 0, sizeof(Counters), h->stream));
    HIP_TRY(h, h->work.create(h->stream));
    h->tile_capacity = ((max_width + 7) / 8) * ((max_height + 7) / 8 + 1);
    for (int k = 0; k < 2; ++k) HIP_TRY(h, hipMalloc((void**)&h->tile_cost[k], (size_t)h->tile_capacity * sizeof(uint32_t)));
    HIP_TRY(h, hipMalloc((void**)&h->tile_order, (size_t)h->tile_capacity * sizeof(uint32_t)));
    HIP_TRY(h, hipMalloc((void**)&h->frame_taper, 2u * rt2::TAPER_WORDS * sizeof(uint32_t)));
    {
        hipDeviceProp_t prop;
        HIP_TRY(h, hipGetDeviceProperties(&prop, device_ordinal));
        // 4 waves per SIMD (the render kernels' register budget) = 4 workgroups of 4 waves per CU
        h->opt.persistent_blocks = prop.multiProcessorCount * (int)BLOCKS_PER_CU;
        h->compute_units = prop.multiProcessorCount > 0 ? (uint32_t)prop.multiProcessorCount : 1u;
    }
    static const float lut[256] = {RT_SRGB_LUT_VALUES};
    HIP_TRY(h, hipMalloc((void**)&h->srgb_lut, sizeof(lut)));
    HIP_TRY(h, hipMemcpyAsync(h->srgb_lut, lut, sizeof(lut), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return RT_OK;
}

void rt_destroy(rt_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->multi_copy_pending && h->multi_copied) (void)hipEventSynchronize(h->multi_copied);  // (the root still reads h->image)
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    free_scene(h);
    free_textures(h);
    free_dev(h->own_image);
    free_dev(h->multi_gathered);
    free_dev(h->multi_frame);
    free_dev(h->batch_scratch);
    free_dev(h->park_queue[0]);
    free_dev(h->park_queue[1]);
    free_dev(h->park_counts);
    for (PipeSlot& ps : h->pipe) pipe_slot_destroy(ps);
    if (h->pipe_book) (void)hipEventDestroy(h->pipe_book);
    if (h->pipe_main) (void)hipEventDestroy(h->pipe_main);
    if (h->copy_stream) {
        (void)hipStreamSynchronize(h->copy_stream);
        (void)hipStreamDestroy(h->copy_stream);
    }
    if (h->snapshot_taken) (void)hipEventDestroy(h->snapshot_taken);
    if (h->snapshot_read) (void)hipEventDestroy(h->snapshot_read);
    free_dev(h->snapshot);
    if (h->display_taken) (void)hipEventDestroy(h->display_taken);
    if (h->display_read) (void)hipEventDestroy(h->display_read);
    free_dev(h->display_snapshot);
    free_dev(h->exposure_scratch);
    free_dev(h->denoise_scratch);
    free_dev(h->adaptive_scratch);
    free_dev(h->wf_state);
    free_dev(h->wf_hit);
    free_dev(h->wf_lists);
    free_dev(h->wf_counts);
    if (h->multi_event) (void)hipEventDestroy(h->multi_event);
    if (h->multi_copied) (void)hipEventDestroy(h->multi_copied);
    if (g_rccl.lib)
        for (void* c : h->multi_comms) (void)g_rccl.CommDestroy((ncclComm_t)c);
    free_dev(h->counters);
    free_dev(h->work.mem);
    free_dev(h->primary.table);
    free_dev(h->pixel_cache_mem);
#if RT_WALK2
    free_dev(h->walk2);
#endif
    free_dev(h->tile_cost[0]);
    free_dev(h->tile_cost[1]);
    free_dev(h->tile_order);
    free_dev(h->frame_taper);
    free_dev(h->srgb_lut);
    for (auto& e : h->ev_pool) {
        (void)hipEventDestroy(e.first);
        (void)hipEventDestroy(e.second);
    }
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    delete h;
}

}  // extern "C"

namespace {

// The handle state of an uploaded scene, after its blob is on the device and h->geom / h->inst hold its facts: what
// follows from the layout and the kernels' LDS map.
void commit_scene(rt_handle* h, const rt_camera_uniform& camera) {
    const SceneGeom& g = h->geom;
    const InstanceFacts& s = h->inst;
    h->stack_entries = g.max_height ? g.max_height : 1;
    // One-dword stack entries hold 7 bits of leaf count and 24 bits of triangle index; they cost
    // a few instructions per push/pop, so they are used when they buy occupancy: when two-dword
    // entries would not leave room for the scene blob and the primary-ray memo in LDS.
    const bool wide_fits = s.lay.bytes + wave_lds_bytes(h->stack_entries, true, s.tlas_entries, true, true) <= LDS_BUDGET_BYTES;
    h->stack_must_wide = g.max_leaf_ref > 127u || g.n_triangles > (1u << 24);
    h->stack_wide = h->stack_must_wide || wide_fits;
    h->top_available = g.top_mesh_records >= 64 ? std::min<uint32_t>(g.top_mesh_records, 2048u) : 0u;
    // LDS residency: blob + the four waves' stacks, cost tables and lane state within the
    // per-workgroup budget (the primary-ray memo goes to LDS only if it still fits, see render_impl)
    h->lds_scene = s.lay.bytes + wave_lds_bytes(h->stack_entries, h->stack_wide, s.tlas_entries, true, false) <= LDS_BUDGET_BYTES;
    h->camera = camera;
    h->have_scene = true;
    h->tiles.reset();
    invalidate_primary_tables(h);  // (the tables hold hits: a function of the scene)
}

// Every launch enqueued so far on any of the handle's streams is complete (they all may read the blob).
int drain_streams(rt_handle* h) {
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (PipeSlot& ps : h->pipe)
        if (ps.stream) HIP_TRY(h, hipStreamSynchronize(ps.stream));
    return RT_OK;
}

// Where rt_update_instances / rt_refit_triangles (`who`) write the head of `lay`, once every launch that may read the blob
// is complete (the streams are drained): the blob itself while the head keeps its size; else a new blob, allocated before
// the drain, zeroed when the scene is empty (16 zero bytes), with the old blob's tail copied device to device on the
// handle's stream -- on any failure it is freed and the failure reported.  The caller writes the head (a refit: its boxes
// and triangle records first), synchronises and adopts the blob.
int drop_new_blob(rt_handle* h, float4* fresh, int rc) {  // (the current blob is not a new one: left alone)
    if (fresh == h->blob) return rc;
    (void)hipStreamSynchronize(h->stream);
    (void)hipFree(fresh);
    return rc;
}
int blob_for_head(rt_handle* h, const char* who, const SceneLayout& lay, uint64_t tail_bytes, float4*& fresh) {
    fresh = h->blob;
    if (lay.wide_off == h->inst.lay.wide_off) return drain_streams(h);
    if (hipMalloc((void**)&fresh, lay.bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, RT_ERR_OUT_OF_MEMORY, std::string(who) + ": no device memory for the resized scene");
    }
    if (int rc = drain_streams(h); rc != RT_OK) return drop_new_blob(h, fresh, rc);
    hipError_t e = (uint64_t)lay.wide_off + tail_bytes != lay.bytes ? hipMemsetAsync(fresh, 0, lay.bytes, h->stream) : hipSuccess;
    if (e == hipSuccess && tail_bytes)
        e = hipMemcpyAsync((char*)fresh + lay.wide_off, (const char*)h->blob + h->inst.lay.wide_off, tail_bytes, hipMemcpyDeviceToDevice, h->stream);
    return e == hipSuccess ? RT_OK : drop_new_blob(h, fresh, fail(h, RT_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e)));
}
// ... and, once the stream has completed everything written into it, a new blob takes the old one's place.
void adopt_blob(rt_handle* h, float4* fresh) {
    if (fresh == h->blob) return;
    free_dev(h->blob);
    h->blob = fresh;
}

}  // namespace

extern "C" {

int rt_upload_scene(rt_handle* h, const rt_scene_uniform* scene, const rt_sphere* spheres,
                    uint32_t n_spheres, const rt_mesh_uniform* meshes, uint32_t n_meshes,
                    const rt_packed_triangle* triangles, uint32_t n_triangles, const rt_node* nodes,
                    uint32_t n_nodes) {
    if (!h || !scene) return fail(h, RT_ERR_INVALID_ARGUMENT, "null handle or scene");
    h->generation += 1;
    if ((n_spheres && !spheres) || (n_meshes && !meshes) || (n_triangles && !triangles) || (n_nodes && !nodes))
        return fail(h, RT_ERR_INVALID_ARGUMENT, "null array with non-zero count");
    // ray_tracer.rs:15-19, bvh.rs:140
    if (n_meshes > RT_MAX_MESHES) return fail(h, RT_ERR_CAPACITY, "more than 400 meshes");
    if (n_spheres > RT_MAX_SPHERES) return fail(h, RT_ERR_CAPACITY, "more than 500 spheres");
    if (n_triangles > RT_MAX_TRIANGLES) return fail(h, RT_ERR_CAPACITY, "more than 1375000 triangles");
    if (n_nodes > RT_MAX_NODES) return fail(h, RT_ERR_CAPACITY, "more than 2600000 BVH nodes");
    if (scene->spheres != n_spheres || scene->meshes != n_meshes)
        return fail(h, RT_ERR_INVALID_ARGUMENT, "SceneUniform counts disagree with the array lengths");
    HIP_TRY(h, hipSetDevice(h->device));

    try {
        SceneGeom g;
        InstanceFacts s;
        std::vector<rt2::Quad> head, tail;  // [0, lay.wide_off) and [lay.wide_off, lay.bytes) of the blob
        std::string why;
        int rc = rt2::pack_geometry(meshes, n_meshes, triangles, n_triangles, nodes, n_nodes, g, tail, why);
        if (rc == RT_OK) rc = rt2::pack_instances(h->opt.pack, g, spheres, n_spheres, meshes, n_meshes, s, head, why);
        if (rc != RT_OK) return fail(h, rc, why);
        const SceneLayout& lay = s.lay;
        std::vector<rt_mesh_uniform> inst_meshes(meshes, meshes + n_meshes);
        std::vector<rt_sphere> inst_spheres(spheres, spheres + n_spheres);
#if RT_WALK2
        free_dev(h->walk2);
        h->walk2 = nullptr;
        if (s.have_defer) {  // per internal node of the deferred mesh: its record, then copies of its children's records
            const uint32_t base = g.mesh[s.defer_mesh].wide_base;
            const rt2::Rec2* wide = reinterpret_cast<const rt2::Rec2*>(tail.data());  // (the tail starts with the wide records)
            std::vector<rt2::Rec2> w2((size_t)s.defer_internal * 3u, rt2::Rec2{});
            for (uint32_t k = 0; k < s.defer_internal; ++k) {
                w2[(size_t)k * 3] = wide[base + k];
                for (int c = 0; c < 2; ++c)
                    if (const rt2::Child ch = rt2::read_rec2(wide[base + k], c); ch.count == 0u) w2[(size_t)k * 3 + 1 + c] = wide[ch.idx];
            }
            HIP_TRY(h, hipMalloc((void**)&h->walk2, w2.size() * sizeof(rt2::Rec2)));
            HIP_TRY(h, hipMemcpy(h->walk2, w2.data(), w2.size() * sizeof(rt2::Rec2), hipMemcpyHostToDevice));
            h->walk2_base = base;
        }
#endif
        free_scene(h);
        HIP_TRY(h, hipMalloc((void**)&h->blob, lay.bytes));
        if ((uint64_t)lay.wide_off + tail.size() * sizeof(rt2::Quad) != lay.bytes)  // (an empty scene: 16 zero bytes)
            HIP_TRY(h, hipMemsetAsync(h->blob, 0, lay.bytes, h->stream));
        if (!head.empty())
            HIP_TRY(h, hipMemcpyAsync(h->blob, head.data(), head.size() * sizeof(rt2::Quad), hipMemcpyHostToDevice, h->stream));
        if (!tail.empty())
            HIP_TRY(h, hipMemcpyAsync((char*)h->blob + lay.wide_off, tail.data(), tail.size() * sizeof(rt2::Quad), hipMemcpyHostToDevice, h->stream));
#if RT_EXPERIMENTS
#include "experiments/rt_api_hybrid_blob.inl"   // (statement fragment: the small blob of the hybrid launches, from g, s, head, tail)
#endif
        HIP_TRY(h, hipStreamSynchronize(h->stream));  // host staging vectors die here
        h->geom = std::move(g);
        h->inst = s;
        h->terminal = rt2::terminal_skip_scene(head.data(), s.lay, s.n_items, n_meshes);
        commit_scene(h, scene->camera);
        h->inst_meshes.swap(inst_meshes);
        h->inst_spheres.swap(inst_spheres);
    } catch (const std::bad_alloc&) {
        return fail(h, RT_ERR_OUT_OF_MEMORY, "out of host memory");
    }
    return RT_OK;
}

int rt_update_instances(rt_handle* h, const rt_scene_uniform* scene, const rt_sphere* spheres, uint32_t n_spheres,
                        const rt_mesh_uniform* meshes, uint32_t n_meshes) {
    if (!h || !scene) return fail(h, RT_ERR_INVALID_ARGUMENT, "null handle or scene");
    if (!h->have_scene) return fail(h, RT_ERR_NO_SCENE, "rt_upload_scene has not been called");
    if ((n_spheres && !spheres) || (n_meshes && !meshes))
        return fail(h, RT_ERR_INVALID_ARGUMENT, "null array with non-zero count");
    if (n_spheres > RT_MAX_SPHERES) return fail(h, RT_ERR_CAPACITY, "more than 500 spheres");
    if (scene->spheres != n_spheres || scene->meshes != n_meshes)
        return fail(h, RT_ERR_INVALID_ARGUMENT, "SceneUniform counts disagree with the array lengths");
    const SceneGeom& g = h->geom;
    if (n_meshes != g.mesh.size())
        return fail(h, RT_ERR_INVALID_ARGUMENT, "mesh count " + std::to_string(n_meshes) + " differs from the uploaded " +
                                                    std::to_string(g.mesh.size()) + " (new geometry needs rt_upload_scene)");
    for (uint32_t i = 0; i < n_meshes; ++i)
        if (meshes[i].node_offset != g.mesh[i].node_offset || meshes[i].triangle_offset != g.mesh[i].triangle_offset ||
            meshes[i].triangles != g.mesh[i].triangles)
            return fail(h, RT_ERR_INVALID_ARGUMENT, "mesh " + std::to_string(i) +
                                                        ": node_offset / triangle_offset / triangles differ from the uploaded "
                                                        "scene (new geometry needs rt_upload_scene)");
#if RT_EXPERIMENTS || RT_WALK2
    // (the hybrid small blob and walk2 are derived from the head and the deferred mesh, which an update may change)
    return fail(h, RT_ERR_INVALID_ARGUMENT, "rt_update_instances is not available in the experiments build (its hybrid small "
                                            "blob and walk2 records derive from the head): use rt_upload_scene");
#endif
    HIP_TRY(h, hipSetDevice(h->device));
    try {
        InstanceFacts s;
        std::vector<rt2::Quad> head;
        std::string why;
        int rc = rt2::pack_instances(h->opt.pack, g, spheres, n_spheres, meshes, n_meshes, s, head, why);
        if (rc != RT_OK) return fail(h, rc, why);
        std::vector<rt_mesh_uniform> inst_meshes(meshes, meshes + n_meshes);
        std::vector<rt_sphere> inst_spheres(spheres, spheres + n_spheres);
        // The head in place -- after every launch that may read it, and complete before the next one -- or, when its size
        // changes, in a new blob: the old tail device to device, the new head from the host, the old blob freed after both.
        float4* target;
        if ((rc = blob_for_head(h, "rt_update_instances", s.lay, g.tail_bytes(), target)) != RT_OK) return rc;
        hipError_t e = head.empty() ? hipSuccess : hipMemcpyAsync(target, head.data(), head.size() * sizeof(rt2::Quad), hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);  // (host staging vector dies here)
        if (e != hipSuccess) return drop_new_blob(h, target, fail(h, RT_ERR_DEVICE, std::string("rt_update_instances: ") + hipGetErrorString(e)));
        adopt_blob(h, target);
        h->inst = s;
        h->terminal = rt2::terminal_skip_scene(head.data(), s.lay, s.n_items, n_meshes);  // (materials change in place)
        commit_scene(h, scene->camera);
        h->inst_meshes.swap(inst_meshes);
        h->inst_spheres.swap(inst_spheres);
        h->generation += 1;
    } catch (const std::bad_alloc&) {
        return fail(h, RT_ERR_OUT_OF_MEMORY, "out of host memory");
    }
    return RT_OK;
}

int rt_refit_bvh(const rt_mesh_uniform* meshes, uint32_t n_meshes, const rt_packed_triangle* triangles, uint32_t n_triangles,
                 rt_node* nodes, uint32_t n_nodes, uint32_t first, uint32_t n) {
    try {
        std::string err;
        const int rc = rt2::refit_bvh(meshes, n_meshes, triangles, n_triangles, nodes, n_nodes, first, n, err);
        return rc == RT_OK ? RT_OK : fail(nullptr, rc, err);
    } catch (const std::bad_alloc&) {
        return fail(nullptr, RT_ERR_OUT_OF_MEMORY, "out of host memory");
    }
}

// The device refit: validation and the scratch first, then the fit kernels, which write only the
// scratch; their per-mesh results (one small readback) feed the instance phase; only then, once nothing can be refused,
// the boxes and triangle records go into the blob -- the current one, or a resized one -- and the head is committed as
// rt_update_instances commits it.
int rt_refit_triangles(rt_handle* h, const rt_packed_triangle* triangles, uint32_t first, uint32_t n, int flags) {
    if (!h) return fail(h, RT_ERR_INVALID_ARGUMENT, "null handle");
    if (flags & ~RT_REFIT_HOST_MEMORY) return fail(h, RT_ERR_INVALID_ARGUMENT, "unknown flags");
    if (!h->have_scene) return fail(h, RT_ERR_NO_SCENE, "rt_upload_scene has not been called");
    const bool host = (flags & RT_REFIT_HOST_MEMORY) != 0;
    if (n && !triangles) return fail(h, RT_ERR_INVALID_ARGUMENT, "null triangles");
    if (n && !host && ((uintptr_t)triangles & 15u) != 0u)
        return fail(h, RT_ERR_INVALID_ARGUMENT, "device triangles not aligned (16 bytes)");
    const SceneGeom& g = h->geom;
    if ((uint64_t)first + n > g.n_triangles)
        return fail(h, RT_ERR_INVALID_ARGUMENT, "triangle range [" + std::to_string(first) + ", " + std::to_string((uint64_t)first + n) +
                                                    ") exceeds the " + std::to_string(g.n_triangles) + " uploaded triangles");
#if RT_EXPERIMENTS || RT_WALK2
    // (as rt_update_instances: the hybrid small blob and walk2 records derive from the head and the deferred mesh's records)
    return fail(h, RT_ERR_INVALID_ARGUMENT, "rt_refit_triangles is not available in the experiments build (its hybrid small "
                                            "blob and walk2 records derive from the scene): use rt_upload_scene");
#endif
    char* scratch = nullptr;
    auto done = [&](int rc) {  // (every exit once the scratch exists: nothing may still use it when it is freed)
        if (scratch) {
            (void)hipStreamSynchronize(h->stream);
            (void)hipFree(scratch);
            scratch = nullptr;
        }
        return rc;
    };
    try {
        // ---- the selection (rt_refit_bvh's rule, on the uploaded meshes' facts) and the slots ----
        std::vector<rt2::RefitSpan> spans(g.mesh.size());
        for (size_t i = 0; i < g.mesh.size(); ++i) {
            const MeshGeom& mg = g.mesh[i];
            spans[i] = rt2::RefitSpan{mg.tri_lo, mg.tri_hi, mg.node_lo, mg.node_hi, mg.triangle_offset};
        }
        std::vector<uint32_t> sel;
        std::string why;
        if (int rc = rt2::refit_select(spans, first, n, sel, why); rc != RT_OK) return fail(h, rc, why);
        std::vector<RefitMesh> table(sel.size());
        uint64_t slots = 0;
        for (size_t q = 0; q < sel.size(); ++q) {
            const MeshGeom& mg = g.mesh[sel[q]];
            RefitMesh& r = table[q];
            r.slot0 = (uint32_t)slots;
            r.wide_base = mg.wide_base;
            r.internal = mg.root_count ? 0u : mg.internal;
            r.root_idx = mg.root_idx;
            r.root_count = mg.root_count;
            slots += r.internal ? r.internal : 1u;
        }
        // ---- scratch: mesh table, results, parent links, arrival counters, boxes, staging of host triangles ----
        auto up = [](uint64_t b) { return (b + 255u) & ~(uint64_t)255u; };
        const uint64_t tab_b = up(table.size() * sizeof(RefitMesh)), res_b = up(table.size() * sizeof(RefitResult));
        const uint64_t par_b = up(slots * 4u), arr_b = up(slots * 4u), box_b = up(slots * 64u);
        const uint64_t stage_b = host ? up((uint64_t)n * sizeof(rt_packed_triangle)) : 0u;
        const uint64_t scratch_b = tab_b + res_b + par_b + arr_b + box_b + stage_b;
        if (!fits_cap(h, scratch_b))
            return fail(h, RT_ERR_OUT_OF_MEMORY, "option max_device_mb leaves no room for the refit's " +
                                                     std::to_string((scratch_b + (1u << 20) - 1) >> 20) + " MB of scratch");
        HIP_TRY(h, hipSetDevice(h->device));
        if (scratch_b && hipMalloc((void**)&scratch, scratch_b) != hipSuccess) {
            scratch = nullptr;
            (void)hipGetLastError();
            return fail(h, RT_ERR_OUT_OF_MEMORY, "rt_refit_triangles: no device memory for the scratch");
        }
        auto hip_fail = [&](const char* what, hipError_t e) {
            return done(fail(h, RT_ERR_DEVICE, std::string("rt_refit_triangles: ") + what + ": " + hipGetErrorString(e)));
        };
        RefitArgs a{};
        a.first = first;
        a.n = n;
        a.n_meshes = (uint32_t)table.size();
        a.slots = (uint32_t)slots;
        if (scratch) {
            a.meshes = reinterpret_cast<const RefitMesh*>(scratch);
            a.results = reinterpret_cast<RefitResult*>(scratch + tab_b);
            a.parent = reinterpret_cast<uint32_t*>(scratch + tab_b + res_b);
            a.arrivals = reinterpret_cast<uint32_t*>(scratch + tab_b + res_b + par_b);
            a.boxes = reinterpret_cast<unsigned long long*>(scratch + tab_b + res_b + par_b + arr_b);
        }
        a.tris = host ? (const void*)(scratch + tab_b + res_b + par_b + arr_b + box_b) : (const void*)triangles;
        hipError_t e = hipSuccess;
        std::vector<RefitResult> results(table.size());
        if (!table.empty()) {
            if ((e = hipMemcpyAsync((void*)a.meshes, table.data(), table.size() * sizeof(RefitMesh), hipMemcpyHostToDevice, h->stream)) != hipSuccess) return hip_fail("hipMemcpyAsync", e);
            if ((e = hipMemsetAsync(a.results, 0, res_b, h->stream)) != hipSuccess) return hip_fail("hipMemsetAsync", e);
            if ((e = hipMemsetAsync(a.parent, 0xff, par_b, h->stream)) != hipSuccess) return hip_fail("hipMemsetAsync", e);
            if ((e = hipMemsetAsync(a.arrivals, 0, arr_b, h->stream)) != hipSuccess) return hip_fail("hipMemsetAsync", e);
        }
        if (host && n && (e = hipMemcpyAsync((void*)a.tris, triangles, (size_t)n * sizeof(rt_packed_triangle), hipMemcpyHostToDevice, h->stream)) != hipSuccess)
            return hip_fail("hipMemcpyAsync", e);
        // ---- fit: the scratch only (the blob's wide records are read for their references, which a refit keeps) ----
        a.blob = h->blob;
        a.wide_off = h->inst.lay.wide_off;
        a.tri_off = h->inst.lay.tri_off;
        a.shade_off = h->inst.lay.shade_off;
        if ((e = launch_refit_fit(a, h->stream)) != hipSuccess) return hip_fail("launch_refit_fit", e);
        if (!table.empty() && (e = hipMemcpyAsync(results.data(), a.results, table.size() * sizeof(RefitResult), hipMemcpyDeviceToHost, h->stream)) != hipSuccess)
            return hip_fail("hipMemcpyAsync", e);
        if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return hip_fail("hipStreamSynchronize", e);
        // ---- the geometry facts of the refitted meshes, then the instance phase ----
        SceneGeom g2 = g;
        for (size_t q = 0; q < sel.size(); ++q) {
            const RefitResult& r = results[q];
            if ((r.flags & REFIT_DONE) == 0u || (r.flags & REFIT_BAD) != 0u)
                return done(fail(h, RT_ERR_DEVICE, "rt_refit_triangles: mesh " + std::to_string(sel[q]) +
                                                       ": the device refit did not reach its root (inconsistent BVH records)"));
            MeshGeom& mg = g2.mesh[sel[q]];
            for (int k = 0; k < 3; ++k) { mg.box_lo[k] = r.lo[k]; mg.box_hi[k] = r.hi[k]; }
            if (mg.root_count == 0) {
                mg.contains = (r.flags & REFIT_CONTAINS) != 0u;
                mg.unions = (r.flags & REFIT_UNIONS) != 0u;
            }
            mg.hierarchy_ok = !mg.deep && (r.flags & REFIT_IMPROPER) == 0u;
        }
        g2.roots_are_unions = true;
        for (const MeshGeom& mg : g2.mesh)
            if (mg.root_count == 0 && !mg.unions) g2.roots_are_unions = false;
        InstanceFacts s;
        std::vector<rt2::Quad> head;
        if (int rc = rt2::pack_instances(h->opt.pack, g2, h->inst_spheres.data(), (uint32_t)h->inst_spheres.size(), h->inst_meshes.data(),
                                         (uint32_t)h->inst_meshes.size(), s, head, why); rc != RT_OK)
            return done(fail(h, rc, why));
        // ---- write: from here on nothing is refused ----
        const SceneLayout& lay = s.lay;
        float4* target;  // (a resized head: a new blob, the old tail copied, then refitted there)
        if (int rc = blob_for_head(h, "rt_refit_triangles", lay, g2.tail_bytes(), target); rc != RT_OK) return done(rc);
        a.blob = target;
        a.wide_off = lay.wide_off;
        a.tri_off = lay.tri_off;
        a.shade_off = lay.shade_off;
        if ((e = launch_refit_write(a, h->stream)) != hipSuccess) return drop_new_blob(h, target, hip_fail("launch_refit_write", e));
        if (!head.empty() &&
            (e = hipMemcpyAsync(target, head.data(), head.size() * sizeof(rt2::Quad), hipMemcpyHostToDevice, h->stream)) != hipSuccess)
            return drop_new_blob(h, target, hip_fail("hipMemcpyAsync", e));
        if ((e = hipStreamSynchronize(h->stream)) != hipSuccess) return drop_new_blob(h, target, hip_fail("hipStreamSynchronize", e));
        adopt_blob(h, target);
        h->geom = std::move(g2);
        h->inst = s;
        h->terminal = rt2::terminal_skip_scene(head.data(), s.lay, s.n_items, (uint32_t)h->inst_meshes.size());
        commit_scene(h, h->camera);
        h->generation += 1;
        return done(RT_OK);
    } catch (const std::bad_alloc&) {
        return done(fail(h, RT_ERR_OUT_OF_MEMORY, "out of host memory"));
    }
}

// rt_render_multi (device-to-device transport): the root may still be copying this handle's previous frame out of
// h->image.  Everything that writes, rebinds or reads the image on the handle's stream waits for that copy first.
static int wait_pending_copy(rt_handle* h) {
    if (h->multi_copy_pending) {
        HIP_TRY(h, hipStreamWaitEvent(h->stream, h->multi_copied, 0));
        h->multi_copy_pending = false;
    }
    return RT_OK;
}

int rt_upload_textures(rt_handle* h, const rt_texture_desc* descs, uint32_t n) {
    if (!h || (n && !descs)) return fail(h, RT_ERR_INVALID_ARGUMENT, "null argument");
    h->generation += 1;
    if (n > RT_MAX_TEXTURES) return fail(h, RT_ERR_CAPACITY, "Cannot load more than 64 textures");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    free_textures(h);
    std::vector<DTexture> dt(n);
    for (uint32_t i = 0; i < n; ++i) {
        size_t bytes = (size_t)descs[i].width * descs[i].height * 4;
        uint8_t* p = nullptr;
        if (bytes) {
            if (!descs[i].rgba8) return fail(h, RT_ERR_INVALID_ARGUMENT, "texture without data");
            HIP_TRY(h, hipMalloc((void**)&p, bytes));
            h->texture_data.push_back(p);
            HIP_TRY(h, hipMemcpyAsync(p, descs[i].rgba8, bytes, hipMemcpyHostToDevice, h->stream));
        }
        dt[i] = DTexture{p, descs[i].width, descs[i].height};
    }
    int rc = upload(h, h->textures, dt.data(), dt.size());
    if (rc != RT_OK) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->n_textures = n;
    return RT_OK;
}

int rt_set_camera(rt_handle* h, const rt_camera_uniform* camera) {
    if (!h || !camera) return fail(h, RT_ERR_INVALID_ARGUMENT, "null argument");
    // (a host that re-sends the same camera every frame -- the reference's update_buffers -- keeps its frames rendered ahead)
    if (memcmp(&h->camera, camera, sizeof(rt_camera_uniform)) != 0) h->generation += 1;
    h->camera = *camera;
    return RT_OK;
}

int rt_set_option(rt_handle* h, const char* name, int value) {
    if (!h || !name) return RT_ERR_INVALID_ARGUMENT;
    h->generation += 1;  // (frames rendered ahead under the old setting are dropped: render_single)
    const rt2::SetResult r = rt2::set_option(h->opt, name, value);
    if (r.code() != RT_OK) return fail(h, r.code(), r.error);
    if (r.effects & rt2::OPT_DROPS_PRIMARY) invalidate_primary_tables(h);
    if (r.effects & rt2::OPT_RESETS_TILES) h->tiles.reset();
    if (r.effects & rt2::OPT_CLEARS_AHEAD_FAILED) h->ahead.try_again();
    return RT_OK;
}

int rt_set_counters(rt_handle* h, int enabled) {
    if (!h) return RT_ERR_INVALID_ARGUMENT;
    h->count_tests = enabled ? 1 : 0;
    h->generation += 1;
    return RT_OK;
}

uint64_t rt_strip_texels(uint32_t width, uint32_t height, uint32_t rank, uint32_t world) {
    if (world == 0 || rank >= world) return 0;
    uint32_t strips = (height + 7) / 8;
    uint32_t local = strips / world + (rank < strips % world ? 1 : 0);
    return (uint64_t)local * 8u * width;
}

// Sum of the recorded launch times (HIP events around every launch since rt_reset_timing).  The pairs are recorded on
// whichever stream the launch ran on -- the pipelined frames' internal streams too -- and synchronising the handle's
// stream only proves that the KERNELS before a pair's second event are done (the blends wait for them), not that the
// runtime has retired the event itself: every pair is synchronised before it is read (hipEventElapsedTime on an event
// that is not ready is hipErrorNotReady; seen once in 850 fuzz scenes with four frames in flight).
static hipError_t harvest_event_times(rt_handle* h, double& sum_ms) {
    for (size_t i = 0; i < h->ev_used; ++i) {
        hipError_t e = hipEventSynchronize(h->ev_pool[i].second);
        if (e != hipSuccess) return e;
        float ms = 0.0f;
        e = hipEventElapsedTime(&ms, h->ev_pool[i].first, h->ev_pool[i].second);
        if (e != hipSuccess) return e;
        sum_ms += ms;
    }
    return hipSuccess;
}

// The wavefront sequence's host side lives with the other measured-slower features: compiled with
// -DRT_EXPERIMENTS=1 only; the product build has the two stubs below and never sets WavefrontPlan::on.
struct WavefrontPlan { bool on = false; uint32_t frame_slots = 0; uint64_t slots = 0, rounds = 0; };
#if RT_EXPERIMENTS
#include "experiments/rt_api_wavefront.inl"
#else
static int wavefront_prepare(rt_handle*, const rt_params*, const RenderArgs&, uint32_t, uint32_t, WavefrontPlan&, bool&) { return RT_OK; }
static int wavefront_run(rt_handle*, const RenderArgs&, const WavefrontPlan&) { return RT_OK; }
#endif

// The scene- and option-dependent part of a launch's arguments: the scene, its item list and stack sizing, and which
// instantiation the kernels take (scene in LDS, many-mesh, SIMPLE).  render_impl launches with these, and so does the
// test library's per-ray probe (rt_test_intersect), which therefore walks exactly what a render walks.
static void scene_args(const rt_handle* h, RenderArgs& a) {
    a.blob = h->blob;
    a.lay = h->inst.lay;
    // (an explicitly requested deferred-walk sequence -- option "sort_rounds" > 0, tests -- reads the scene in place: the
    // parking instantiations exist for global-memory scenes only; the automatic setting never defers a mesh of a scene
    // that fits the LDS)
    a.lds_scene = (h->lds_scene && h->opt.lds_scene && !(h->opt.sort_rounds > 0 && h->inst.have_defer)) ? 1u : 0u;
    a.cull_roots = (h->geom.roots_are_unions && (h->opt.cull_roots == 1 || (h->opt.cull_roots < 0 && h->geom.mesh.size() >= 16))) ? 1u : 0u;
    a.many_mesh = (h->inst.has_tlas || (a.cull_roots && !h->inst.has_forest)) ? 1u : 0u;
    a.forest_cull = h->opt.cull_roots != 0 ? 1u : 0u;
    a.cross_prune = h->opt.cross_prune != 0 ? 1u : 0u;
    {
        uint32_t ds, dv;
        memcpy(&ds, &h->camera.defocus_strength, 4);
        memcpy(&dv, &h->camera.diverge_strength, 4);
        a.simple = (h->opt.specialise && h->inst.plain_materials && ds == 0u && dv == 0u) ? 1u : 0u;  // (both strengths +0)
    }
    a.textures = h->textures;
    a.srgb_lut = h->srgb_lut;
    a.n_meshes = (uint32_t)h->geom.mesh.size();
    a.n_spheres = (uint32_t)h->inst_spheres.size();
    a.n_textures = h->n_textures;
    a.stack_entries = h->stack_entries;
    a.tlas_entries = h->inst.tlas_entries;
    a.stack_wide = (h->stack_must_wide || (h->opt.stack_wide < 0 ? h->stack_wide : h->opt.stack_wide != 0)) ? 1u : 0u;
    // (the global-memory kernels park a pending mesh hit of 5 dwords in the stack column, intersect_scene)
    if (!a.lds_scene && a.stack_entries < (a.stack_wide ? 3u : 5u)) a.stack_entries = a.stack_wide ? 3u : 5u;
    a.n_items = h->inst.n_items;
}

// What the steps of one render_impl call decide and share.
struct LaunchPlan {
    FrameShape shape;
    uint32_t n_batch = 0;        // frames of the batch (0: a single frame)
    bool blend_later = false;    // (frames rendered ahead: the calls that ask for them blend them, render_single)
    uint64_t need_texels = 0;    // texels of this rank's share
    size_t park_records = 0, park_bytes = 0;  // deferred walks: records and bytes of ONE park queue
    uint32_t n_rounds = 0;       // how many rounds of deferred walks this launch would run (0: none)
    bool rounds = false;         // ... and whether it runs them
    WavefrontPlan wf;
    bool pipe = false;           // a pipelined single frame
    uint32_t pslot = 0;          // its pipeline slot
    hipStream_t S = nullptr;     // the stream this frame's sampling launch and its bookkeeping run on
    bool pipe_barrier = false;   // this frame rewrites shared tables (tile order, primary rays): the other stream's frame has to be done
    bool took_idle_path = false; // this frame would have been pipelined, found nothing in flight and takes the plain launch
    bool wrote_tables = false;   // this launch rewrites a table later launches read (tile order, tile costs, primary table)
    uint32_t n_tiles = 0;
    uint32_t tapered_head = 0;   // the frame group this launch takes if it carries a taper table (frame_groups; 0, 1: none)
    std::pair<hipEvent_t, hipEvent_t>* ev = nullptr;  // the launch's (start, stop) events
};

static int validate_and_shape(rt_handle* h, LaunchPlan& pl) {
    if (!h->have_scene) return fail(h, RT_ERR_NO_SCENE, "rt_upload_scene has not been called");
    if (pl.shape.world == 0 || pl.shape.rank >= pl.shape.world) return fail(h, RT_ERR_INVALID_ARGUMENT, "bad rank/world");
    if (pl.shape.width == 0 || pl.shape.height == 0) return fail(h, RT_ERR_INVALID_ARGUMENT, "empty image");
    pl.need_texels = pl.shape.texels();
    if (pl.need_texels > h->image_texels)
        return fail(h, RT_ERR_CAPACITY, "image larger than the bound image buffer");
    HIP_TRY(h, hipSetDevice(h->device));
    return wait_pending_copy(h);
}

static int prepare_batch_scratch(rt_handle* h, RenderArgs& a, const LaunchPlan& pl) {
    const uint32_t n_batch = pl.n_batch;
    if (!n_batch) return RT_OK;
    if (n_batch > RT_MAX_BATCH_FRAMES) return fail(h, RT_ERR_INVALID_ARGUMENT, "batch too large");
    const uint64_t scratch_stride = pl.need_texels;
    if (h->batch_scratch_texels < scratch_stride * n_batch) {
        // Room for the largest batch the options allow, not just this one: a later, larger batch of the same shape
        // (a warm-up of 5 frames, then 20) must not re-allocate -- a hipMalloc of hundreds of megabytes costs tens of
        // milliseconds -- in the middle of a host's frame sequence.
        const uint64_t slots = std::max<uint64_t>(n_batch, std::min<uint64_t>((uint64_t)h->opt.batch_frames, RT_MAX_BATCH_FRAMES));
        const size_t old_bytes = h->batch_scratch_texels * sizeof(float4);
        if (!fits_cap(h, scratch_stride * n_batch * sizeof(float4), old_bytes))
            return fail(h, RT_ERR_OUT_OF_MEMORY, "option max_device_mb leaves no room for the scratch images of this batch");
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        free_dev(h->batch_scratch);
        h->batch_scratch_texels = 0;
        if (fits_cap(h, scratch_stride * slots * sizeof(float4)) &&
            hipMalloc((void**)&h->batch_scratch, scratch_stride * slots * sizeof(float4)) == hipSuccess) {
            h->batch_scratch_texels = scratch_stride * slots;
        } else {   // (not that much memory: what this batch needs)
            (void)hipGetLastError();
            HIP_TRY(h, hipMalloc((void**)&h->batch_scratch, scratch_stride * n_batch * sizeof(float4)));
            h->batch_scratch_texels = scratch_stride * n_batch;
        }
        h->batch_zeroed = FrameShape{};  // (new memory: zero it below)
    }
    // The padding rows of a ragged last strip are never rendered: they must blend as zeros, not as the samples an
    // earlier batch of another shape left there.  Zero ALL of the scratch whenever the shape of its frames changes
    // (slot k of any later batch of this shape starts at k strides: the number of frames does not matter).
    if (h->batch_zeroed != pl.shape) {
        HIP_TRY(h, hipMemsetAsync(h->batch_scratch, 0, h->batch_scratch_texels * sizeof(float4), h->stream));
        h->batch_zeroed = pl.shape;
    }
    a.batch_frames = n_batch;
    a.batch_stride = scratch_stride;
    a.batch_tile_major = (uint32_t)h->opt.batch_tile_major;
    return RT_OK;
}

// the frame's constants: parameters, camera, the memo's ray origin, the blend weights, the reciprocal of the sample count
static void frame_constants(const rt_handle* h, const rt_params* params, RenderArgs& a) {
    a.params = *params;
    a.camera = h->camera;
    for (int k = 0; k < 3; ++k) {  // see pixel_cache_begin: the same IEEE operations, unfused
        volatile float rz = h->camera.cam_to_world[0][k] * 0.0f, uz = h->camera.cam_to_world[1][k] * 0.0f;
        volatile float t = h->camera.cam_to_world[3][k] + rz;
        a.memo_ro[k] = t + uz;
    }
    blend_weights(params->frames, a.blend_weight, a.blend_rest);
    {
        const int32_t n = params->rays_per_pixel;
        a.spp_reciprocal = (n > 0 && (n & (n - 1)) == 0) ? 1.0f / (float)n : 0.0f;
    }
}

// Which kernel runs and what its workgroups hold: the variant, the pixel memo's home, the LDS-staged tops of the
// experiments build, the persistent grid.
static int choose_kernel_shape(rt_handle* h, const rt_params* params, RenderArgs& a, const LaunchPlan& pl) {
    const uint32_t rank = pl.shape.rank, world = pl.shape.world, n_batch = pl.n_batch;
    scene_args(h, a);
    // the per-lane primary-ray cache is used when it still leaves room for 4 workgroups per CU
    a.image = n_batch ? h->batch_scratch : h->image;
    a.counters = h->counters;
    a.strip_rank = rank;
    a.strip_world = world;
    a.tiles_x = (params->width + 7) / 8;
    uint32_t strips = (params->height + 7) / 8;
    a.tiles_y = strips / world + (rank < strips % world ? 1 : 0);
    a.count_tests = (uint32_t)h->count_tests;
    a.kernel_variant = rt2::kernel_variant_for(h->opt, (uint64_t)a.tiles_x * a.tiles_y, n_batch, a.count_tests != 0u);
    // (all fields that size the LDS are set by now)
    a.pixel_cache = 0;
    a.pixel_cache_mem = nullptr;
    if (h->opt.pixel_cache == 1) {
        a.pixel_cache = 1;
        if (render_lds_bytes(a) > LDS_BUDGET_BYTES) a.pixel_cache = 0;  // no room in LDS
    }
    // LDS-staged top of the big mesh's BVH (global-memory scenes): as many of its breadth-first numbered
    // records as fit beside the stacks without costing a workgroup per CU, or what option "lds_top" says
    a.top_base = h->geom.top_mesh_base;
    a.top_count = 0;
    if (RT_EXPERIMENTS && !a.lds_scene && h->top_available && h->opt.lds_top != 0) {
        const size_t used = render_lds_bytes(a);
        uint32_t fit = used < LDS_BUDGET_BYTES ? (uint32_t)((LDS_BUDGET_BYTES - used) / WIDE_REC_BYTES) : 0u;
        if (h->opt.lds_top > 0) fit = (uint32_t)h->opt.lds_top;
        a.top_count = std::min(fit, h->top_available);
    }
    a.tlas_lds = 0;
    if (RT_EXPERIMENTS && !a.lds_scene && a.many_mesh && h->inst.has_tlas && h->opt.lds_tlas != 0 && params->debug_flag == 0) {
        // 1: as many of the breadth-first numbered records (the top levels first) as fit without costing a workgroup per
        // CU; 2: the whole tree if the LDS can hold it at all
        const size_t used = render_lds_bytes(a), need = (size_t)h->inst.n_tlas_records * WIDE_REC_BYTES;
        const uint32_t per_cu_now = rt2::blocks_per_cu_for(used);
        const size_t room = rt2::CU_LDS_BYTES / per_cu_now > used ? rt2::CU_LDS_BYTES / per_cu_now - used : 0;
        if (h->opt.lds_tlas == 2) {
            if (used + need <= 64u * 1024u) a.tlas_lds = h->inst.n_tlas_records;
        } else {
            a.tlas_lds = std::min<uint32_t>(h->inst.n_tlas_records, (uint32_t)(room / WIDE_REC_BYTES));
        }
    }
    a.persistent_blocks = rt2::persistent_blocks_for(h->opt, render_lds_bytes(a));
    const size_t memo_words = (size_t)h->opt.persistent_blocks * WAVES_PER_BLOCK * PIXEL_MEMO_DWORDS * 64u;
    if (h->opt.pixel_cache && a.pixel_cache == 0 && a.kernel_variant == 0 && params->debug_flag == 0 &&
        (h->pixel_cache_words >= memo_words || fits_cap(h, memo_words * sizeof(uint32_t), h->pixel_cache_words * sizeof(uint32_t)))) {
        // persistent kernel: a fixed number of waves, so the cache can live in global memory
        if (int rc = regrow(h, h->pixel_cache_mem, h->pixel_cache_words, memo_words, h->stream); rc != RT_OK) return rc;
        a.pixel_cache = 2;
        a.pixel_cache_mem = h->pixel_cache_mem;
    }
    a.fast_miss = h->opt.fast_miss != 0 && a.pixel_cache != 0u ? 1u : 0u;
    a.roulette_skip = h->opt.roulette_skip != 0 && a.pixel_cache != 0u ? 1u : 0u;
    // the terminal skip (rt2::terminal_skip_for; a parking launch of the product reads its scene from global memory)
    a.terminal_dark = rt2::terminal_skip_for(h->terminal, a.lds_scene != 0u, a.many_mesh != 0u, render_takes_simple(a), a.count_tests != 0u,
                                             RT_EXPERIMENTS && h->opt.hybrid != 0, h->terminal_skip_on);
    if (params->number_of_bounces >= (1 << 30)) a.terminal_dark = 0u;  // (the kernels borrow bit 30 of the segment number: PATH_TERMINAL)
    for (int k = 0; k < 3; ++k) a.terminal_c[k] = a.terminal_dark != 0u ? h->terminal.c[k] : 0.0f;
    return RT_OK;
}

// how many rounds of deferred walks this launch would run (0: none)
static void plan_rounds(const rt_handle* h, const rt_params* params, const RenderArgs& a, LaunchPlan& pl) {
    const size_t park_records = (size_t)pl.need_texels * (pl.n_batch ? pl.n_batch : 1u);
    const size_t park_bytes = ((park_records + 63) / 64) * (size_t)PARK_PLANES * 64u * sizeof(float4);  // per queue
    uint32_t n_rounds = h->opt.sort_rounds > 0 ? (uint32_t)h->opt.sort_rounds : 0u;
    if (h->opt.sort_rounds < 0 && h->inst.have_defer) {
        n_rounds = rt2::automatic_rounds(park_records, params->rays_per_pixel, h->inst.defer_internal);
        if (n_rounds && h->park_capacity < park_records) {
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || 2 * park_bytes > free_b / 2) n_rounds = 0;  // (both queues within half of what is free: 288 GB are there to be used)
            if (!fits_cap(h, 2 * park_bytes, 2 * (((h->park_capacity + 63) / 64) * (size_t)PARK_PLANES * 64u * sizeof(float4)))) n_rounds = 0;  // (option max_device_mb)
        }
    }
    pl.park_records = park_records;
    pl.park_bytes = park_bytes;
    pl.n_rounds = n_rounds;
    pl.rounds = n_rounds > 0 && h->inst.have_defer && a.many_mesh == 0 && a.kernel_variant == 0 && params->debug_flag == 0 &&
                params->rays_per_pixel > 0 && a.lds_scene == 0u;
}

// The intersection vote (path_begin): rt2::vote_thresholds.
static void vote_thresholds(const rt_handle* h, RenderArgs& a, const LaunchPlan& pl) {
    rt2::vote_thresholds(h->opt, pl.rounds, a.lds_scene == 0u || a.many_mesh != 0u, a.vote_eighths, a.vote_patience);
}

// Frames of a batch per work item (RenderArgs::frame_group): rt2::frame_group_for, for every launch that has a batch --
// rt_render_frames, its strips, the frames rendered ahead.  This is the size of a launch without a taper table;
// pl.tapered_head is the longer head (rt2::frame_group_tapered_for) that tile_feedback gives the launch once it knows
// that the launch carries a table written for that head.
static void frame_groups(rt_handle* h, RenderArgs& a, LaunchPlan& pl) {
    // (`costly` as for the vote; the one-wave-per-tile kernel and a launch without samples take no groups either)
    const bool tile_major = a.batch_tile_major != 0u;
    const bool costly = a.lds_scene == 0u || a.many_mesh != 0u || a.kernel_variant != 0u || a.params.rays_per_pixel <= 0;
    uint32_t g = rt2::frame_group_for(pl.n_batch, (uint64_t)a.tiles_x * a.tiles_y, a.persistent_blocks * WAVES_PER_BLOCK, tile_major, pl.rounds,
                                      costly);
    uint32_t head = RT_FRAME_TAPER != 0 ? rt2::frame_group_tapered_for(pl.n_batch, (uint64_t)a.tiles_x * a.tiles_y,
                                                                       a.persistent_blocks * WAVES_PER_BLOCK, tile_major, pl.rounds, costly)
                                        : 0u;
    // (a forced size -- the test library's -- stands in for the caps and the item floors only)
    if (h->frame_group_forced != 0u && rt2::FRAME_GROUP_CAP > 1u &&
        rt2::frame_group_for(pl.n_batch, ~0ull, 1u, tile_major, pl.rounds, costly) > 1u)
        g = head = std::min(h->frame_group_forced, pl.n_batch);
    a.frame_group = h->last_frame_group = g;
    pl.tapered_head = head;
}

// Pipelined single frames: a plain one-frame launch (no batch, no sequence of launches).
// S is the stream this frame's sampling launch and its bookkeeping run on.
static int pipeline_acquire(rt_handle* h, const rt_params* params, const RenderArgs& a, LaunchPlan& pl) {
    const uint64_t need_texels = pl.need_texels;
    const bool wavefront_wanted = RT_EXPERIMENTS && h->opt.wavefront != 0 && a.many_mesh != 0 && !h->geom.any_deep && params->debug_flag == 0 && params->rays_per_pixel > 0;
    const int pipeline_opt = rt2::pipeline_depth(h->opt, hw_queues_requested(), pl.shape.world);
    if (!h->queues_noted && pipeline_opt != 0 && (hw_queues_requested() < 5 || pipeline_opt + 1 > hw_queues_requested())) {
        // Not an error, said once (rt_last_error after a call that returned RT_OK): the pipeline is limited by, or
        // oversubscribes, the hardware queues the host asked the runtime for.
        h->queues_noted = true;
        h->err = "note: GPU_MAX_HW_QUEUES is " + std::to_string(hw_queues_requested()) + " (read when the first handle was created): " +
                 (h->opt.pipeline < 0 ? "the frame pipeline runs " + std::to_string(pipeline_opt) + " frames deep instead of 4"
                                  : "option pipeline = " + std::to_string(pipeline_opt) + " needs " + std::to_string(pipeline_opt + 1) + " queues, its streams will share queues and serialise") +
                 "; export GPU_MAX_HW_QUEUES=8 (12 for strip shares of >= 4 ranks) before the HIP runtime initialises (INTEGRATION.md section 3)";
    }
    const uint32_t pipe_depth = pipeline_opt >= 2 ? (uint32_t)pipeline_opt : 2u;
    bool pipe = pipeline_opt != 0 && pl.n_batch == 0 && params->debug_flag == 0 && params->rays_per_pixel > 0 &&
                !pl.rounds && !wavefront_wanted;   // (strips too: the gather reads the image behind the blend, on the handle's stream)
    if (pipe && h->pipe_scratch_texels < need_texels) {   // (option max_device_mb: the pipeline's scratch images have to fit)
        size_t held = 0;
        for (const PipeSlot& ps : h->pipe) if (ps.scratch) held += h->pipe_scratch_texels * sizeof(float4);
        if (!fits_cap(h, (size_t)pipe_depth * need_texels * sizeof(float4), held)) pipe = false;
    } else if (pipe) {
        uint32_t have = 0;
        for (uint32_t k = 0; k < pipe_depth; ++k) have += h->pipe[k].scratch ? 1u : 0u;
        if (!fits_cap(h, (size_t)(pipe_depth - have) * h->pipe_scratch_texels * sizeof(float4))) pipe = false;
    }
    if (pipe && h->opt.pipeline_when_idle == 0) {
        // Every pipelined frame ends with its blend on the handle's stream: an idle stream means no frame is in flight,
        // i.e. this frame has nothing to overlap with (yet).  It takes the plain launch; the frames a host issues while
        // this one runs are pipelined behind it.
        const hipError_t q = hipStreamQuery(h->stream);
        (void)hipGetLastError();  // (hipErrorNotReady is an answer, not a failure: do not leave it for the launchers' hipGetLastError)
        if (q == hipSuccess) { pipe = false; pl.took_idle_path = true; }
        else if (q != hipErrorNotReady) return fail(h, RT_ERR_DEVICE, std::string("hipStreamQuery: ") + hipGetErrorString(q));
    }
    pl.pipe = pipe;
    pl.pslot = h->pipe_seq % pipe_depth;
    pl.S = h->stream;
    if (!pipe) return RT_OK;
    PipeSlot& slot = h->pipe[pl.pslot];
    h->pipe_seq = (h->pipe_seq + 1) % 840u;   // (a multiple of every depth)
    for (uint32_t k = 0; k < pipe_depth; ++k)   // (no more streams than frames in flight: they share the process's hardware queues)
        if (int rc = pipe_slot_create(h, h->pipe[k]); rc != RT_OK) return rc;
    if (!h->pipe_book) HIP_TRY(h, hipEventCreateWithFlags(&h->pipe_book, hipEventDisableTiming));
    if (!h->pipe_main) HIP_TRY(h, hipEventCreateWithFlags(&h->pipe_main, hipEventDisableTiming));
    if (h->pipe_scratch_texels < need_texels) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));   // (the blends on this stream wait for every sampling launch)
        for (PipeSlot& ps : h->pipe) {
            free_dev(ps.scratch);
            ps.blended_set = false;
        }
        h->pipe_scratch_texels = need_texels;
    }
    if (!slot.scratch) {
        HIP_TRY(h, hipMalloc((void**)&slot.scratch, h->pipe_scratch_texels * sizeof(float4)));
        slot.zeroed = FrameShape{};  // (nothing zeroed yet)
    }
    const hipStream_t S = pl.S = slot.stream;
    // this frame's scratch image is free once the frame before last has been blended out of it; the tables the last
    // bookkeeping frame rewrote are complete; whatever the handle's stream did outside the pipeline is complete
    if (slot.blended_set) HIP_TRY(h, hipStreamWaitEvent(S, slot.blended, 0));
    // The blend covers all need_texels, the sampling launch writes the pixels of the frame only: the padding rows of
    // a ragged last strip (world > 1, height % 8 != 0) must blend as zeros, as in the batch path -- a fresh
    // allocation, or samples an earlier frame of another shape left there, would otherwise reach the strip
    // buffer's padding rows (the assembled frame never reads them).
    if (slot.zeroed != pl.shape) {
        HIP_TRY(h, hipMemsetAsync(slot.scratch, 0, need_texels * sizeof(float4), S));
        slot.zeroed = pl.shape;
    }
    if (h->pipe_book_set) HIP_TRY(h, hipStreamWaitEvent(S, h->pipe_book, 0));
    // (not for a frame that took the plain launch because nothing was in flight and rewrote no table: the host SAW the
    // stream idle before it, so everything older is complete; this frame's samples go to a scratch image, and its blend
    // follows that launch in the handle's stream's order anyway -- so the second frame of a burst overlaps the first)
    if (h->pipe_main_set && h->pipe_main_need) HIP_TRY(h, hipStreamWaitEvent(S, h->pipe_main, 0));
    return RT_OK;
}

// before rewriting a shared table: the other stream's sampling launch is done
static hipError_t barrier_other(rt_handle* h, LaunchPlan& pl) {
    pl.wrote_tables = true;
    if (!pl.pipe || pl.pipe_barrier) return hipSuccess;
    pl.pipe_barrier = true;
    if (h->pipe_main_set) {   // (... and whatever the handle's stream last launched outside the pipeline)
        const hipError_t e = hipStreamWaitEvent(pl.S, h->pipe_main, 0);
        if (e != hipSuccess) return e;
    }
    for (uint32_t k = 0; k < rt2::PIPE_MAX; ++k)
        if (k != pl.pslot && h->pipe[k].sampled_set) {
            const hipError_t e = hipStreamWaitEvent(pl.S, h->pipe[k].sampled, 0);
            if (e != hipSuccess) return e;
        }
    return hipSuccess;
}

// does the table serve (camera, shape, with / without hits) as it stands?
static bool primary_table_serves(const PrimaryTable& t, size_t texels, const rt_camera_uniform& camera, const FrameShape& shape,
                                 bool want_hits) {
    return t.table && t.texels >= texels && t.valid && t.shape == shape && (!want_hits || t.with_hits) &&
           memcmp(&t.camera, &camera, sizeof(rt_camera_uniform)) == 0;
}

// Makes the table serve (the handle's camera, shape, with / without hits) on `stream`: grown if it is too small,
// recomputed, marked.  The caller's business, because it is what differs between the shared table and a slot's own: whoever
// may still read a table that has to grow has been synchronised, and barrier_other() before a table that other streams'
// frames read is rewritten.
static int primary_table_make(rt_handle* h, RenderArgs& a, PrimaryTable& t, size_t texels, const FrameShape& shape, bool want_hits,
                              hipStream_t stream) {
    if (t.texels < texels) {
        t.valid = false;
        if (int rc = replace_dev(h, &t.table, t.texels, texels, 64); rc != RT_OK) return rc;
    }
    a.primary = nullptr;
    HIP_TRY(h, launch_primary(a, t.table, want_hits, stream));
    t.valid = true;
    t.shape = shape;
    t.with_hits = want_hits;
    t.camera = h->camera;
    return RT_OK;
}

// Primary-ray table for the memo: which one, and whether it is recomputed first, is rt2::choose_primary's decision
// (host/launch_state.h) over the facts gathered here
static int bind_primary_table(rt_handle* h, const rt_params* params, RenderArgs& a, LaunchPlan& pl) {
    a.primary = nullptr;
    a.primary_complete = 0u;
    rt2::PrimaryFacts f;
    f.primary_table = h->opt.primary_table, f.primary_hits = h->opt.primary_hits, f.primary_per_slot = h->opt.primary_per_slot;
    f.camera_moved = h->last_sampled.valid && memcmp(&h->last_sampled.camera, &h->camera, sizeof(rt_camera_uniform)) != 0;
    if (params->debug_flag == 0 && params->rays_per_pixel > 0) h->last_sampled.sampled(h->camera);
    f.n_batch = pl.n_batch, f.pipelined = pl.pipe, f.pixel_cache = a.pixel_cache, f.count_tests = a.count_tests;
    f.debug_flag = params->debug_flag, f.rays_per_pixel = params->rays_per_pixel;
    const size_t texels = (size_t)((params->width + 7) / 8) * ((params->height + 7) / 8) * 64;  // whole 8x8 tiles
    const bool want_hits = rt2::primary_wants_hits(h->opt.primary_hits, a.count_tests);
    auto facts = [&](const PrimaryTable& t) {  // (option max_device_mb: may a table that is too small be replaced by one that is not?)
        const bool large_enough = t.texels >= texels;
        return rt2::TableFacts{primary_table_serves(t, texels, h->camera, pl.shape, want_hits), large_enough,
                               large_enough || fits_cap(h, texels * 64u, t.texels * 64u)};
    };
    PrimaryTable& own = h->pipe[pl.pslot].primary;
    f.shared = facts(h->primary), f.own = facts(own);
    const rt2::PrimaryChoice c = rt2::choose_primary(f);
    if (c.table == rt2::PrimaryChoice::NONE) return RT_OK;
    PrimaryTable& t = c.table == rt2::PrimaryChoice::OWN ? own : h->primary;
    if (c.rebuild) {
        if (c.sync == rt2::PrimaryChoice::SLOT_STREAM) HIP_TRY(h, hipStreamSynchronize(pl.S));
        if (c.sync == rt2::PrimaryChoice::DRAIN_STREAMS)
            if (int rc = drain_streams(h); rc != RT_OK) return rc;
        if (c.barrier) HIP_TRY(h, barrier_other(h, pl));
        if (int rc = primary_table_make(h, a, t, texels, pl.shape, c.want_hits, pl.S); rc != RT_OK) return rc;
    }
    a.primary = t.table;
    a.primary_complete = t.with_hits ? 1u : 0u;
    return RT_OK;
}

static int bind_memo(rt_handle* h, RenderArgs& a, const LaunchPlan& pl) {
    // With a complete table a lane's memo EQUALS its table entry for the pixel's whole life: the kernels whose memo has no
    // room in LDS read the entry in place (pixel_cache = 4) instead of copying it into a buffer in global memory --
    // that copy was most of what the global-memory kernels wrote and half of what they read.
    if (a.pixel_cache == 2u && a.lds_scene == 0u && a.primary != nullptr && a.primary_complete != 0u && h->opt.memo_in_table != 0) {
        a.pixel_cache = 4u;
        a.pixel_cache_mem = nullptr;
    }
    // The global-memory memo is per resident wave and stateful across a pixel's samples: one per concurrent launch.
    // Slot 0 has its own too -- a plain launch on the handle's stream (pixel_cache_mem) may still be running beside
    // the pipelined frame of slot 0 when pipe_main_need is false (a frame that found the stream idle).
    if (pl.pipe && a.pixel_cache == 2u) {
        PipeSlot& slot = h->pipe[pl.pslot];
        const size_t need = (size_t)h->opt.persistent_blocks * WAVES_PER_BLOCK * PIXEL_MEMO_DWORDS * 64u;
        if (int rc = regrow(h, slot.memo, slot.memo_words, need, h->stream); rc != RT_OK) return rc;
        a.pixel_cache_mem = slot.memo;
    }
    return RT_OK;
}

// the two park queues (an automatic sequence that cannot have them falls back to the plain launch)
static int prepare_park_queues(rt_handle* h, LaunchPlan& pl) {
    if (!pl.rounds || h->park_capacity >= pl.park_records) return RT_OK;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    free_dev(h->park_queue[0]);
    free_dev(h->park_queue[1]);
    h->park_capacity = 0;
    const hipError_t e0 = hipMalloc((void**)&h->park_queue[0], pl.park_bytes);
    const hipError_t e1 = e0 == hipSuccess ? hipMalloc((void**)&h->park_queue[1], pl.park_bytes) : e0;
    if (e1 != hipSuccess) {
        (void)hipGetLastError();
        free_dev(h->park_queue[0]);
        free_dev(h->park_queue[1]);
        if (h->opt.sort_rounds > 0) return fail(h, RT_ERR_OUT_OF_MEMORY, "sort_rounds: no device memory for the park queues");
        pl.rounds = false;
    } else {
        h->park_capacity = pl.park_records;
    }
    return RT_OK;
}

// Tile-cost feedback (persistent kernel, path-trace frames only): the tiles are handed out in the order of the rays each
// took in an earlier frame of the same shape, heaviest first.  rt2::TileSchedule (host/launch_state.h) says when the order
// and its taper table are rewritten, whether this launch uses them, and when it records costs; this step does that.
static int tile_feedback(rt_handle* h, const rt_params* params, RenderArgs& a, LaunchPlan& pl) {
    const uint32_t n_tiles = pl.n_tiles;
    rt2::TileLaunch l;
    l.shape = pl.shape, l.n_batch = pl.n_batch, l.tapered_head = pl.tapered_head;
    l.period = h->opt.tile_feedback_period, l.taper_buffer = h->frame_taper != nullptr;
    l.applies = h->opt.tile_feedback && params->debug_flag == 0 && n_tiles <= h->tile_capacity && n_tiles > 0 && a.kernel_variant == 0;
    const rt2::TileDecision d = h->tiles.step(l);
    const auto act = [&]() -> int {
        if (d.rewrite_order) {
            const long long per_tile = 64ll * (params->rays_per_pixel > 0 ? params->rays_per_pixel : 0) *
                                       (params->number_of_bounces >= 0 ? params->number_of_bounces + 1 : 0);
            const uint32_t max_cost = per_tile > 0xffffffffll ? 0xffffffffu : (uint32_t)per_tile;
            HIP_TRY(h, barrier_other(h, pl));
            HIP_TRY(h, launch_tile_order(h->tile_cost[d.order_from], n_tiles, max_cost, h->tile_order, pl.S));
            // (the taper's floor: segments that a complete primary table serves are counted as rays and cost next to nothing)
            if (d.write_taper) {
                const long long served = a.primary_complete != 0u ? 64ll * params->rays_per_pixel : 0ll;
                HIP_TRY(h, launch_frame_taper(h->tile_cost[d.order_from], n_tiles, max_cost, served > 0xffffffffll ? 0xffffffffu : (uint32_t)served,
                                              pl.n_batch, pl.tapered_head, a.persistent_blocks * WAVES_PER_BLOCK, rt2::FRAME_TAPER_ALPHA,
                                              h->frame_taper, pl.S));
            }
        }
        if (d.use_order) a.tile_order = h->tile_order;
        if (d.take_head) {
            a.frame_group = h->last_frame_group = pl.tapered_head;
            a.frame_taper = h->frame_taper;
        }
        if (d.record_costs) {
            a.tile_cost = h->tile_cost[d.record_into];
            pl.wrote_tables = true;
            HIP_TRY(h, hipMemsetAsync(a.tile_cost, 0, (size_t)n_tiles * sizeof(uint32_t), pl.S));
        }
        return RT_OK;
    };
    const int rc = act();
    if (rc != RT_OK) h->tiles.reset();  // (the schedule counts on what was not done: it starts over)
    return rc;
}

// Test-only (rt_test_frame_taper): the forced segments as this launch's table, in place of the rule's -- for a launch that
// takes groups at all (frame_groups).  The items are counted here, for this batch's frames and this launch's tiles; a
// first rank past the tiles gives an empty segment.
static int forced_taper(rt_handle* h, RenderArgs& a, const LaunchPlan& pl) {
    if (RT_FRAME_TAPER != 0 && a.frame_group > 1u && !h->taper_forced.empty() && h->frame_taper) {
        uint32_t table[rt2::TAPER_WORDS] = {};
        const uint32_t segments = (uint32_t)h->taper_forced.size() / 2u;
        uint32_t item = 0;
        for (uint32_t k = 0; k < segments; ++k) {
            const uint32_t rank = std::min(h->taper_forced[2 * k], pl.n_tiles), g = h->taper_forced[2 * k + 1];
            const uint32_t next = k + 1 < segments ? std::min(h->taper_forced[2 * k + 2], pl.n_tiles) : pl.n_tiles;
            uint32_t* seg = table + rt2::TAPER_HEAD_WORDS + 3 * k;
            seg[0] = rank;
            seg[1] = g;
            seg[2] = item;
            item += (next - rank) * ((pl.n_batch + g - 1u) / g);
        }
        table[0] = segments;
        table[1] = item;
        table[2] = pl.n_batch;
        table[3] = a.frame_group;
        HIP_TRY(h, hipStreamSynchronize(h->stream));  // (an earlier batch may still read the table)
        HIP_TRY(h, hipMemcpy(h->frame_taper + rt2::TAPER_WORDS, table, sizeof(table), hipMemcpyHostToDevice));
        a.frame_taper = h->frame_taper + rt2::TAPER_WORDS;
    }
    h->last_taper = a.frame_group > 1u ? a.frame_taper : nullptr;  // (the slot is q_out's in a launch that parks)
    return RT_OK;
}

// the launch's pair of timing events, out of the pool
static int timing_events(rt_handle* h, LaunchPlan& pl) {
    if (h->ev_used == h->ev_pool.size()) {
        if (h->ev_pool.size() >= 4096) {
            // the pool is full: add the recorded times to the running total, then reuse the events
            HIP_TRY(h, harvest_event_times(h, h->ev_ms_harvested));
            h->ev_used = 0;
        } else {
            hipEvent_t s0 = nullptr, s1 = nullptr;
            HIP_TRY(h, hipEventCreate(&s0));
            HIP_TRY(h, hipEventCreate(&s1));
            h->ev_pool.emplace_back(s0, s1);
        }
    }
    pl.ev = &h->ev_pool[h->ev_used++];
    return RT_OK;
}

// what rt_last_launch reports
static void note_launch(rt_handle* h, const rt_params* params, const RenderArgs& a, const LaunchPlan& pl) {
    const uint32_t tile_blocks = (pl.n_tiles + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    h->last_launch[0] = (uint32_t)render_lds_bytes(a);
    h->last_launch[1] = a.kernel_variant == 1 || params->debug_flag != 0 ? tile_blocks : std::min(a.persistent_blocks, tile_blocks);
    h->last_launch[2] = a.lds_scene;
    h->last_launch[3] = (a.many_mesh ? 1u : 0u) | (render_takes_simple(a) ? 2u : 0u) |
                        (a.kernel_variant == 1 ? 4u : 0u) | (pl.rounds ? 8u : 0u) |
                        (h->fixed_switches_on && render_takes_fixed(a) ? 32u : 0u);
    h->last_terminal_dark = params->debug_flag != 0 ? 0u : a.terminal_dark;
}

// Blend n frames of `texels` texels each out of `scratch` into the image, in frame order on the handle's stream:
// wgsl:157-158 per frame, each with the weights of its own frame number (the host's two operations, as in a one-frame launch)
static int blend_frames(rt_handle* h, const float4* scratch, uint64_t texels, uint32_t n, int32_t frames0) {
    BlendArgs b{};
    b.image = h->image;
    b.scratch = scratch;
    b.texels = texels;
    b.stride = texels;
    b.n = n;
    b.frames0 = frames0;
    for (uint32_t k = 0; k < n; ++k) blend_weights((int32_t)((uint32_t)frames0 + k), b.weight[k], b.rest[k]);
    HIP_TRY(h, launch_blend_frames(b, h->stream));
    return RT_OK;
}

// sample into this slot's scratch image on its stream; blend in frame order on the handle's stream
static int launch_pipelined(rt_handle* h, const rt_params* params, RenderArgs& a, const LaunchPlan& pl) {
    PipeSlot& slot = h->pipe[pl.pslot];
    a.image = slot.scratch;
    a.batch_frames = 1;
    a.batch_stride = pl.need_texels;
    a.batch_tile_major = 0;
    HIP_TRY(h, launch_render(a, pl.S, h->fixed_switches_on));
    HIP_TRY(h, hipEventRecord(slot.sampled, pl.S));
    slot.sampled_set = true;
    HIP_TRY(h, hipEventRecord(pl.ev->second, pl.S));
    HIP_TRY(h, hipStreamWaitEvent(h->stream, slot.sampled, 0));
    if (int rc = blend_frames(h, slot.scratch, pl.need_texels, 1, params->frames); rc != RT_OK) return rc;
    HIP_TRY(h, hipEventRecord(slot.blended, h->stream));
    slot.blended_set = true;
    return RT_OK;
}

// launch 0 takes the tiles and parks every pixel in front of its first entry into the big mesh; then, round
// after round, rt_walk_kernel walks the mesh for the parked rays and a render launch resumes those pixels
// (parking them again at their next entry); the last render launch does not park: it walks what is left
// inline.  Everything is ordered on the stream; a launch whose queue is empty ends at once.
static int launch_rounds(rt_handle* h, RenderArgs& a, const LaunchPlan& pl) {
    if (!h->park_counts) HIP_TRY(h, hipMalloc((void**)&h->park_counts, 72 * sizeof(uint32_t)));
    HIP_TRY(h, hipMemsetAsync(h->park_counts, 0, 72 * sizeof(uint32_t), h->stream));
    a.defer_mesh = h->inst.defer_mesh;
    a.defer_xform = h->inst.defer_xform;
#if RT_WALK2
    a.walk2 = h->walk2;
    a.walk2_base = h->walk2_base;
#endif
    const uint32_t R = pl.n_rounds;
    a.park = 1;
    a.park_levels = (uint32_t)h->opt.park_levels;
    a.q_in = nullptr;
    a.q_in_count = nullptr;
    a.q_out = h->park_queue[0];
    a.q_out_count = h->park_counts;
    // Hybrid launches: the render launches that PARK never walk the big mesh, so they run the LDS-scene kernels on
    // the small blob (everything but the big mesh's BVH and triangles) with the small meshes' stack depth; a winner on
    // the big mesh reads its shading record from the full blob.  The last launch (park = 0) and rt_walk_kernel
    // read the full blob as before.
    RenderArgs ah = a;
    bool hybrid = RT_EXPERIMENTS && h->opt.hybrid != 0 && h->small_ok && !a.lds_scene && a.count_tests == 0 && a.kernel_variant == 0;
    if (hybrid) {
        ah.blob = h->small_blob;
        ah.lay = h->small_lay;
        ah.lds_scene = 1;
        ah.hybrid = 1;
        ah.big_blob = h->blob;
        ah.big_shade_off = h->inst.lay.shade_off;
        ah.top_count = 0;
        ah.stack_entries = h->small_stack_entries ? h->small_stack_entries : 1u;
        ah.stack_wide = 0;
        ah.pixel_cache = h->opt.pixel_cache ? 1u : 0u;
        if (ah.pixel_cache && render_lds_bytes(ah) > LDS_BUDGET_BYTES) {
            // (the global-memory memo buffer; the plain launches may read theirs in place from the table -- pixel_cache 4 --,
            // which the LDS-scene kernels of the hybrid launches have not compiled in: a parked pixel's memo is rebuilt from
            // the table on resume either way, RenderArgs::primary_complete)
            ah.pixel_cache = (a.pixel_cache == 2u || a.pixel_cache == 4u) && h->pixel_cache_mem ? 2u : 0u;
            ah.pixel_cache_mem = h->pixel_cache_mem;
        }
        if (!ah.pixel_cache) ah.primary = nullptr;
        ah.fast_miss = h->opt.fast_miss != 0 && ah.pixel_cache != 0u ? 1u : 0u;
        ah.roulette_skip = h->opt.roulette_skip != 0 && ah.pixel_cache != 0u ? 1u : 0u;
        if (render_lds_bytes(ah) > LDS_BUDGET_BYTES) hybrid = false;
        ah.persistent_blocks = (uint32_t)h->opt.persistent_blocks;
        ah.park_levels = 0;  // (the small blob has no record of the big mesh's BVH)
    }
    if (!hybrid) ah = a;
    auto sync_queues = [&]() {  // (the queue fields move with the rounds: keep the hybrid copy's in step)
        ah.park = a.park; ah.q_in = a.q_in; ah.q_in_count = a.q_in_count; ah.q_out = a.q_out; ah.q_out_count = a.q_out_count;
        ah.work_counter = a.work_counter; ah.defer_mesh = a.defer_mesh; ah.defer_xform = a.defer_xform;
    };
    sync_queues();
    HIP_TRY(h, launch_render(ah, h->stream, h->fixed_switches_on));
    for (uint32_t r = 0; r < R; ++r) {
        const bool last = r + 1 == R;
        a.q_in = h->park_queue[r & 1u];
        a.q_in_count = h->park_counts + r;
        HIP_TRY(h, h->work.next(h->stream, a.work_counter));
        {
            RenderArgs w = a;
            w.top_count = 0;  // (nothing is staged into the walk kernel's LDS)
            HIP_TRY(h, launch_walk(w, h->compute_units, h->stream));
        }
        HIP_TRY(h, h->work.next(h->stream, a.work_counter));
        a.park = last ? 0u : 1u;
        a.q_out = last ? nullptr : h->park_queue[(r + 1) & 1u];
        a.q_out_count = last ? nullptr : h->park_counts + r + 1;
        sync_queues();
        HIP_TRY(h, launch_render(last ? a : ah, h->stream, h->fixed_switches_on));
    }
    return RT_OK;
}

// what rt_get_stats reports
static void account_launch(rt_handle* h, const rt_params* params, const LaunchPlan& pl) {
    const uint32_t n_batch = pl.n_batch;
    h->launches_total += 1;
    if (!pl.blend_later) h->ahead.launched(n_batch ? n_batch : 1u);  // (frames rendered ahead: render_single reports them)
    if (params->debug_flag == 0 && params->rays_per_pixel > 0) {
        // pixels this call renders (strips are clipped to the image height)
        unsigned long long rows = 0;
        for (uint32_t st = pl.shape.rank; st < (params->height + 7) / 8; st += pl.shape.world) {
            uint32_t y0 = st * 8, y1 = y0 + 8 < params->height ? y0 + 8 : params->height;
            rows += y1 - y0;
        }
        h->paths_total += rows * params->width * (unsigned long long)params->rays_per_pixel * (n_batch ? n_batch : 1u);
    }
}

// One launch of the hot path: a single frame (n_batch == 0: wgsl `main`, blending in place), or a batch
// of n_batch >= 2 consecutive frames (Params.frames advancing by one each, app.rs:44-53) sampled in one
// persistent launch over (frame, tile) work items and blended in frame order by a dense second kernel.
// The steps run in this order; each is the function of that name above.
static int render_impl(rt_handle* h, const rt_params* params, uint32_t rank, uint32_t world, uint32_t n_batch = 0,
                       bool blend_later = false) {
    if (!h || !params) return fail(h, RT_ERR_INVALID_ARGUMENT, "null argument");
    h->ahead.broken();  // (whatever launches here breaks a sequence of frames rendered ahead: render_single)
    LaunchPlan pl;
    pl.shape = FrameShape{params->width, params->height, rank, world};
    pl.n_batch = n_batch;
    pl.blend_later = blend_later;
    RenderArgs a{};
    int rc;
    if ((rc = validate_and_shape(h, pl)) != RT_OK) return rc;
    if ((rc = prepare_batch_scratch(h, a, pl)) != RT_OK) return rc;
    frame_constants(h, params, a);
    if ((rc = choose_kernel_shape(h, params, a, pl)) != RT_OK) return rc;
    plan_rounds(h, params, a, pl);
    vote_thresholds(h, a, pl);
    frame_groups(h, a, pl);
    if ((rc = pipeline_acquire(h, params, a, pl)) != RT_OK) return rc;
    if ((rc = bind_primary_table(h, params, a, pl)) != RT_OK) return rc;
    if ((rc = bind_memo(h, a, pl)) != RT_OK) return rc;
    // (a ring per pipe stream: its memset only touches launches of its own, in-order stream)
    HIP_TRY(h, (pl.pipe ? h->pipe[pl.pslot].work : h->work).next(pl.S, a.work_counter));
    pl.n_tiles = a.tiles_x * a.tiles_y;
    a.tile_order = nullptr;
    a.tile_cost = nullptr;
    // Wavefront sequence (option "wavefront", experiments build only: experiments/rt_api_wavefront.inl)
    if ((rc = wavefront_prepare(h, params, a, pl.n_tiles, n_batch, pl.wf, pl.rounds)) != RT_OK) return rc;
    if ((rc = prepare_park_queues(h, pl)) != RT_OK) return rc;
    if ((rc = tile_feedback(h, params, a, pl)) != RT_OK) return rc;
    if ((rc = forced_taper(h, a, pl)) != RT_OK) return rc;
    if ((rc = timing_events(h, pl)) != RT_OK) return rc;
    note_launch(h, params, a, pl);
    if (pl.pipe && pl.pipe_barrier) {   // the tables this frame rewrote: later frames of the other stream wait for them
        HIP_TRY(h, hipEventRecord(h->pipe_book, pl.S));
        h->pipe_book_set = true;
    }
    HIP_TRY(h, hipEventRecord(pl.ev->first, pl.S));
    if (pl.wf.on) rc = wavefront_run(h, a, pl.wf);
    else if (pl.pipe) rc = launch_pipelined(h, params, a, pl);
    else if (pl.rounds) rc = launch_rounds(h, a, pl);
    else HIP_TRY(h, launch_render(a, h->stream, h->fixed_switches_on));
    if (rc != RT_OK) return rc;
    if (n_batch && !blend_later && (rc = blend_frames(h, h->batch_scratch, pl.need_texels, n_batch, params->frames)) != RT_OK) return rc;
    if (!pl.pipe) {
        HIP_TRY(h, hipEventRecord(pl.ev->second, h->stream));
        if (h->pipe[0].stream) {   // (pipelined frames may follow: their streams wait for this launch)
            HIP_TRY(h, hipEventRecord(h->pipe_main, h->stream));
            h->pipe_main_set = true;
            h->pipe_main_need = !(pl.took_idle_path && !pl.wrote_tables);
        }
    }
    account_launch(h, params, pl);
    return RT_OK;
}

// n consecutive frames; batches of "batch_frames" frames per launch.  Debug views, single frames and
// frames without samples take the one-frame path (nothing to overlap).
static int render_single(rt_handle* h, const rt_params* params, uint32_t rank, uint32_t world);
static int render_frames_impl(rt_handle* h, const rt_params* params, uint32_t n_frames, uint32_t rank, uint32_t world) {
    if (!h || !params) return fail(h, RT_ERR_INVALID_ARGUMENT, "null argument");
    if (n_frames == 1) return render_single(h, params, rank, world);  // (one frame per call: rt_render's path)
    rt_params p = *params;
    uint32_t done = 0;
    uint32_t cap = (uint32_t)h->opt.batch_frames;
    if (h->opt.max_device_mb != 0 && world != 0 && rank < world) {   // (option max_device_mb: as many scratch frames as fit; 1 = plain launches)
        const uint64_t texels = FrameShape{params->width, params->height, rank, world}.texels();
        const size_t other = optional_bytes(h) - h->batch_scratch_texels * sizeof(float4);
        const size_t room = h->opt.max_device_bytes() > other ? h->opt.max_device_bytes() - other : 0;
        const uint64_t fit = texels ? room / (texels * sizeof(float4)) : cap;
        if (fit < cap) cap = fit >= 2 ? (uint32_t)fit : 1u;
    }
    const uint32_t per = rt2::equal_batch(n_frames, cap);
    while (done < n_frames) {
        uint32_t n = n_frames - done;
        if (n > per) n = per;
        if (params->debug_flag != 0 || params->rays_per_pixel <= 0) n = 1;
        p.frames = (int32_t)((uint32_t)params->frames + done);
        const int rc = render_impl(h, &p, rank, world, n >= 2 ? n : 0u);
        if (rc != RT_OK) return rc;
        done += n;
    }
    return RT_OK;
}

// ---- one frame per call, frames rendered ahead (option "frame_ahead"; the sequence: rt2::AheadSequence) ---------------
// blend slot `slot` of the frames rendered ahead into the image: wgsl:157-158 with the frame's own weight
static int blend_ahead_slot(rt_handle* h, uint32_t slot, int32_t frames) {
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = wait_pending_copy(h); rc != RT_OK) return rc;
    if (int rc = blend_frames(h, h->batch_scratch + (size_t)slot * h->ahead.texels, h->ahead.texels, 1, frames); rc != RT_OK) return rc;
    if (h->pipe[0].stream) {  // (pipelined frames may follow: their blends are ordered behind this one)
        HIP_TRY(h, hipEventRecord(h->pipe_main, h->stream));
        h->pipe_main_set = true;
        h->pipe_main_need = true;
    }
    return RT_OK;
}

static int render_single(rt_handle* h, const rt_params* params, uint32_t rank, uint32_t world) {
    if (!h || !params) return fail(h, RT_ERR_INVALID_ARGUMENT, "null argument");
    const rt2::FrameCall call{*params, rank, world, h->generation};
    const rt2::AheadStep step = h->ahead.one_frame_call(call);
    if (step.slot >= 0) {
        const int rc = blend_ahead_slot(h, (uint32_t)step.slot, params->frames);
        if (rc == RT_OK) h->ahead.served(call);
        else h->ahead.broken();
        return rc;
    }
    if (step.continues && h->have_scene && world != 0 && rank < world && params->width != 0 && params->height != 0) {
        const uint64_t need_texels = FrameShape{params->width, params->height, rank, world}.texels();
        const bool automatic = h->opt.frame_ahead < 0;
        // (a host that WAITS for its frames finds the stream idle; one that runs ahead of the device finds it busy)
        const bool host_waits = automatic && !(hipSetDevice(h->device) == hipSuccess && hipStreamQuery(h->stream) == hipErrorNotReady);
        (void)hipGetLastError();  // (hipErrorNotReady is an answer, not a failure: not for the launchers' hipGetLastError)
        const uint32_t full = rt2::ahead_depth(h->opt, *params, h->count_tests != 0, h->ahead.failed_once, h->lds_scene, need_texels, host_waits);
        if (automatic && full >= 2) {
            // (room for the full depth at once: the batches on the way up would each re-allocate the scratch images -- a
            // stream synchronisation apiece)
            if (h->batch_scratch_texels < need_texels * full && fits_cap(h, need_texels * full * sizeof(float4), h->batch_scratch_texels * sizeof(float4)) &&
                hipSetDevice(h->device) == hipSuccess && hipStreamSynchronize(h->stream) == hipSuccess) {
                float4* bigger = nullptr;
                if (hipMalloc((void**)&bigger, need_texels * full * sizeof(float4)) == hipSuccess) {
                    free_dev(h->batch_scratch);
                    h->batch_scratch = bigger;
                    h->batch_scratch_texels = need_texels * full;
                    h->batch_zeroed = FrameShape{};  // (new memory: render_impl zeroes it)
                } else {
                    (void)hipGetLastError();
                }
            }
        }
        const uint32_t d = h->ahead.start_depth(full, automatic);
        if (d >= 2 && need_texels <= h->image_texels) {
            int rc = render_impl(h, params, rank, world, d, true);
            if (rc == RT_OK) {
                h->ahead.began(call, d, need_texels);
                rc = blend_ahead_slot(h, 0, params->frames);
                if (rc == RT_OK) h->ahead.remember(call);
                else h->ahead.broken();
                return rc;
            }
            h->ahead.failed(automatic);  // (no room for the batch: this handle renders its frames one by one from now on)
            (void)hipGetLastError();
        }
    }
    const int rc = render_impl(h, params, rank, world);
    if (rc == RT_OK) h->ahead.remember(call);
    else h->ahead.forget();
    return rc;
}

int rt_render(rt_handle* h, const rt_params* params) { return render_single(h, params, 0, 1); }

int rt_render_frames(rt_handle* h, const rt_params* params, uint32_t n_frames) {
    return render_frames_impl(h, params, n_frames, 0, 1);
}

int rt_render_strips(rt_handle* h, const rt_params* params, uint32_t rank, uint32_t world) {
    return render_single(h, params, rank, world);
}

int rt_render_strips_frames(rt_handle* h, const rt_params* params, uint32_t n_frames, uint32_t rank, uint32_t world) {
    return render_frames_impl(h, params, n_frames, rank, world);
}

int rt_assemble_strips(rt_handle* h, const void* gathered_device, uint32_t width, uint32_t height, uint32_t world) {
    if (!h || !gathered_device || world == 0) return fail(h, RT_ERR_INVALID_ARGUMENT, "bad arguments");
    if ((uint64_t)width * height > h->image_texels)
        return fail(h, RT_ERR_CAPACITY, "image larger than the bound image buffer");
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = wait_pending_copy(h); rc != RT_OK) return rc;
    unsigned long long pad = rt_strip_texels(width, height, 0, world);
    HIP_TRY(h, launch_assemble((const float4*)gathered_device, h->image, width, height, world, pad, h->stream));
    return RT_OK;
}

// ---- multi-GPU frame in one process ------------------------------------------------------------
// Gather transport between distinct devices: RCCL (grouped ncclSend / ncclRecv = a gather: every peer
// sends over its own xGMI link to the root), loaded on first use -- librccl is ~570 MB and no other
// entry point needs it.
static int render_multi_impl(rt_handle** per_gpu, int n_gpus, const rt_params* params, uint32_t n_frames,
                             float* rgba32f_out) {
    if (!per_gpu || n_gpus < 1 || !params) return RT_ERR_INVALID_ARGUMENT;
    for (int r = 0; r < n_gpus; ++r)
        if (!per_gpu[r]) return RT_ERR_INVALID_ARGUMENT;
    rt_handle* root = per_gpu[0];
    if (n_frames == 0) return RT_OK;
    const uint32_t world = (uint32_t)n_gpus;
    const uint64_t pad = rt_strip_texels(params->width, params->height, 0, world);
    const uint64_t frame_texels = (uint64_t)params->width * params->height;
    // transport: RCCL between distinct devices (option "multi_rccl" = 1, default), device-to-device
    // copies when several handles share a device (tests) or when the option is 0; 2 forces RCCL on a
    // one-handle "node" (exercises the RCCL path on a single-GPU box)
    bool distinct = true;
    for (int r = 0; r < n_gpus; ++r)
        for (int q = 0; q < r; ++q)
            if (per_gpu[r]->device == per_gpu[q]->device) distinct = false;
    bool use_rccl = distinct && ((root->opt.multi_rccl == 1 && n_gpus > 1) || root->opt.multi_rccl == 2);
    if (root->opt.multi_rccl == 2 && !distinct)
        return fail(root, RT_ERR_INVALID_ARGUMENT, "multi_rccl = 2 (RCCL always) needs one device per handle: a communicator cannot "
                                                   "hold two ranks of one device (multi_rccl = 1 uses device-to-device copies there)");
    // root-side staging, grown on demand
    HIP_TRY(root, hipSetDevice(root->device));
    if (int rc = regrow(root, root->multi_gathered, root->multi_gathered_texels, pad * world, root->stream); rc != RT_OK) return rc;
    if (int rc = regrow(root, root->multi_frame, root->multi_frame_texels, frame_texels, root->stream); rc != RT_OK) return rc;
    for (int r = 0; r < n_gpus; ++r) {  // every rank's "the root has copied my strips" event: of the root's device
        rt_handle* h = per_gpu[r];
        if (h->multi_copied && h->multi_copied_device == root->device) continue;
        if (h->multi_copied) {
            if (h->multi_copy_pending) (void)hipEventSynchronize(h->multi_copied);
            h->multi_copy_pending = false;
            (void)hipEventDestroy(h->multi_copied);
            h->multi_copied = nullptr;
        }
        HIP_TRY(root, hipEventCreateWithFlags(&h->multi_copied, hipEventDisableTiming));
        h->multi_copied_device = root->device;
    }
    if (use_rccl) {
        std::vector<int> devs(n_gpus);
        for (int r = 0; r < n_gpus; ++r) devs[r] = per_gpu[r]->device;
        if (root->multi_comm_devices != devs) {
            // Automatic mode (multi_rccl = 1) falls back to device-to-device copies when librccl cannot be loaded or
            // the communicators cannot be made (the reason stays in rt_last_error); multi_rccl = 2 insists.
            std::string why;
            if (!g_rccl.load()) {
                why = g_rccl.why;
            } else {
                multi_drop_comms(root);
                std::vector<ncclComm_t> comms(n_gpus);
                const ncclResult_t r = g_rccl.CommInitAll(comms.data(), n_gpus, devs.data());
                if (r != ncclSuccess) {
                    why = std::string("ncclCommInitAll: ") + g_rccl.GetErrorString(r);
                } else {
                    for (ncclComm_t c : comms) root->multi_comms.push_back((void*)c);
                    root->multi_comm_devices = devs;
                }
            }
            if (!why.empty()) {
                if (root->opt.multi_rccl == 2) return fail(root, RT_ERR_DEVICE, why + " (option multi_rccl = 0 selects device-to-device copies)");
                root->err = "rt_render_multi: " + why + "; gathering with device-to-device copies instead";
                root->opt.multi_rccl = 0;  // (do not try again on every frame)
                use_rccl = false;
            }
        }
    }
    if (!use_rccl) {
        // peer access for the device-to-device copies (without it the runtime stages them through the host)
        for (int r = 1; r < n_gpus; ++r) {
            const int peer = per_gpu[r]->device;
            if (peer == root->device || root->multi_peers_enabled.count(peer)) continue;
            int can = 0;
            HIP_TRY(root, hipDeviceCanAccessPeer(&can, root->device, peer));
            if (can) {
                hipError_t e = hipDeviceEnablePeerAccess(peer, 0);
                if (e == hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
                else if (e != hipSuccess) return fail(root, RT_ERR_DEVICE, std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e));
            }
            root->multi_peers_enabled.insert(peer);
        }
    }
    // 1. every GPU renders its strips (asynchronous, in parallel across devices).  render_impl makes a
    //    rank's stream wait until the root has finished copying that rank's previous frame.
    for (int r = 0; r < n_gpus; ++r) {
        int rc = render_frames_impl(per_gpu[r], params, n_frames, (uint32_t)r, world);
        if (rc != RT_OK) {
            if (per_gpu[r] != root) root->err = "rank " + std::to_string(r) + ": " + per_gpu[r]->err;
            return rc;
        }
    }
    // 2. gather: one transfer per rank into the root's [world][pad] buffer
    auto rank_texels = [&](int r) {  // (world == 1: the "strips" are the frame itself, no padding of a ragged last strip)
        return FrameShape{params->width, params->height, (uint32_t)r, world}.texels();
    };
    if (use_rccl) {
        std::vector<GatherLeg> legs;
        for (int r = 0; r < n_gpus; ++r) {
            rt_handle* h = per_gpu[r];
            legs.push_back(GatherLeg{h->image, root->multi_gathered + (size_t)r * pad, (size_t)rank_texels(r) * 4, r, h->device,
                                     (ncclComm_t)root->multi_comms[r], h->stream});
        }
        auto set_device = [](int device, std::string& err) {
            const hipError_t e = hipSetDevice(device);
            if (e != hipSuccess && err.empty()) err = std::string("hipSetDevice: ") + hipGetErrorString(e);
            return e == hipSuccess ? 0 : 1;
        };
        std::string gerr;
        if (!rccl_grouped_gather(g_rccl, legs, root->device, (ncclComm_t)root->multi_comms[0], root->stream, set_device, gerr)) {
            // the group has been closed (rt_rccl.h); a half-issued gather may have left a send without its receive on
            // a stream: the communicators are aborted and made again by the next call
            multi_drop_comms(root, true);
            return fail(root, RT_ERR_DEVICE, "rt_render_multi gather: " + gerr);
        }
        // (a rank's send is ordered on its own stream before its next render: no extra event needed)
    } else {
        for (int r = 0; r < n_gpus; ++r) {
            rt_handle* h = per_gpu[r];
            const uint64_t n = rank_texels(r);
            if (n == 0) continue;
            HIP_TRY(h, hipSetDevice(h->device));
            if (!h->multi_event) HIP_TRY(h, hipEventCreateWithFlags(&h->multi_event, hipEventDisableTiming));
            HIP_TRY(h, hipEventRecord(h->multi_event, h->stream));
            HIP_TRY(root, hipSetDevice(root->device));
            HIP_TRY(root, hipStreamWaitEvent(root->stream, h->multi_event, 0));
            if (h->device == root->device)
                HIP_TRY(root, hipMemcpyAsync(root->multi_gathered + (size_t)r * pad, h->image, n * sizeof(float4),
                                             hipMemcpyDeviceToDevice, root->stream));
            else
                HIP_TRY(root, hipMemcpyPeerAsync(root->multi_gathered + (size_t)r * pad, root->device, h->image, h->device,
                                                 n * sizeof(float4), root->stream));
            if (h->stream != root->stream) {
                // the rank's next render overwrites h->image: it has to wait for this copy
                HIP_TRY(root, hipEventRecord(h->multi_copied, root->stream));
                h->multi_copy_pending = true;
            }
        }
    }
    // 3. assemble on the root and (optionally) read back
    HIP_TRY(root, hipSetDevice(root->device));
    HIP_TRY(root, launch_assemble(root->multi_gathered, root->multi_frame, params->width, params->height, world, pad,
                                  root->stream));
    if (rgba32f_out) {
        HIP_TRY(root, hipMemcpyAsync(rgba32f_out, root->multi_frame, frame_texels * sizeof(float4),
                                     hipMemcpyDeviceToHost, root->stream));
        HIP_TRY(root, hipStreamSynchronize(root->stream));
    }
    return RT_OK;
}

int rt_render_multi(rt_handle** per_gpu, int n_gpus, const rt_params* params, float* rgba32f_out) {
    return render_multi_impl(per_gpu, n_gpus, params, 1, rgba32f_out);
}

int rt_render_multi_frames(rt_handle** per_gpu, int n_gpus, const rt_params* params, uint32_t n_frames, float* rgba32f_out) {
    return render_multi_impl(per_gpu, n_gpus, params, n_frames, rgba32f_out);
}

int rt_read_multi_frame(rt_handle* root, float* rgba32f_out, size_t bytes) {
    if (!root || !rgba32f_out) return fail(root, RT_ERR_INVALID_ARGUMENT, "null argument");
    if (!root->multi_frame || bytes > root->multi_frame_texels * sizeof(float4))
        return fail(root, RT_ERR_INVALID_ARGUMENT, "no assembled frame of that size");
    HIP_TRY(root, hipSetDevice(root->device));
    HIP_TRY(root, hipMemcpyAsync(rgba32f_out, root->multi_frame, bytes, hipMemcpyDeviceToHost, root->stream));
    HIP_TRY(root, hipStreamSynchronize(root->stream));
    return RT_OK;
}

// ---- ray queries (include/rt_abi.h: rt_intersect_rays, rt_occluded_rays, rt_pick; rt_queries.inl: rt_query_kernel) ----
// A query launch takes the arguments a render of the scene takes (scene_args), no pixel memo, and the render's
// persistent grid (workgroups that fit the CUs' LDS).  It reads nothing but the scene and writes nothing but its output:
// the image, the tables, the pipeline slots and the counters are not touched.
static_assert(sizeof(rt_ray) == 32 && sizeof(rt_hit) == 64, "rt_ray / rt_hit layout");

// The arguments of a launch on the scene outside a render (queries, rt_pick, rt_render_gbuffer, the test probe): what a
// render of the scene takes (scene_args), the handle's camera, and the caller's frame parameters or none.
static RenderArgs query_args(const rt_handle* h, const rt_params* params) {
    RenderArgs a{};
    scene_args(h, a);
    a.params = params ? *params : rt_params{};
    a.camera = h->camera;
    return a;
}

// Device memory a host-memory call may stage through: at most 64 MB, within what option max_device_mb leaves.
static size_t staging_room(const rt_handle* h) {
    size_t room = (size_t)64 << 20;
    if (h->opt.max_device_mb != 0) {
        const size_t held = optional_bytes(h);
        room = std::min(room, h->opt.max_device_bytes() > held ? h->opt.max_device_bytes() - held : 0);
    }
    return room;
}

// The loop of a host-memory call (the ray queries, rt_render_gbuffer, rt_radiance_rays): one temporary device buffer of
// `bytes` (what_for: its name in the out-of-memory message), then step(buf, i0, m, what) for the chunks [i0, i0 + m) of the
// call's n items.  A step queues its chunk's copies and launch on the handle's stream; when one of them fails it names it in
// `what` and returns its error.  The stream is drained after every chunk -- the buffer is used again, and the results are on
// the host when the call returns -- and before the buffer is freed, whatever happened.
extern "C++" {
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
}  // extern "C++" (a template among the C entry points)

// out_bytes: bytes of output per ray (sizeof(rt_hit) or 4)
static int query_impl(rt_handle* h, const rt_ray* rays, uint64_t n, void* out, size_t out_bytes, int flags, bool any) {
    if (!h) return fail(h, RT_ERR_INVALID_ARGUMENT, "null handle");
    const int known = RT_QUERY_HOST_MEMORY | (any ? RT_QUERY_PRUNE_TMAX : 0);
    if (flags & ~known) return fail(h, RT_ERR_INVALID_ARGUMENT, "unknown flags");
    if (n == 0) return RT_OK;
    if (!rays || !out) return fail(h, RT_ERR_INVALID_ARGUMENT, "null argument");
    if (n > 0x7fffffffull) return fail(h, RT_ERR_CAPACITY, "more than 2^31 - 1 rays");
    if (!h->have_scene) return fail(h, RT_ERR_NO_SCENE, "rt_upload_scene has not been called");
    const bool host = (flags & RT_QUERY_HOST_MEMORY) != 0, prune = (flags & RT_QUERY_PRUNE_TMAX) != 0;
    if (!host && (((uintptr_t)rays & 15u) != 0u || ((uintptr_t)out & (out_bytes == 4 ? 3u : 15u)) != 0u))
        return fail(h, RT_ERR_INVALID_ARGUMENT, "device rays / results not aligned (16 bytes; 4 for occlusion flags)");
    HIP_TRY(h, hipSetDevice(h->device));
    const RenderArgs a = query_args(h, nullptr);
    const uint32_t blocks = rt2::persistent_blocks_for(h->opt, render_lds_bytes(a));
    if (!host) {
        HIP_TRY(h, launch_query(a, rays, n, out, any, prune, blocks, h->compute_units, h->stream));
        return RT_OK;
    }
    // host memory: chunks of at most 64 MB of device memory (rays, then results), within option max_device_mb
    const size_t per_ray = sizeof(rt_ray) + out_bytes;
    const uint64_t chunk = std::min<uint64_t>(n, staging_room(h) / per_ray);
    if (chunk == 0) return fail(h, RT_ERR_OUT_OF_MEMORY, "option max_device_mb leaves no room for a query's staging buffers");
    return staged_chunks(h, chunk * per_ray, n, chunk, "a query's staging buffers", [&](uint8_t* buf, uint64_t i0, uint64_t m, const char*& what) {
        uint8_t* d_out = buf + chunk * sizeof(rt_ray);
        hipError_t e = hipSuccess;
        if (what = "hipMemcpyAsync", (e = hipMemcpyAsync(buf, rays + i0, m * sizeof(rt_ray), hipMemcpyHostToDevice, h->stream)) != hipSuccess) return e;
        if (what = "launch_query", (e = launch_query(a, buf, m, d_out, any, prune, blocks, h->compute_units, h->stream)) != hipSuccess) return e;
        what = "hipMemcpyAsync";
        return hipMemcpyAsync(static_cast<uint8_t*>(out) + i0 * out_bytes, d_out, m * out_bytes, hipMemcpyDeviceToHost, h->stream);
    });
}

int rt_intersect_rays(rt_handle* h, const rt_ray* rays, uint64_t n, rt_hit* hits, int flags) {
    return query_impl(h, rays, n, hits, sizeof(rt_hit), flags, false);
}

int rt_occluded_rays(rt_handle* h, const rt_ray* rays, uint64_t n, uint32_t* occluded, int flags) {
    return query_impl(h, rays, n, occluded, sizeof(uint32_t), flags, true);
}

int rt_pick(rt_handle* h, const rt_params* params, uint32_t x, uint32_t y, rt_hit* hit) {
    if (!h || !params || !hit) return fail(h, RT_ERR_INVALID_ARGUMENT, "null argument");
    if (x >= params->width || y >= params->height) return fail(h, RT_ERR_INVALID_ARGUMENT, "texel outside the frame");
    if (!h->have_scene) return fail(h, RT_ERR_NO_SCENE, "rt_upload_scene has not been called");
    HIP_TRY(h, hipSetDevice(h->device));
    const RenderArgs a = query_args(h, params);
    float4* d = nullptr;  // one rt_ray, then one rt_hit
    HIP_TRY(h, hipMalloc((void**)&d, sizeof(rt_ray) + sizeof(rt_hit)));
    hipError_t e = launch_pick_ray(a, x, y, d, h->stream);
    if (e == hipSuccess) e = launch_query(a, d, 1, d + 2, false, false, 1, 1, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(hit, d + 2, sizeof(rt_hit), hipMemcpyDeviceToHost, h->stream);
    const hipError_t e2 = hipStreamSynchronize(h->stream);
    free_dev(d);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return fail(h, RT_ERR_DEVICE, std::string("rt_pick: ") + hipGetErrorString(e));
    return RT_OK;
}

// ---- first-hit buffers of a frame (include/rt_abi.h: rt_render_gbuffer; rt_queries.inl: rt_gbuffer_kernel) ----
// Launched like a query: the arguments a render of the scene takes, nothing read but the scene and nothing written but
// the caller's planes.
int rt_render_gbuffer(rt_handle* h, const rt_params* params, const rt_gbuffer* out, int flags) {
    if (!h || !params || !out) return fail(h, RT_ERR_INVALID_ARGUMENT, "null argument");
    if (out->struct_bytes != sizeof(rt_gbuffer)) return fail(h, RT_ERR_INVALID_ARGUMENT, "rt_gbuffer.struct_bytes is not sizeof(rt_gbuffer)");
    if (out->_p0 != 0u) return fail(h, RT_ERR_INVALID_ARGUMENT, "rt_gbuffer._p0 must be 0");
    if (flags & ~RT_GBUFFER_HOST_MEMORY) return fail(h, RT_ERR_INVALID_ARGUMENT, "unknown flags");
    const uint32_t W = params->width, H = params->height;
    if (W == 0u || H == 0u) return fail(h, RT_ERR_INVALID_ARGUMENT, "zero width or height");
    if ((uint64_t)W * H > 0x7fffffffull) return fail(h, RT_ERR_CAPACITY, "more than 2^31 - 1 texels");
    // the planes in struct order: pointer, bytes per texel, alignment of a device pointer
    void* const ptr[11] = {out->depth, out->dir, out->point, out->normal, out->bary, out->texcoord, out->albedo, out->emission,
                           out->object, out->primitive, out->flags};
    static const uint32_t bytes[11] = {4, 12, 12, 12, 8, 8, 16, 16, 4, 4, 1}, align[11] = {4, 4, 4, 4, 4, 4, 16, 16, 4, 4, 1};
    static const char* const names[11] = {"depth", "dir", "point", "normal", "bary", "texcoord", "albedo", "emission", "object",
                                          "primitive", "flags"};
    size_t per_texel = 0;
    for (int c = 0; c < 11; ++c) per_texel += ptr[c] ? bytes[c] : 0u;
    if (per_texel == 0) return RT_OK;   // no plane asked for
    if (!h->have_scene) return fail(h, RT_ERR_NO_SCENE, "rt_upload_scene has not been called");
    const bool host = (flags & RT_GBUFFER_HOST_MEMORY) != 0;
    if (!host)
        for (int c = 0; c < 11; ++c)
            if (ptr[c] && ((uintptr_t)ptr[c] & (align[c] - 1u)) != 0u)
                return fail(h, RT_ERR_INVALID_ARGUMENT, std::string("device plane ") + names[c] + " is not aligned to " + std::to_string(align[c]) + " bytes");
    HIP_TRY(h, hipSetDevice(h->device));
    RenderArgs a = query_args(h, nullptr);
    a.params.width = W;
    a.params.height = H;
    GBufferArgs g{};
    g.width = W;
    g.height = H;
    auto bind = [&](void* const p[11]) {
        g.depth = (float*)p[0]; g.dir = (float*)p[1]; g.point = (float*)p[2]; g.normal = (float*)p[3]; g.bary = (float*)p[4];
        g.texcoord = (float*)p[5]; g.albedo = (float4*)p[6]; g.emission = (float4*)p[7]; g.object = (uint32_t*)p[8];
        g.primitive = (uint32_t*)p[9]; g.flags = (uint8_t*)p[10];
    };
    if (!host) {
        g.row0 = 0;
        g.rows = H;
        bind(ptr);
        HIP_TRY(h, launch_gbuffer(a, g, h->stream));
        return RT_OK;
    }
    // host memory: bands of whole rows through one temporary device buffer of at most 64 MB, within option max_device_mb;
    // each plane's part of it starts at a multiple of 256 bytes (11 x 256 bytes of slack at most)
    const size_t slack = 11u * 256u, room = staging_room(h);
    const size_t row_bytes = (size_t)W * per_texel;
    const uint32_t band = room > slack ? (uint32_t)std::min<uint64_t>(H, (room - slack) / row_bytes) : 0u;
    if (band == 0u) return fail(h, RT_ERR_OUT_OF_MEMORY, "option max_device_mb leaves no room for one row of the G-buffer's staging planes");
    size_t plane_off[11] = {};
    size_t off = 0;
    for (int c = 0; c < 11; ++c) {
        if (!ptr[c]) continue;
        plane_off[c] = off;
        off = (off + (size_t)band * W * bytes[c] + 255u) & ~(size_t)255u;
    }
    return staged_chunks(h, off, H, band, "the G-buffer's staging planes", [&](uint8_t* buf, uint64_t r0, uint64_t rows, const char*& what) {
        void* d_ptr[11] = {};
        for (int c = 0; c < 11; ++c)
            if (ptr[c]) d_ptr[c] = buf + plane_off[c];
        bind(d_ptr);
        g.row0 = (uint32_t)r0;
        g.rows = (uint32_t)rows;
        hipError_t e = hipSuccess;
        if (what = "launch_gbuffer", (e = launch_gbuffer(a, g, h->stream)) != hipSuccess) return e;
        what = "hipMemcpyAsync";
        for (int c = 0; c < 11 && e == hipSuccess; ++c) {
            if (!ptr[c]) continue;
            const size_t row = (size_t)W * bytes[c];
            e = hipMemcpyAsync(static_cast<uint8_t*>(ptr[c]) + r0 * row, d_ptr[c], rows * row, hipMemcpyDeviceToHost, h->stream);
        }
        return e;
    });
}

// ---- radiance along rays the host gives (include/rt_abi.h: rt_radiance_rays; rt_queries.inl: rt_radiance_kernel) ----
// Launched like a query: the arguments a render of the scene takes, the caller's bounces, samples and skybox, nothing read
// but the scene and the rays and nothing written but the caller's output (and a launch counter of the handle's ring).
static_assert(sizeof(rt_path_ray) == 32, "rt_path_ray layout");

int rt_radiance_rays(rt_handle* h, const rt_params* params, const rt_path_ray* rays, uint64_t n, float* rgba32f_out, int flags) {
    if (!h) return fail(h, RT_ERR_INVALID_ARGUMENT, "null handle");
    if (flags & ~RT_RADIANCE_HOST_MEMORY) return fail(h, RT_ERR_INVALID_ARGUMENT, "unknown flags");
    if (n == 0) return RT_OK;
    if (!params || !rays || !rgba32f_out) return fail(h, RT_ERR_INVALID_ARGUMENT, "null argument");
    if (params->number_of_bounces < 0) return fail(h, RT_ERR_INVALID_ARGUMENT, "number_of_bounces must be >= 0");
    if (params->rays_per_pixel < 1) return fail(h, RT_ERR_INVALID_ARGUMENT, "rays_per_pixel must be >= 1");
    if (n > 0x7fffffffull) return fail(h, RT_ERR_CAPACITY, "more than 2^31 - 1 rays");
    if (!h->have_scene) return fail(h, RT_ERR_NO_SCENE, "rt_upload_scene has not been called");
    const bool host = (flags & RT_RADIANCE_HOST_MEMORY) != 0;
    if (!host && ((((uintptr_t)rays) | ((uintptr_t)rgba32f_out)) & 15u) != 0u)
        return fail(h, RT_ERR_INVALID_ARGUMENT, "device rays / results not aligned (16 bytes)");
    HIP_TRY(h, hipSetDevice(h->device));
    RenderArgs a = query_args(h, nullptr);
    a.params.number_of_bounces = params->number_of_bounces;
    a.params.rays_per_pixel = params->rays_per_pixel;
    a.params.skybox = params->skybox;
    a.spp_reciprocal = (params->rays_per_pixel & (params->rays_per_pixel - 1)) == 0 ? 1.0f / (float)params->rays_per_pixel : 0.0f;  // (frame_constants)
    // SIMPLE from the scene alone: the rays are the caller's, the handle's camera has no part in them
    a.simple = (h->opt.specialise && h->inst.plain_materials) ? 1u : 0u;
    // The first hit of a ray serves all its samples from the lane's LDS memo, wherever a workgroup's LDS can hold one (a
    // ray of one sample has nothing to reuse); with it path_end's and the pre-step's shortcuts on that memo.
    a.pixel_cache = params->rays_per_pixel > 1 ? 1u : 0u;
    if (a.pixel_cache && render_lds_bytes(a) > rt2::CU_LDS_BYTES) a.pixel_cache = 0u;
    a.fast_miss = a.roulette_skip = a.pixel_cache;
    uint32_t* next_ray = nullptr;
    if (!host) {
        HIP_TRY(h, h->work.next(h->stream, next_ray));
        HIP_TRY(h, launch_radiance(a, rays, (uint32_t)n, rgba32f_out, next_ray, h->compute_units, h->stream));
        return RT_OK;
    }
    // host memory: chunks of at most 64 MB of device memory (rays, then results: 48 bytes per ray), within option max_device_mb
    const size_t per_ray = sizeof(rt_path_ray) + sizeof(float4);
    const uint64_t chunk = std::min<uint64_t>(n, staging_room(h) / per_ray);
    if (chunk == 0) return fail(h, RT_ERR_OUT_OF_MEMORY, "option max_device_mb leaves no room for a radiance call's staging buffers");
    return staged_chunks(h, chunk * per_ray, n, chunk, "a radiance call's staging buffers", [&](uint8_t* buf, uint64_t i0, uint64_t m, const char*& what) {
        uint8_t* d_out = buf + chunk * sizeof(rt_path_ray);
        hipError_t e = hipSuccess;
        if (what = "hipMemcpyAsync", (e = hipMemcpyAsync(buf, rays + i0, m * sizeof(rt_path_ray), hipMemcpyHostToDevice, h->stream)) != hipSuccess) return e;
        if (what = "CounterRing::next", (e = h->work.next(h->stream, next_ray)) != hipSuccess) return e;
        if (what = "launch_radiance", (e = launch_radiance(a, buf, (uint32_t)m, d_out, next_ray, h->compute_units, h->stream)) != hipSuccess) return e;
        what = "hipMemcpyAsync";
        return hipMemcpyAsync(rgba32f_out + 4 * i0, d_out, m * sizeof(float4), hipMemcpyDeviceToHost, h->stream);
    });
}

// ---- the passes over a rendered frame: rt_denoise, rt_denoise_variance / rt_luminance_moments, rt_adaptive_plan /
// rt_adaptive_merge, rt_temporal_accumulate / rt_temporal_accumulate_moving / rt_temporal_accumulate_deforming, rt_upsample,
// rt_display, rt_auto_exposure ----
// Launched like a query: nothing read but the caller's planes (or the image) and nothing written but the caller's outputs
// and a scratch the handle keeps.  Each entry point lists its planes once, in a table of FramePlane, and fills its launch
// arguments from the two pointer arrays frame_call gives it: the caller's own pointers on device memory, addresses in one
// temporary device buffer on host memory.

// One plane of a frame pass: read from `in`, written to `out`, or both -- an output that takes its input's place in the
// staging buffer, as `out` takes `color`'s.  An entry with neither pointer is absent and takes no room.
struct FramePlane {
    const void* in;
    void* out;
    size_t bytes;
};

extern "C++" {
// The staging buffer of the host-memory path: the planes that are there in table order, each at a multiple of 256 bytes.
template <int N>
static size_t staged_bytes(const FramePlane (&planes)[N], size_t* offsets = nullptr) {
    size_t total = 0;
    for (int c = 0; c < N; ++c) {
        if (!planes[c].in && !planes[c].out) continue;
        if (offsets) offsets[c] = total;
        total = (total + planes[c].bytes + 255u) & ~(size_t)255u;
    }
    return total;
}

// launch(in, out) on the planes of the table, in[c] / out[c] null for an absent plane.  Device memory: the table's own
// pointers, and the launch is queued.  Host memory: every plane whole through one temporary device buffer within option
// max_device_mb (a pass may read any row: no bands) -- the inputs copied in, in[c] == out[c] the staged plane, the outputs
// copied out, all in table order, and the stream drained (staged_chunks).
template <int N, class Launch>
static int frame_call(rt_handle* h, bool host, const FramePlane (&planes)[N], const char* what_for, const char* launch_name, Launch&& launch) {
    const void* in[N] = {};
    void* out[N] = {};
    if (!host) {
        for (int c = 0; c < N; ++c) in[c] = planes[c].in, out[c] = planes[c].out;
        const hipError_t e = launch(in, out);
        return e == hipSuccess ? RT_OK : fail(h, RT_ERR_DEVICE, std::string(launch_name) + "(a, h->stream): " + hipGetErrorString(e));
    }
    size_t offsets[N] = {};
    const size_t total = staged_bytes(planes, offsets);
    if (!fits_cap(h, total)) return fail(h, RT_ERR_OUT_OF_MEMORY, std::string("option max_device_mb leaves no room for ") + what_for);
    return staged_chunks(h, total, 1, 1, what_for, [&](uint8_t* buf, uint64_t, uint64_t, const char*& what) {
        hipError_t e = hipSuccess;
        what = "hipMemcpyAsync";
        for (int c = 0; c < N && e == hipSuccess; ++c) {
            if (!planes[c].in && !planes[c].out) continue;
            in[c] = out[c] = buf + offsets[c];
            if (planes[c].in) e = hipMemcpyAsync(out[c], planes[c].in, planes[c].bytes, hipMemcpyHostToDevice, h->stream);
        }
        if (e != hipSuccess) return e;
        if (what = launch_name, (e = launch(in, out)) != hipSuccess) return e;
        what = "hipMemcpyAsync";
        for (int c = 0; c < N && e == hipSuccess; ++c)
            if (planes[c].out) e = hipMemcpyAsync(planes[c].out, out[c], planes[c].bytes, hipMemcpyDeviceToHost, h->stream);
        return e;
    });
}

// A scratch the handle keeps between calls (`what`: its name in the messages), grown to `need` bytes on demand within option
// max_device_mb, together with the `staging` bytes the call is about to take (what_for: their name).  A call whose scratch
// is large enough checks its staging alone -- on device memory too, where that is 0 bytes: such a call is refused once the
// handle holds more than the cap, while the passes without a scratch (rt_temporal_accumulate, rt_adaptive_merge) go on.
template <class T>
static int grow_scratch(rt_handle* h, T*& scratch, size_t& held, size_t need, size_t staging, const char* what, const char* what_for) {
    auto no_room = [&](const char* for_what) { return fail(h, RT_ERR_OUT_OF_MEMORY, std::string("option max_device_mb leaves no room for ") + for_what); };
    if (held >= need) return fits_cap(h, staging) ? RT_OK : no_room(what_for);
    if (!fits_cap(h, need + staging, held)) return no_room(what);
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // (an earlier call may still use the old scratch)
    free_dev(scratch);
    held = 0;
    const hipError_t e = hipMalloc((void**)&scratch, need);
    if (e == hipErrorOutOfMemory) return fail(h, RT_ERR_OUT_OF_MEMORY, std::string("no device memory for ") + what);
    HIP_TRY(h, e);
    held = need;
    return RT_OK;
}

// A _host entry point: the host unit's restatement, its error kept for rt_last_error(NULL).
template <class Desc>
static int host_call(int (*restatement)(const Desc*, std::string&), const Desc* desc) {
    try {
        std::string err;
        const int rc = restatement(desc, err);
        return rc == RT_OK ? RT_OK : fail(nullptr, rc, err);
    } catch (const std::bad_alloc&) {
        return fail(nullptr, RT_ERR_OUT_OF_MEMORY, "out of host memory");
    }
}
}  // extern "C++" (templates among the C entry points)

// The colour plane of a pass: the caller's, or for NULL (device memory only: the checks refuse it elsewhere) the handle's
// image, which must hold the frame.
static int frame_color(rt_handle* h, const float*& color, size_t texels) {
    if (color) return RT_OK;
    if (texels > h->image_texels) return fail(h, RT_ERR_CAPACITY, "the frame has more texels than the image (color is NULL)");
    color = reinterpret_cast<const float*>(h->image);
    return RT_OK;
}

// Before a pass on device memory that reads `color` and writes `out`: a copy of the image that is still under way is
// waited for when either is the image, and the image counts as changed when `out` lies in it, as by rt_write_image.
static int image_access(rt_handle* h, const float* color, const float* out) {
    const float* image = reinterpret_cast<const float*>(h->image);
    const bool out_is_image = out >= image && out < image + 4 * h->image_texels;
    if (color == image || out_is_image) {
        if (int rc = wait_pending_copy(h); rc != RT_OK) return rc;
    }
    if (out_is_image) h->generation += 1;
    return RT_OK;
}

int rt_denoise_host(const rt_denoise_desc* desc) { return host_call(rt2::denoise_host, desc); }
int rt_denoise_variance_host(const rt_vdenoise_desc* desc) { return host_call(rt2::vdenoise_host, desc); }
int rt_luminance_moments_host(const rt_vdenoise_desc* desc) { return host_call(rt2::luminance_moments_host, desc); }
int rt_adaptive_plan_host(const rt_adaptive_plan_desc* desc) { return host_call(rt2::adaptive_plan_host, desc); }
int rt_adaptive_merge_host(const rt_adaptive_merge_desc* desc) { return host_call(rt2::adaptive_merge_host, desc); }
int rt_temporal_accumulate_host(const rt_temporal_desc* desc) { return host_call(rt2::temporal_host, desc); }
int rt_temporal_accumulate_moving_host(const rt_temporal_motion_desc* desc) { return host_call(rt2::temporal_motion_host, desc); }
int rt_temporal_accumulate_deforming_host(const rt_temporal_deform_desc* desc) { return host_call(rt2::temporal_deform_host, desc); }
int rt_upsample_host(const rt_upsample_desc* desc) { return host_call(rt2::upsample_host, desc); }
int rt_display_host(const rt_display_desc* desc) { return host_call(rt2::display_host, desc); }
int rt_auto_exposure_host(const rt_auto_exposure_desc* desc) { return host_call(rt2::auto_exposure_host, desc); }

// ---- denoising a rendered frame (include/rt_abi.h: rt_denoise; rt_denoise.hip; host/denoise.cpp) ----
static const char* const DENOISE_SCRATCH = "the denoiser's scratch images";
static const char* const DENOISE_STAGING = "the denoiser's staging planes";

int rt_denoise(rt_handle* h, const rt_denoise_desc* desc, int flags) {
    if (!h) return fail(h, RT_ERR_INVALID_ARGUMENT, "null handle");
    if (flags & ~RT_DENOISE_HOST_MEMORY) return fail(h, RT_ERR_INVALID_ARGUMENT, "unknown flags");
    const bool host = (flags & RT_DENOISE_HOST_MEMORY) != 0;
    std::string err;
    if (const int rc = rt2::denoise_check(desc, true, host, err); rc != RT_OK) return fail(h, rc, err);
    const size_t texels = (size_t)desc->width * desc->height;
    const float* color = desc->color;
    if (int rc = frame_color(h, color, texels); rc != RT_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const FramePlane planes[5] = {{color, desc->out, texels * 16u}, {desc->normal, nullptr, texels * 12u}, {desc->point, nullptr, texels * 12u},
                                  {desc->albedo, nullptr, texels * 16u}, {desc->emission, nullptr, texels * 16u}};
    if (int rc = grow_scratch(h, h->denoise_scratch, h->denoise_scratch_bytes, texels * 64u, host ? staged_bytes(planes) : 0u,
                              DENOISE_SCRATCH, DENOISE_STAGING); rc != RT_OK) return rc;
    if (int rc = host ? RT_OK : image_access(h, color, desc->out); rc != RT_OK) return rc;
    DenoiseArgs a{};
    a.width = desc->width;
    a.height = desc->height;
    a.iterations = (int)desc->iterations;
    a.sigma_color = desc->sigma_color;
    a.sigma_normal = desc->sigma_normal;
    a.sigma_point = desc->sigma_point;
    a.guide = h->denoise_scratch;
    a.ping[0] = h->denoise_scratch + 2 * texels;
    a.ping[1] = h->denoise_scratch + 3 * texels;
    return frame_call(h, host, planes, DENOISE_STAGING, "launch_denoise", [&](const void* const* in, void* const* out) {
        a.color = (const float*)in[0]; a.out = (float*)out[0];
        a.normal = (const float*)in[1]; a.point = (const float*)in[2]; a.albedo = (const float*)in[3]; a.emission = (const float*)in[4];
        return launch_denoise(a, h->stream);
    });
}

// ---- variance-guided denoising (include/rt_abi.h: rt_denoise_variance, rt_luminance_moments; rt_vdenoise.hip;
// host/vdenoise.cpp) ----
// Launched in rt_denoise's scratch: each call of either rewrites every word of it that it later reads.
// The two entry points: moments_only is rt_luminance_moments, which needs no scratch and takes fewer planes.
static int vdenoise_call(rt_handle* h, const rt_vdenoise_desc* desc, int flags, bool moments_only) {
    if (!h) return fail(h, RT_ERR_INVALID_ARGUMENT, "null handle");
    if (flags & ~RT_VDENOISE_HOST_MEMORY) return fail(h, RT_ERR_INVALID_ARGUMENT, "unknown flags");
    const bool host = (flags & RT_VDENOISE_HOST_MEMORY) != 0;
    std::string err;
    if (const int rc = rt2::vdenoise_check(desc, moments_only, true, host, err); rc != RT_OK) return fail(h, rc, err);
    const size_t texels = (size_t)desc->width * desc->height;
    const float* color = desc->color;
    if (int rc = frame_color(h, color, texels); rc != RT_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    // the first five are rt_denoise's
    const bool with_moments = !moments_only && desc->moments, with_variance = !moments_only && desc->out_variance;
    const FramePlane planes[8] = {{color, desc->out, texels * 16u}, {desc->normal, nullptr, texels * 12u}, {desc->point, nullptr, texels * 12u},
                                  {desc->albedo, nullptr, texels * 16u}, {desc->emission, nullptr, texels * 16u},
                                  {with_moments ? desc->moments : nullptr, nullptr, texels * 16u},
                                  {with_moments ? desc->history : nullptr, nullptr, texels * 4u},
                                  {nullptr, with_variance ? desc->out_variance : nullptr, texels * 4u}};
    if (int rc = grow_scratch(h, h->denoise_scratch, h->denoise_scratch_bytes, moments_only ? 0u : texels * 64u,
                              host ? staged_bytes(planes) : 0u, DENOISE_SCRATCH, DENOISE_STAGING); rc != RT_OK) return rc;
    if (int rc = host ? RT_OK : image_access(h, color, desc->out); rc != RT_OK) return rc;
    VDenoiseArgs a{};
    a.width = desc->width;
    a.height = desc->height;
    if (!moments_only) {
        a.iterations = (int)desc->iterations;
        a.sigma_luminance = desc->sigma_luminance;
        a.sigma_normal = desc->sigma_normal;
        a.sigma_point = desc->sigma_point;
        a.min_history = desc->min_history;
        a.guide = h->denoise_scratch;
        a.ping[0] = h->denoise_scratch + 2 * texels;
        a.ping[1] = h->denoise_scratch + 3 * texels;
    }
    return frame_call(h, host, planes, DENOISE_STAGING, moments_only ? "launch_luminance_moments" : "launch_vdenoise",
                      [&](const void* const* in, void* const* out) {
        a.color = (const float*)in[0]; a.out = (float*)out[0];
        a.normal = (const float*)in[1]; a.point = (const float*)in[2]; a.albedo = (const float*)in[3]; a.emission = (const float*)in[4];
        a.moments = (const float*)in[5]; a.history = (const float*)in[6]; a.out_variance = (float*)out[7];
        return moments_only ? launch_luminance_moments(a, h->stream) : launch_vdenoise(a, h->stream);
    });
}

int rt_denoise_variance(rt_handle* h, const rt_vdenoise_desc* desc, int flags) { return vdenoise_call(h, desc, flags, false); }
int rt_luminance_moments(rt_handle* h, const rt_vdenoise_desc* desc, int flags) { return vdenoise_call(h, desc, flags, true); }

// ---- adaptive sampling (include/rt_abi.h: rt_adaptive_plan, rt_adaptive_merge; rt_adaptive.hip; host/adaptive.cpp) ----
int rt_adaptive_plan(rt_handle* h, const rt_adaptive_plan_desc* desc, int flags) {
    if (!h) return fail(h, RT_ERR_INVALID_ARGUMENT, "null handle");
    if (flags & ~RT_ADAPTIVE_HOST_MEMORY) return fail(h, RT_ERR_INVALID_ARGUMENT, "unknown flags");
    const bool host = (flags & RT_ADAPTIVE_HOST_MEMORY) != 0;
    std::string err;
    if (const int rc = rt2::adaptive_plan_check(desc, true, host, err); rc != RT_OK) return fail(h, rc, err);
    const size_t texels = (size_t)desc->width * desc->height, budget = desc->budget;
    HIP_TRY(h, hipSetDevice(h->device));
    static const char* const what_for = "the adaptive plan's staging planes";
    const FramePlane planes[6] = {{desc->variance, nullptr, texels * 4u}, {desc->dir, nullptr, texels * 12u}, {nullptr, desc->counts, texels * 4u},
                                  {nullptr, desc->offsets, texels * 4u}, {nullptr, desc->rays, budget * sizeof(rt_path_ray)},
                                  {nullptr, desc->totals, 16u}};
    if (int rc = grow_scratch(h, h->adaptive_scratch, h->adaptive_scratch_bytes, adaptive_scratch_bytes(texels),
                              host ? staged_bytes(planes) : 0u, "the adaptive plan's scratch", what_for); rc != RT_OK) return rc;
    AdaptivePlanArgs a{};
    a.width = desc->width; a.height = desc->height; a.budget = desc->budget;
    a.min_samples = desc->min_samples; a.max_samples = desc->max_samples; a.first_frame = desc->first_frame;
    for (int k = 0; k < 3; ++k) a.origin[k] = desc->origin[k];
    a.scratch = h->adaptive_scratch;
    return frame_call(h, host, planes, what_for, "launch_adaptive_plan", [&](const void* const* in, void* const* out) {
        a.variance = (const float*)in[0]; a.dir = (const float*)in[1];
        a.counts = (uint32_t*)out[2]; a.offsets = (uint32_t*)out[3]; a.rays = out[4]; a.totals = (uint32_t*)out[5];
        return launch_adaptive_plan(a, h->stream);
    });
}

int rt_adaptive_merge(rt_handle* h, const rt_adaptive_merge_desc* desc, int flags) {
    if (!h) return fail(h, RT_ERR_INVALID_ARGUMENT, "null handle");
    if (flags & ~RT_ADAPTIVE_HOST_MEMORY) return fail(h, RT_ERR_INVALID_ARGUMENT, "unknown flags");
    const bool host = (flags & RT_ADAPTIVE_HOST_MEMORY) != 0;
    std::string err;
    if (const int rc = rt2::adaptive_merge_check(desc, true, host, err); rc != RT_OK) return fail(h, rc, err);
    const size_t texels = (size_t)desc->width * desc->height, budget = desc->budget;
    const float* color = desc->color;
    if (int rc = frame_color(h, color, texels); rc != RT_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = host ? RT_OK : image_access(h, color, desc->out); rc != RT_OK) return rc;
    // the outputs take the places of color, history and moments
    const FramePlane planes[7] = {{desc->radiance, nullptr, budget * 16u}, {desc->counts, nullptr, texels * 4u}, {desc->offsets, nullptr, texels * 4u},
                                  {color, desc->out, texels * 16u}, {desc->history, desc->out_history, texels * 4u},
                                  {desc->albedo, nullptr, texels * 16u}, {desc->moments, desc->out_moments, texels * 16u}};
    AdaptiveMergeArgs a{};
    a.width = desc->width; a.height = desc->height; a.budget = desc->budget; a.max_history = desc->max_history;
    return frame_call(h, host, planes, "the adaptive merge's staging planes", "launch_adaptive_merge", [&](const void* const* in, void* const* out) {
        a.radiance = (const float*)in[0]; a.counts = (const uint32_t*)in[1]; a.offsets = (const uint32_t*)in[2];
        a.color = (const float*)in[3]; a.out = (float*)out[3]; a.history = (const float*)in[4]; a.out_history = (float*)out[4];
        a.albedo = (const float*)in[5]; a.moments = (const float*)in[6]; a.out_moments = (float*)out[6];
        return launch_adaptive_merge(a, h->stream);
    });
}

// ---- temporal accumulation (include/rt_abi.h: rt_temporal_accumulate; rt_temporal.hip; host/temporal.cpp) ----
// No scratch is kept.  The three calls are one: `desc` is the kind's desc, which the check widens (rt_temporal_api.h), and
// the rows of a part the kind does not have -- the motion table (rt_temporal_accumulate_moving: one more input that is not
// frame-shaped), the current G-buffer's primitive, bary and flags planes and the previous triangles
// (rt_temporal_accumulate_deforming: a second one) -- are absent from the table and take no room.
static int temporal_accumulate(rt_handle* h, const void* desc, rt2::TemporalKind kind, int flags) {
    if (!h) return fail(h, RT_ERR_INVALID_ARGUMENT, "null handle");
    if (flags & ~RT_TEMPORAL_HOST_MEMORY) return fail(h, RT_ERR_INVALID_ARGUMENT, "unknown flags");
    const bool host = (flags & RT_TEMPORAL_HOST_MEMORY) != 0;
    std::string err;
    rt_temporal_deform_desc d;
    if (const int rc = rt2::temporal_check(desc, kind, true, host, d, err); rc != RT_OK) return fail(h, rc, err);
    const size_t texels = (size_t)d.width * d.height;
    const float* color = d.color;
    if (int rc = frame_color(h, color, texels); rc != RT_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = host ? RT_OK : image_access(h, color, d.out); rc != RT_OK) return rc;
    // `out` takes the colour plane's place
    const FramePlane planes[16] = {{color, d.out, texels * 16u}, {d.point, nullptr, texels * 12u}, {d.normal, nullptr, texels * 12u},
                                   {d.object, nullptr, texels * 4u}, {d.prev_color, nullptr, texels * 16u},
                                   {d.prev_history, nullptr, texels * 4u}, {d.prev_point, nullptr, texels * 12u},
                                   {d.prev_normal, nullptr, texels * 12u}, {d.prev_object, nullptr, texels * 4u},
                                   {nullptr, d.out_history, texels * 4u}, {nullptr, d.motion, texels * 8u},
                                   {d.motions, nullptr, (size_t)d.n_objects * sizeof(rt_object_motion)},
                                   {d.primitive, nullptr, texels * 4u}, {d.bary, nullptr, texels * 8u}, {d.flags, nullptr, texels},
                                   {d.prev_triangles, nullptr, (size_t)d.n_prev_triangles * sizeof(rt_packed_triangle)}};
    static const char* const LAUNCH[3] = {"launch_temporal", "launch_temporal_motion", "launch_temporal_deform"};   // (the device error names the kind)
    TemporalArgs a{};
    a.call = rt2::temporal_call(d);
    a.n_objects = d.n_objects;
    a.tri_first = d.tri_first;
    a.n_prev_triangles = d.n_prev_triangles;
    return frame_call(h, host, planes, "the staging planes of temporal accumulation", LAUNCH[(int)kind], [&](const void* const* in, void* const* out) {
        a.color = (const float*)in[0]; a.out = (float*)out[0]; a.point = (const float*)in[1]; a.normal = (const float*)in[2];
        a.object = (const uint32_t*)in[3]; a.prev_color = (const float*)in[4]; a.prev_history = (const float*)in[5];
        a.prev_point = (const float*)in[6]; a.prev_normal = (const float*)in[7]; a.prev_object = (const uint32_t*)in[8];
        a.out_history = (float*)out[9]; a.motion = (float*)out[10]; a.motions = (const rttp::Motion*)in[11];
        a.primitive = (const uint32_t*)in[12]; a.bary = (const float*)in[13]; a.flags = (const uint8_t*)in[14];
        a.prev_triangles = (const rttp::Tri*)in[15];
        return launch_temporal(a, kind, h->stream);
    });
}

int rt_temporal_accumulate(rt_handle* h, const rt_temporal_desc* desc, int flags) { return temporal_accumulate(h, desc, rt2::TemporalKind::PLAIN, flags); }
int rt_temporal_accumulate_moving(rt_handle* h, const rt_temporal_motion_desc* desc, int flags) { return temporal_accumulate(h, desc, rt2::TemporalKind::MOVING, flags); }
int rt_temporal_accumulate_deforming(rt_handle* h, const rt_temporal_deform_desc* desc, int flags) { return temporal_accumulate(h, desc, rt2::TemporalKind::DEFORMING, flags); }

// ---- guided upsampling (include/rt_abi.h: rt_upsample; rt_upsample.hip; host/upsample.cpp) ----
// No scratch is kept.  The low frame's planes are inputs that are not frame-shaped with respect to the high frame: rows of
// the table with their own sizes, like the motion table of rt_temporal_accumulate_moving.
int rt_upsample(rt_handle* h, const rt_upsample_desc* desc, int flags) {
    if (!h) return fail(h, RT_ERR_INVALID_ARGUMENT, "null handle");
    if (flags & ~RT_UPSAMPLE_HOST_MEMORY) return fail(h, RT_ERR_INVALID_ARGUMENT, "unknown flags");
    const bool host = (flags & RT_UPSAMPLE_HOST_MEMORY) != 0;
    std::string err;
    if (const int rc = rt2::upsample_check(desc, true, host, err); rc != RT_OK) return fail(h, rc, err);
    const size_t lo = (size_t)desc->lo_width * desc->lo_height, texels = (size_t)desc->width * desc->height;
    const float* lo_color = desc->lo_color;
    if (int rc = frame_color(h, lo_color, lo); rc != RT_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = host ? RT_OK : image_access(h, lo_color, desc->out); rc != RT_OK) return rc;
    const FramePlane planes[13] = {{lo_color, nullptr, lo * 16u}, {desc->lo_point, nullptr, lo * 12u}, {desc->lo_normal, nullptr, lo * 12u},
                                   {desc->lo_object, nullptr, lo * 4u}, {desc->lo_albedo, nullptr, lo * 16u},
                                   {desc->depth, nullptr, texels * 4u}, {desc->point, nullptr, texels * 12u},
                                   {desc->normal, nullptr, texels * 12u}, {desc->object, nullptr, texels * 4u},
                                   {desc->albedo, nullptr, texels * 16u}, {desc->emission, nullptr, texels * 16u},
                                   {nullptr, desc->out, texels * 16u}, {nullptr, desc->coverage, texels}};
    UpsampleArgs a{};
    a.call = rt2::upsample_call(*desc);
    return frame_call(h, host, planes, "the staging planes of guided upsampling", "launch_upsample", [&](const void* const* in, void* const* out) {
        a.lo_color = (const float*)in[0]; a.lo_point = (const float*)in[1]; a.lo_normal = (const float*)in[2];
        a.lo_object = (const uint32_t*)in[3]; a.lo_albedo = (const float*)in[4]; a.depth = (const float*)in[5];
        a.point = (const float*)in[6]; a.normal = (const float*)in[7]; a.object = (const uint32_t*)in[8];
        a.albedo = (const float*)in[9]; a.emission = (const float*)in[10]; a.out = (float*)out[11]; a.coverage = (uint8_t*)out[12];
        return launch_upsample(a, h->stream);
    });
}

// ---- display frames (include/rt_abi.h: rt_display, rt_auto_exposure; rt_display.hip; host/display.cpp) ----
// rt_display keeps no scratch; its one-float exposure_scale is a row of the table like any plane.
int rt_display(rt_handle* h, const rt_display_desc* desc, int flags) {
    if (!h) return fail(h, RT_ERR_INVALID_ARGUMENT, "null handle");
    if (flags & ~RT_DISPLAY_HOST_MEMORY) return fail(h, RT_ERR_INVALID_ARGUMENT, "unknown flags");
    const bool host = (flags & RT_DISPLAY_HOST_MEMORY) != 0;
    std::string err;
    if (const int rc = rt2::display_check(desc, host ? rt2::DisplayPath::STAGED : rt2::DisplayPath::DEVICE, err); rc != RT_OK) return fail(h, rc, err);
    const size_t texels = (size_t)desc->width * desc->height;
    const float* color = desc->color;
    if (int rc = frame_color(h, color, texels); rc != RT_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = host ? RT_OK : image_access(h, color, reinterpret_cast<const float*>(desc->out)); rc != RT_OK) return rc;
    const FramePlane planes[3] = {{color, nullptr, texels * 16u}, {desc->exposure_scale, nullptr, 4u}, {nullptr, desc->out, texels * 4u}};
    DisplayArgs a{};
    a.call = rt2::display_call(*desc);
    return frame_call(h, host, planes, "the staging planes of the display pass", "launch_display", [&](const void* const* in, void* const* out) {
        a.color = (const float*)in[0]; a.exposure_scale = (const float*)in[1]; a.out = (uint32_t*)out[2];
        return launch_display(a, h->stream);
    });
}

// The 1 KiB of global bins is the scratch the handle keeps; prev_scale, histogram and scale are rows of 4, 1024 and 4 bytes.
int rt_auto_exposure(rt_handle* h, const rt_auto_exposure_desc* desc, int flags) {
    if (!h) return fail(h, RT_ERR_INVALID_ARGUMENT, "null handle");
    if (flags & ~RT_AUTO_EXPOSURE_HOST_MEMORY) return fail(h, RT_ERR_INVALID_ARGUMENT, "unknown flags");
    const bool host = (flags & RT_AUTO_EXPOSURE_HOST_MEMORY) != 0;
    std::string err;
    if (const int rc = rt2::auto_exposure_check(desc, true, host, err); rc != RT_OK) return fail(h, rc, err);
    const size_t texels = (size_t)desc->width * desc->height;
    const float* color = desc->color;
    if (int rc = frame_color(h, color, texels); rc != RT_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    static const char* const what_for = "the exposure meter's staging planes";
    const FramePlane planes[4] = {{color, nullptr, texels * 16u}, {desc->prev_scale, nullptr, 4u},
                                  {nullptr, desc->histogram, rtdp::BINS * sizeof(uint32_t)}, {nullptr, desc->scale, 4u}};
    if (int rc = grow_scratch(h, h->exposure_scratch, h->exposure_scratch_bytes, rtdp::BINS * sizeof(uint32_t),
                              host ? staged_bytes(planes) : 0u, "the exposure meter's bins", what_for); rc != RT_OK) return rc;
    if (int rc = host ? RT_OK : image_access(h, color, desc->scale); rc != RT_OK) return rc;
    AutoExposureArgs a{};
    a.call = rt2::auto_exposure_call(*desc);
    a.bins = h->exposure_scratch;
    return frame_call(h, host, planes, what_for, "launch_auto_exposure", [&](const void* const* in, void* const* out) {
        a.color = (const float*)in[0]; a.prev_scale = (const float*)in[1]; a.histogram = (uint32_t*)out[2]; a.scale = (float*)out[3];
        return launch_auto_exposure(a, h->stream);
    });
}

int rt_synchronize(rt_handle* h) {
    if (!h) return RT_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return RT_OK;
}

int rt_read_image(rt_handle* h, float* out, size_t bytes) {
    if (!h || !out) return fail(h, RT_ERR_INVALID_ARGUMENT, "null argument");
    if (bytes > h->image_texels * sizeof(float4))
        return fail(h, RT_ERR_INVALID_ARGUMENT, "read larger than the image");
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = wait_pending_copy(h); rc != RT_OK) return rc;
    HIP_TRY(h, hipMemcpyAsync(out, h->image, bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return RT_OK;
}

// The frame of the last call, kept aside in stream order (a device-to-device copy, ~15 us for 33 MB): the handle's stream
// goes on rendering, rt_read_snapshot brings the copy to the host on a stream of its own (the copy engines run beside the
// kernels), so that a host that shows every frame pays max(render, read) per frame instead of their sum.
int rt_snapshot_image(rt_handle* h, size_t bytes) {
    if (!h) return RT_ERR_INVALID_ARGUMENT;
    if (bytes == 0 || bytes > h->image_texels * sizeof(float4))
        return fail(h, RT_ERR_INVALID_ARGUMENT, "snapshot empty or larger than the image");
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = wait_pending_copy(h); rc != RT_OK) return rc;
    // (each object on its own: a creation that failed half-way must not leave later calls with null events)
    if (!h->copy_stream) HIP_TRY(h, hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
    if (!h->snapshot_taken) HIP_TRY(h, hipEventCreateWithFlags(&h->snapshot_taken, hipEventDisableTiming));
    if (!h->snapshot_read) HIP_TRY(h, hipEventCreateWithFlags(&h->snapshot_read, hipEventDisableTiming));
    if (h->snapshot_capacity < bytes) {
        HIP_TRY(h, hipStreamSynchronize(h->copy_stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        free_dev(h->snapshot);
        h->snapshot_capacity = h->snapshot_bytes = 0;
        HIP_TRY(h, hipMalloc((void**)&h->snapshot, bytes));
        h->snapshot_capacity = bytes;
        h->snapshot_read_pending = false;
    }
    // (a read of the previous snapshot that is still under way keeps its bytes: the new copy waits for it)
    if (h->snapshot_read_pending) HIP_TRY(h, hipStreamWaitEvent(h->stream, h->snapshot_read, 0));
    h->snapshot_read_pending = false;
    HIP_TRY(h, hipMemcpyAsync(h->snapshot, h->image, bytes, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(h, hipEventRecord(h->snapshot_taken, h->stream));
    h->snapshot_bytes = bytes;
    return RT_OK;
}

// Blocking read of the last snapshot (not of the image: frames rendered since the snapshot are not waited for).
int rt_read_snapshot(rt_handle* h, float* out, size_t bytes) {
    if (!h || !out) return fail(h, RT_ERR_INVALID_ARGUMENT, "null argument");
    if (h->snapshot_bytes == 0) return fail(h, RT_ERR_INVALID_ARGUMENT, "rt_snapshot_image has not been called");
    if (bytes > h->snapshot_bytes) return fail(h, RT_ERR_INVALID_ARGUMENT, "read larger than the snapshot");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamWaitEvent(h->copy_stream, h->snapshot_taken, 0));
    HIP_TRY(h, hipMemcpyAsync(out, h->snapshot, bytes, hipMemcpyDeviceToHost, h->copy_stream));
    HIP_TRY(h, hipEventRecord(h->snapshot_read, h->copy_stream));
    h->snapshot_read_pending = true;
    HIP_TRY(h, hipStreamSynchronize(h->copy_stream));
    return RT_OK;
}

// The pair above with the display pass in the place of the copy, on a buffer and events of its own (the copy stream is
// shared: reads of the two pairs queue behind each other there, nothing else).
int rt_snapshot_display(rt_handle* h, const rt_display_desc* desc) {
    if (!h) return RT_ERR_INVALID_ARGUMENT;
    std::string err;
    if (const int rc = rt2::display_check(desc, rt2::DisplayPath::SNAPSHOT, err); rc != RT_OK) return fail(h, rc, err);
    const size_t texels = (size_t)desc->width * desc->height, bytes = texels * 4u;
    if (texels > h->image_texels) return fail(h, RT_ERR_CAPACITY, "the frame has more texels than the image");
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = wait_pending_copy(h); rc != RT_OK) return rc;
    if (!h->copy_stream) HIP_TRY(h, hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
    if (!h->display_taken) HIP_TRY(h, hipEventCreateWithFlags(&h->display_taken, hipEventDisableTiming));
    if (!h->display_read) HIP_TRY(h, hipEventCreateWithFlags(&h->display_read, hipEventDisableTiming));
    if (h->display_snapshot_capacity < bytes) {
        if (!fits_cap(h, bytes, h->display_snapshot_capacity))
            return fail(h, RT_ERR_OUT_OF_MEMORY, "option max_device_mb leaves no room for the display snapshot");
        HIP_TRY(h, hipStreamSynchronize(h->copy_stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        free_dev(h->display_snapshot);
        h->display_snapshot_capacity = h->display_snapshot_bytes = 0;
        const hipError_t e = hipMalloc((void**)&h->display_snapshot, bytes);
        if (e == hipErrorOutOfMemory) return fail(h, RT_ERR_OUT_OF_MEMORY, "no device memory for the display snapshot");
        HIP_TRY(h, e);
        h->display_snapshot_capacity = bytes;
        h->display_read_pending = false;
    }
    // (a read of the previous picture that is still under way keeps its bytes: the encode waits for it)
    if (h->display_read_pending) HIP_TRY(h, hipStreamWaitEvent(h->stream, h->display_read, 0));
    h->display_read_pending = false;
    DisplayArgs a{};
    a.call = rt2::display_call(*desc);
    a.color = reinterpret_cast<const float*>(h->image);
    a.exposure_scale = desc->exposure_scale;
    a.out = reinterpret_cast<uint32_t*>(h->display_snapshot);
    HIP_TRY(h, launch_display(a, h->stream));
    HIP_TRY(h, hipEventRecord(h->display_taken, h->stream));
    h->display_snapshot_bytes = bytes;
    return RT_OK;
}

int rt_read_display_snapshot(rt_handle* h, uint8_t* out, size_t bytes) {
    if (!h || !out) return fail(h, RT_ERR_INVALID_ARGUMENT, "null argument");
    if (h->display_snapshot_bytes == 0) return fail(h, RT_ERR_INVALID_ARGUMENT, "rt_snapshot_display has not been called");
    if (bytes > h->display_snapshot_bytes) return fail(h, RT_ERR_INVALID_ARGUMENT, "read larger than the display snapshot");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamWaitEvent(h->copy_stream, h->display_taken, 0));
    HIP_TRY(h, hipMemcpyAsync(out, h->display_snapshot, bytes, hipMemcpyDeviceToHost, h->copy_stream));
    HIP_TRY(h, hipEventRecord(h->display_read, h->copy_stream));
    h->display_read_pending = true;
    HIP_TRY(h, hipStreamSynchronize(h->copy_stream));
    return RT_OK;
}

int rt_write_image(rt_handle* h, const float* in, size_t bytes) {
    if (!h || !in) return fail(h, RT_ERR_INVALID_ARGUMENT, "null argument");
    if (bytes > h->image_texels * sizeof(float4))
        return fail(h, RT_ERR_INVALID_ARGUMENT, "write larger than the image");
    h->generation += 1;
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = wait_pending_copy(h); rc != RT_OK) return rc;
    HIP_TRY(h, hipMemcpyAsync(h->image, in, bytes, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return RT_OK;
}

int rt_get_stats(rt_handle* h, rt_stats* out) {
    if (!h || !out) return fail(h, RT_ERR_INVALID_ARGUMENT, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    Counters c{};
    // (on the handle's stream, never the null stream: a process that has touched the null stream holds one more hardware
    // queue, and with main + three pipeline streams + null the pipelined frames' streams start sharing queues -- measured:
    // 1.30 -> 1.42 ms per frame after the first rt_get_stats)
    HIP_TRY(h, hipMemcpyAsync(&c, h->counters, sizeof(c), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    memset(out, 0, sizeof(*out));
    out->segments = c.segments;
    out->paths = h->paths_total;
    out->node_tests = c.node_tests;
    out->triangle_tests = c.triangle_tests;
    out->segments_reused = c.reused;
    // counters accumulate over all launches since rt_reset_timing
    double total = h->ev_ms_harvested;
    HIP_TRY(h, harvest_event_times(h, total));
    out->kernel_ms = (float)total;
    out->launches = (uint32_t)h->launches_total;
    out->frames = (uint32_t)h->ahead.frames_asked;
    out->frames_speculative = (uint32_t)h->ahead.frames_speculative;
    return RT_OK;
}

int rt_last_launch(rt_handle* h, uint32_t out[6]) {
    if (!h || !out) return fail(h, RT_ERR_INVALID_ARGUMENT, "null argument");
    for (int k = 0; k < 4; ++k) out[k] = h->last_launch[k];
    out[4] = (uint32_t)((optional_bytes(h) + (1u << 20) - 1) >> 20);   // MiB held on the library's own initiative (option max_device_mb)
    out[5] = (uint32_t)h->opt.max_device_mb;                              // the cap (0 = none)
    return RT_OK;
}

int rt_reset_timing(rt_handle* h) {
    if (!h) return RT_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemsetAsync(h->counters, 0, sizeof(Counters), h->stream));
    // (a pipelined frame's sampling launch runs on an internal stream that is not ordered behind this stream's
    // memset: the zeroing is complete before the call returns, so no later launch's counter adds can race with it)
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->ev_used = 0;
    h->ev_ms_harvested = 0.0;
    h->launches_total = 0;
    h->ahead.reset_counts();
    h->paths_total = 0;
    return RT_OK;
}

int rt_set_stream(rt_handle* h, void* hip_stream) {
    if (!h) return RT_ERR_INVALID_ARGUMENT;
    h->generation += 1;
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = wait_pending_copy(h); rc != RT_OK) return rc;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, harvest_event_times(h, h->ev_ms_harvested));  // (the old stream is idle: its recorded times are final)
    h->ev_used = 0;
    h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
    return RT_OK;
}

int rt_bind_image(rt_handle* h, void* device_ptr, uint64_t texels) {
    if (!h) return RT_ERR_INVALID_ARGUMENT;
    h->generation += 1;
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = wait_pending_copy(h); rc != RT_OK) return rc;  // (the caller may free the old buffer after this call)
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (device_ptr) {
        h->image = (float4*)device_ptr;
        h->image_texels = texels;
    } else {
        h->image = h->own_image;
        h->image_texels = (size_t)h->max_width * h->max_height;
    }
    return RT_OK;
}

#if defined(RT_DIAG) || defined(RT_WAVE_TIMES)
int rt_diag_wave_times(rt_handle* h, unsigned long long* out) {
    if (!h || !out) return RT_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, rtd::diag_wave_times(out));
    return RT_OK;
}
#endif
#if defined(RT_DIAG) || defined(RT_DIAGT)
int rt_diag_read(rt_handle* h, unsigned long long* out64, int reset) {
    if (!h || !out64) return RT_ERR_INVALID_ARGUMENT;
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, rtd::diag_read(out64, reset != 0));
    return RT_OK;
}
#endif

#if RT_TEST_ENTRIES
// The test entry points (include/rt_test_abi.h) are NOT part of the product library: they are compiled only with
// -DRT_TEST_ENTRIES=1, into ray_tracer_2_amd/librt2_mi355x_test.so (ray_tracer_2_amd/build.py: build_test_library) --
// the same sources and flags otherwise.
// tests/test_gpu_device_units.py: evaluate the kernels' arithmetic building blocks on the device, element-wise over host arrays.
int rt_test_device_units(rt_handle* h, int fn, const float* x, const float* y, float* out, uint64_t n) {
    if (!h || !x || !y || !out) return fail(h, RT_ERR_INVALID_ARGUMENT, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    float *dx = nullptr, *dy = nullptr, *dout = nullptr;
    const size_t bytes = (size_t)(n ? n : 1) * sizeof(float);
    HIP_TRY(h, hipMalloc((void**)&dx, bytes));
    HIP_TRY(h, hipMalloc((void**)&dy, bytes));
    HIP_TRY(h, hipMalloc((void**)&dout, bytes));
    HIP_TRY(h, hipMemcpyAsync(dx, x, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(dy, y, n * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, launch_units(fn, dx, dy, dout, n, h->stream));
    HIP_TRY(h, hipMemcpyAsync(out, dout, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    free_dev(dx);
    free_dev(dy);
    free_dev(dout);
    return RT_OK;
}

// tests/test_gpu_scene_edits.py: the scene blob as the kernels read it, its SceneLayout and its device address -- to
// compare an updated handle with a fresh upload, and to see that an in-place update kept its allocation.
int rt_test_scene_blob(rt_handle* h, void* out, uint64_t bytes, uint32_t layout_out[12], uint64_t* device_ptr) {
    if (!h) return fail(h, RT_ERR_INVALID_ARGUMENT, "null handle");
    if (!h->have_scene) return fail(h, RT_ERR_NO_SCENE, "rt_upload_scene has not been called");
    if (out && bytes < h->inst.lay.bytes) return fail(h, RT_ERR_INVALID_ARGUMENT, "output smaller than the blob");
    static_assert(sizeof(SceneLayout) == 12 * sizeof(uint32_t), "SceneLayout is 12 words");
    if (layout_out) memcpy(layout_out, &h->inst.lay, sizeof(SceneLayout));
    if (device_ptr) *device_ptr = (uint64_t)(uintptr_t)h->blob;
    if (out) {
        HIP_TRY(h, hipSetDevice(h->device));
        if (int rc = drain_streams(h); rc != RT_OK) return rc;
        HIP_TRY(h, hipMemcpy(out, h->blob, h->inst.lay.bytes, hipMemcpyDeviceToHost));
    }
    return RT_OK;
}

// tests/test_scene_pack_host.py, tests/test_gpu_scene_pack.py: the host packer on scene arrays, without a device -- both
// phases as rt_upload_scene runs them, the blob assembled as the device would hold it (head, tail, zero padding), and the
// instance phase run again on the same geometry facts, as rt_update_instances would.
int rt_test_pack_scene(const rt_sphere* spheres, uint32_t n_spheres, const rt_mesh_uniform* meshes, uint32_t n_meshes,
                       const rt_packed_triangle* triangles, uint32_t n_triangles, const rt_node* nodes, uint32_t n_nodes,
                       const int32_t options[5], void* out, uint64_t bytes, uint32_t layout_out[12], uint32_t facts_out[RT_TEST_PACK_FACTS]) {
    if (!options || (n_spheres && !spheres) || (n_meshes && !meshes) || (n_triangles && !triangles) || (n_nodes && !nodes))
        return fail(nullptr, RT_ERR_INVALID_ARGUMENT, "null array with non-zero count");
    try {
        const rt2::PackOptions opt{options[0], options[1], options[2], options[3], options[4]};
        SceneGeom g;
        InstanceFacts s, again;
        std::vector<rt2::Quad> head, head_again, tail;
        std::string why;
        int rc = rt2::pack_geometry(meshes, n_meshes, triangles, n_triangles, nodes, n_nodes, g, tail, why);
        if (rc == RT_OK) rc = rt2::pack_instances(opt, g, spheres, n_spheres, meshes, n_meshes, s, head, why);
        if (rc == RT_OK) rc = rt2::pack_instances(opt, g, spheres, n_spheres, meshes, n_meshes, again, head_again, why);
        if (rc != RT_OK) return fail(nullptr, rc, why);
        const size_t head_bytes = head.size() * sizeof(rt2::Quad);
        const bool same = head.size() == head_again.size() && (head.empty() || memcmp(head.data(), head_again.data(), head_bytes) == 0) &&
                          memcmp(&s.lay, &again.lay, sizeof(SceneLayout)) == 0;
        if (out && bytes < s.lay.bytes) return fail(nullptr, RT_ERR_INVALID_ARGUMENT, "output smaller than the blob");
        if (layout_out) memcpy(layout_out, &s.lay, sizeof(SceneLayout));
        if (facts_out) {
            const uint32_t f[RT_TEST_PACK_FACTS] = {s.n_items, s.n_tlas_records, s.n_forest_entries, s.tlas_entries, s.has_tlas, s.has_forest, s.plain_materials,
                                                    s.have_defer, s.defer_mesh, s.defer_xform, s.defer_internal, g.max_height, g.max_leaf_ref, g.top_mesh_records,
                                                    g.top_mesh_base, g.roots_are_unions, g.any_deep, same};
            memcpy(facts_out, f, sizeof(f));
        }
        if (out) {
            memset(out, 0, s.lay.bytes);
            if (!head.empty()) memcpy(out, head.data(), head_bytes);
            if (!tail.empty()) memcpy((char*)out + s.lay.wide_off, tail.data(), tail.size() * sizeof(rt2::Quad));
        }
    } catch (const std::bad_alloc&) {
        return fail(nullptr, RT_ERR_OUT_OF_MEMORY, "out of host memory");
    }
    return RT_OK;
}

// tests/test_gpu_intersect.py: intersect_scene for host-given rays, on the uploaded scene, with the arguments and the
// instantiation a render launches (query_args, render_takes_simple) unless `flags` force one.
int rt_test_intersect(rt_handle* h, const float* ro, const float* rd, const uint8_t* active, uint64_t n, int flags,
                      uint32_t* out) {
    if (!h || (n && (!ro || !rd || !out))) return fail(h, RT_ERR_INVALID_ARGUMENT, "null argument");
    if (flags & ~(RT_TEST_ISECT_GENERAL | RT_TEST_ISECT_STATS | RT_TEST_ISECT_SIMPLE))
        return fail(h, RT_ERR_INVALID_ARGUMENT, "unknown flags");
    if ((flags & RT_TEST_ISECT_GENERAL) && (flags & RT_TEST_ISECT_SIMPLE))
        return fail(h, RT_ERR_INVALID_ARGUMENT, "flags ask for both the general and the SIMPLE instantiation");
    if (n > RT_TEST_ISECT_MAX_RAYS) return fail(h, RT_ERR_CAPACITY, "too many rays");
    if (!h->have_scene) return fail(h, RT_ERR_NO_SCENE, "rt_upload_scene has not been called");
    // only rays a render can trace: finite origins, finite non-zero directions (the kernels' normalize gives these)
    for (uint64_t i = 0; i < 3 * n; ++i)
        if (!std::isfinite(ro[i]) || !std::isfinite(rd[i])) return fail(h, RT_ERR_INVALID_ARGUMENT, "non-finite ray");
    for (uint64_t i = 0; i < n; ++i)
        if (rd[3 * i] == 0.0f && rd[3 * i + 1] == 0.0f && rd[3 * i + 2] == 0.0f)
            return fail(h, RT_ERR_INVALID_ARGUMENT, "zero direction");
    const RenderArgs a = query_args(h, nullptr);
    const bool stats = (flags & RT_TEST_ISECT_STATS) != 0;
    bool simple = render_takes_simple(a) && !stats;  // (the counter instantiations are the general code)
    if (flags & RT_TEST_ISECT_GENERAL) simple = false;
    if (flags & RT_TEST_ISECT_SIMPLE) {
        if (a.many_mesh || !h->inst.plain_materials)
            return fail(h, RT_ERR_INVALID_ARGUMENT, "the SIMPLE instantiation needs a few-mesh scene without spheres, glass or textures");
        simple = true;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = wait_pending_copy(h); rc != RT_OK) return rc;
    float *dro = nullptr, *drd = nullptr;
    uint8_t* dact = nullptr;
    uint32_t* dout = nullptr;
    const size_t m = (size_t)(n ? n : 1);
    HIP_TRY(h, hipMalloc((void**)&dro, m * 3 * sizeof(float)));
    HIP_TRY(h, hipMalloc((void**)&drd, m * 3 * sizeof(float)));
    HIP_TRY(h, hipMalloc((void**)&dout, m * RT_TEST_ISECT_WORDS * sizeof(uint32_t)));
    if (active) HIP_TRY(h, hipMalloc((void**)&dact, m));
    HIP_TRY(h, hipMemcpyAsync(dro, ro, n * 3 * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(drd, rd, n * 3 * sizeof(float), hipMemcpyHostToDevice, h->stream));
    if (active) HIP_TRY(h, hipMemcpyAsync(dact, active, n, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemsetAsync(dout, 0, m * RT_TEST_ISECT_WORDS * sizeof(uint32_t), h->stream));
    HIP_TRY(h, launch_test_intersect(a, dro, drd, dact, n, simple, stats, dout, h->stream));
    HIP_TRY(h, hipMemcpyAsync(out, dout, n * RT_TEST_ISECT_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    free_dev(dro);
    free_dev(drd);
    free_dev(dact);
    free_dev(dout);
    return RT_OK;
}

// tests/test_gpu_shade.py: path_end / roulette_skip for host-given lane states and hits, on the uploaded scene's materials
// and textures, with the arguments of a render (query_args) minus the pixel memo and the instantiation it launches
// (render_takes_simple) unless `flags` force one.  Everything is checked here: nothing the kernel indexes with comes from
// the cases unchecked.
int rt_test_shade(rt_handle* h, int which, const uint32_t* cases, const uint8_t* active, uint64_t n, int number_of_bounces,
                  int rays_per_pixel, int skybox, int flags, uint32_t* out) {
    if (!h || (n && (!cases || !out))) return fail(h, RT_ERR_INVALID_ARGUMENT, "null argument");
    if (which != RT_TEST_SHADE_PATH_END && which != RT_TEST_SHADE_ROULETTE_SKIP) return fail(h, RT_ERR_INVALID_ARGUMENT, "unknown function");
    if (flags & ~(RT_TEST_SHADE_GENERAL | RT_TEST_SHADE_NO_FAST_MISS | RT_TEST_SHADE_SIMPLE | RT_TEST_SHADE_TOTAL_REGS))
        return fail(h, RT_ERR_INVALID_ARGUMENT, "unknown flags");
    if ((flags & RT_TEST_SHADE_GENERAL) && (flags & RT_TEST_SHADE_SIMPLE))
        return fail(h, RT_ERR_INVALID_ARGUMENT, "flags ask for both the general and the SIMPLE instantiation");
    if (n > RT_TEST_SHADE_MAX_CASES) return fail(h, RT_ERR_INVALID_ARGUMENT, "too many cases");
    if (!h->have_scene) return fail(h, RT_ERR_NO_SCENE, "rt_upload_scene has not been called");
    RenderArgs a = query_args(h, nullptr);
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t* c = cases + i * RT_TEST_SHADE_WORDS;
        if (c[30] >= a.n_meshes + a.n_spheres) return fail(h, RT_ERR_INVALID_ARGUMENT, "object index outside the scene");
        if (c[18] != RT_TEST_SHADE_STEP_END && c[18] != RT_TEST_SHADE_STEP_TRAVERSE) return fail(h, RT_ERR_INVALID_ARGUMENT, "unknown step mode");
    }
    a.params.number_of_bounces = number_of_bounces;
    a.params.rays_per_pixel = rays_per_pixel;
    a.params.skybox = skybox;
    a.pixel_cache = 0u;  // (no memo: path_end's FAST_MISS reads none, and the LDS map holds none)
    a.fast_miss = a.roulette_skip = 0u;
    bool simple = render_takes_simple(a);
    if (flags & RT_TEST_SHADE_GENERAL) simple = false;
    if (flags & RT_TEST_SHADE_SIMPLE) {
        if (a.many_mesh || !h->inst.plain_materials)
            return fail(h, RT_ERR_INVALID_ARGUMENT, "the SIMPLE instantiation needs a few-mesh scene without spheres, glass or textures");
        simple = true;
    }
    const bool total_lds = total_in_lds(a.lds_scene != 0u) && !(flags & RT_TEST_SHADE_TOTAL_REGS);
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = wait_pending_copy(h); rc != RT_OK) return rc;
    uint32_t *dcases = nullptr, *dout = nullptr;
    uint8_t* dact = nullptr;
    const size_t m = (size_t)(n ? n : 1), bytes = m * RT_TEST_SHADE_WORDS * sizeof(uint32_t), used = (size_t)n * RT_TEST_SHADE_WORDS * sizeof(uint32_t);
    // One exit: whatever fails, the stream is drained before the buffers are freed (nothing queued may still point at them),
    // and they are freed (staged_chunks' form).
    const char* what = "hipMalloc";
    hipError_t e = hipMalloc((void**)&dcases, bytes);
    if (e == hipSuccess) e = hipMalloc((void**)&dout, bytes);
    if (e == hipSuccess && active) e = hipMalloc((void**)&dact, m);
    if (e == hipSuccess) {
        what = "hipMemcpyAsync";
        e = hipMemcpyAsync(dcases, cases, used, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess && active) e = hipMemcpyAsync(dact, active, n, hipMemcpyHostToDevice, h->stream);
        if (e == hipSuccess) what = "hipMemsetAsync", e = hipMemsetAsync(dout, 0, bytes, h->stream);
        if (e == hipSuccess)
            what = "launch_test_shade", e = launch_test_shade(a, which, dcases, dact, n, simple, !(flags & RT_TEST_SHADE_NO_FAST_MISS), total_lds, dout, h->stream);
        if (e == hipSuccess) what = "hipMemcpyAsync", e = hipMemcpyAsync(out, dout, used, hipMemcpyDeviceToHost, h->stream);
        const hipError_t drained = hipStreamSynchronize(h->stream);
        if (e == hipSuccess) what = "hipStreamSynchronize", e = drained;
    }
    free_dev(dcases);
    free_dev(dact);
    free_dev(dout);
    if (e != hipSuccess) return fail(h, RT_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
    return RT_OK;
}

int rt_test_sweep(rt_handle* h, int which, uint64_t* out3) {
    if (!h || !out3 || which < 0 || which > 4) return fail(h, RT_ERR_INVALID_ARGUMENT, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    unsigned long long* d = nullptr;
    HIP_TRY(h, hipMalloc((void**)&d, 3 * sizeof(unsigned long long)));
    HIP_TRY(h, hipMemsetAsync(d, 0, 3 * sizeof(unsigned long long), h->stream));
    HIP_TRY(h, launch_sweep(which, d, h->stream));
    HIP_TRY(h, hipMemcpyAsync(out3, d, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    free_dev(d);
    return RT_OK;
}

int rt_test_device_sample_texture(rt_handle* h, const rt_texture_desc* tex, const float* uv, float* rgba_out, uint64_t n) {
    if (!h || !tex || !tex->rgba8 || !uv || !rgba_out || tex->width == 0 || tex->height == 0)
        return fail(h, RT_ERR_INVALID_ARGUMENT, "bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    uint8_t* dt = nullptr;
    float *duv = nullptr, *dout = nullptr;
    const size_t tb = (size_t)tex->width * tex->height * 4;
    HIP_TRY(h, hipMalloc((void**)&dt, tb));
    HIP_TRY(h, hipMalloc((void**)&duv, (size_t)(n ? n : 1) * 2 * sizeof(float)));
    HIP_TRY(h, hipMalloc((void**)&dout, (size_t)(n ? n : 1) * 4 * sizeof(float)));
    HIP_TRY(h, hipMemcpyAsync(dt, tex->rgba8, tb, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(duv, uv, n * 2 * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, launch_units_texture(dt, tex->width, tex->height, h->srgb_lut, duv, dout, n, h->stream));
    HIP_TRY(h, hipMemcpyAsync(rgba_out, dout, n * 4 * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    free_dev(dt);
    free_dev(duv);
    free_dev(dout);
    return RT_OK;
}

// Test-only: raw copies of the wavefront sequence's buffers after the last launch (0 path state, 1 hit records,
// 2 the two slot lists, 3 the per-round list counts), for tests/tools that check the sequence slot by slot.
int rt_test_read_wavefront(rt_handle* h, int which, void* out, uint64_t bytes) {
    if (!h || !out) return fail(h, RT_ERR_INVALID_ARGUMENT, "null argument");
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const size_t blocks = h->wf_capacity / 64;
    const void* src = nullptr;
    size_t have = 0;
    switch (which) {
        case 0: src = h->wf_state; have = blocks * WF_STATE_PLANES * 64 * sizeof(float4); break;
        case 1: src = h->wf_hit; have = blocks * WF_HIT_PLANES * 64 * sizeof(float4); break;
        case 2: src = h->wf_lists; have = 2 * h->wf_capacity * sizeof(uint32_t); break;
        case 3: src = h->wf_counts; have = h->wf_counts_capacity * sizeof(uint32_t); break;
        case 4: src = h->park_counts; have = h->park_counts ? 72 * sizeof(uint32_t) : 0; break;
        case 5: case 6:   // the park records of the last sequence's even / odd rounds (rt_device.h: PARK_PLANES)
            src = h->park_queue[which - 5];
            have = src ? ((h->park_capacity + 63) / 64) * (size_t)PARK_PLANES * 64u * sizeof(float4) : 0;
            break;
        default: return fail(h, RT_ERR_INVALID_ARGUMENT, "which must be 0..6");
    }
    if (!src || bytes > have) return fail(h, RT_ERR_INVALID_ARGUMENT, "no wavefront buffer of that size");
    HIP_TRY(h, hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return RT_OK;
}

// Test-only, no GPU needed: the automatic depth of option "frame_ahead" (rt2::ahead_depth) for a one-frame call that continues
// an accumulation -- scene staged in LDS or read from global memory, texels of the call's share, samples per pixel, bounces,
// and whether the host counts as one that waits for its frames.  tests/test_frame_ahead_policy.py pins the documented
// figures with it.
int rt_test_frame_ahead_depth(int lds_scene, uint64_t texels, int rays_per_pixel, int number_of_bounces, int host_waits) {
    rt_params p{};
    p.rays_per_pixel = rays_per_pixel;
    p.number_of_bounces = number_of_bounces;
    p.frames = 1;
    return (int)rt2::ahead_depth(rt2::Options{}, p, false, false, lds_scene != 0, texels, host_waits != 0);
}

// Test-only, no device and no handle (tests/test_options_host.py): row `index` of the option table, and the setter on a
// fresh set of options.
int rt_test_option_table(uint32_t index, char name_out[RT_TEST_OPTION_NAME_BYTES], int32_t info_out[4]) {
    static_assert(RT_TEST_OPT_BOOLEAN == rt2::OPT_BOOLEAN && RT_TEST_OPT_UPLOAD == rt2::OPT_UPLOAD && RT_TEST_OPT_EXPERIMENT == rt2::OPT_EXPERIMENT &&
                      RT_TEST_OPT_DROPS_PRIMARY == rt2::OPT_DROPS_PRIMARY && RT_TEST_OPT_RESETS_TILES == rt2::OPT_RESETS_TILES &&
                      RT_TEST_OPT_CLEARS_AHEAD_FAILED == rt2::OPT_CLEARS_AHEAD_FAILED && RT_TEST_OPT_ONE_IS_AUTO == rt2::OPT_ONE_IS_AUTO &&
                      RT_TEST_OPT_NOT_ONE == rt2::OPT_NOT_ONE,
                  "include/rt_test_abi.h repeats the flags of host/launch_options.h");
    const rt2::OptionRow* row = rt2::option_row(index);
    if (!row || !name_out || !info_out || strlen(row->name) >= RT_TEST_OPTION_NAME_BYTES) return RT_ERR_INVALID_ARGUMENT;
    rt2::Options fresh;
    strcpy(name_out, row->name);
    const int32_t info[4] = {row->lo, row->hi, row->at(fresh), (int32_t)row->flags};
    memcpy(info_out, info, sizeof(info));
    return RT_OK;
}
int rt_test_set_option(const char* name, int value, int32_t stored_out[2]) {
    if (!name || !stored_out) return RT_ERR_INVALID_ARGUMENT;
    rt2::Options opt;
    const rt2::SetResult r = rt2::set_option(opt, name, value);
    stored_out[0] = r.row ? r.row->at(opt) : 0;
    stored_out[1] = (int32_t)r.effects;
    return r.code() == RT_OK ? RT_OK : fail(nullptr, r.code(), r.error);
}

// Test-only, no device and no handle (tests/test_launch_rules_host.py): one launch rule of host/launch_options.h on the
// option values given (what rt_test_set_option stored for them).
int rt_test_launch_rule(int which, const int64_t in[8], int64_t out[2]) {
    if (!in || !out) return RT_ERR_INVALID_ARGUMENT;
    rt2::Options opt;
    uint32_t a = 0, b = 0;
    switch (which) {
        case RT_TEST_RULE_VOTES:
            opt.vote_eighths = (int)in[0];
            opt.vote_patience = (int)in[1];
            rt2::vote_thresholds(opt, in[2] != 0, in[3] != 0, a, b);
            break;
        case RT_TEST_RULE_ROUNDS: a = rt2::automatic_rounds((size_t)in[0], (int)in[1], (uint32_t)in[2]); break;
        case RT_TEST_RULE_VARIANT:
            opt.kernel_variant = (int)in[0];
            opt.persistent_blocks = (int)in[1];
            a = rt2::kernel_variant_for(opt, (uint64_t)in[2], (uint32_t)in[3], in[4] != 0);
            break;
        case RT_TEST_RULE_DEPTH:
            opt.pipeline = (int)in[0];
            a = (uint32_t)rt2::pipeline_depth(opt, (int)in[1], (uint32_t)in[2]);
            break;
        case RT_TEST_RULE_BATCH: a = in[1] >= 1 ? rt2::equal_batch((uint32_t)in[0], (uint32_t)in[1]) : 0u; break;
        case RT_TEST_RULE_GRID:
            opt.persistent_blocks = (int)in[1];
            a = rt2::blocks_per_cu_for((size_t)in[0]);
            b = rt2::persistent_blocks_for(opt, (size_t)in[0]);
            break;
        case RT_TEST_RULE_FRAME_GROUP:
            a = rt2::frame_group_for((uint32_t)in[0], (uint64_t)in[1], (uint32_t)in[2], in[3] != 0, in[4] != 0, in[5] != 0);
            b = rt2::FRAME_GROUP_CAP;
            break;
        case RT_TEST_RULE_FRAME_GROUP_TAPERED:
            a = rt2::frame_group_tapered_for((uint32_t)in[0], (uint64_t)in[1], (uint32_t)in[2], in[3] != 0, in[4] != 0, in[5] != 0);
            b = rt2::FRAME_GROUP_CAP_TAPERED | rt2::FRAME_GROUP_MIN_ITEMS_PER_WAVE_TAPERED << 16;
            break;
        case RT_TEST_RULE_FRAME_TAPER: {
            static_assert(RT_TEST_TAPER_WORDS == rt2::TAPER_WORDS, "include/rt_test_abi.h: the taper table");
            // (in[6]: the address of n_tiles costs followed by room for the table)
            uint32_t* words = (uint32_t*)(uintptr_t)in[6];
            const uint32_t n_tiles = (uint32_t)in[5];
            if (!words || in[5] < 0 || in[5] > (1ll << 24)) return fail(nullptr, RT_ERR_INVALID_ARGUMENT, "frame taper rule: costs and at most 2^24 tiles");
            uint32_t count[rt2::TAPER_BINS];
            unsigned long long weight[rt2::TAPER_BINS];
            rt2::frame_taper_histogram(words, n_tiles, (uint32_t)in[3], (uint32_t)in[4], count, weight);
            b = in[7] > 0 ? (uint32_t)in[7] : rt2::FRAME_TAPER_ALPHA;
            rt2::frame_taper_table(count, weight, rt2::TAPER_BINS, (uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2], b, words + n_tiles);
            a = words[n_tiles];
            break;
        }
        case RT_TEST_RULE_TERMINAL_SKIP: {
            // (in[0]: the address of a packed blob -- rt_test_pack_scene's --, in[1]: of its 12 layout words, in[7]: of three floats)
            const rt2::Quad* head = (const rt2::Quad*)(uintptr_t)in[0];
            const uint32_t* words = (const uint32_t*)(uintptr_t)in[1];
            float* c_out = (float*)(uintptr_t)in[7];
            if (!head || !words || !c_out || in[2] < 0 || in[3] < 0) return fail(nullptr, RT_ERR_INVALID_ARGUMENT, "terminal skip rule: a blob, its layout, room for terminal_c");
            SceneLayout lay;
            static_assert(sizeof(lay) == 12 * sizeof(uint32_t), "SceneLayout: 12 words");
            memcpy(&lay, words, sizeof(lay));
            const rt2::TerminalScene t = rt2::terminal_skip_scene(head, lay, (uint32_t)in[2], (uint32_t)in[3]);
            a = rt2::terminal_skip_for(t, in[4] != 0, false, in[5] != 0, in[6] != 0, false);
            b = t.dark;
            for (int k = 0; k < 3; ++k) c_out[k] = a != 0u ? t.c[k] : 0.0f;
            a = a != 0u ? 1u : 0u;
            break;
        }
        default: return fail(nullptr, RT_ERR_INVALID_ARGUMENT, "unknown rule");
    }
    out[0] = a;
    out[1] = b;
    return RT_OK;
}

// Test-only: the terminal skip of handle `h` (RenderArgs::terminal_dark).  on >= 0 switches it for the handle's later
// launches (1: rt2::terminal_skip_for decides, the default; 0: no launch skips); last_out: the mask the handle's last
// render launch ran with (0: it skipped nothing) and the bits of its terminal_c.
int rt_test_terminal_skip(rt_handle* h, int on, uint32_t last_out[4]) {
    if (!h) return RT_ERR_INVALID_ARGUMENT;
    if (on >= 0) h->terminal_skip_on = on != 0;
    if (last_out) {
        last_out[0] = h->last_terminal_dark;
        for (int k = 0; k < 3; ++k) {
            const float c = h->last_terminal_dark != 0u ? h->terminal.c[k] : 0.0f;
            memcpy(&last_out[1 + k], &c, 4);
        }
    }
    return RT_OK;
}

// Test-only: the fixed switches of handle `h` (rt2::FixedSwitches).  on >= 0 switches them for the handle's later launches
// (1: rt2::fixed_switches_ok decides, the default; 0: every launch runs the general kernel); last_out: 1 if the handle's
// last render launch ran the FIXED instantiation (rt_last_launch out[3] & 32).
int rt_test_fixed_switches(rt_handle* h, int on, uint32_t* last_out) {
    if (!h) return RT_ERR_INVALID_ARGUMENT;
    if (on >= 0) h->fixed_switches_on = on != 0;
    if (last_out) *last_out = (h->last_launch[3] & 32u) != 0u ? 1u : 0u;
    return RT_OK;
}

// Test-only: rt2::fixed_switches_ok on host-given values, and the constants of rt2::FixedSwitches beside the answer.
int rt_test_fixed_switches_rule(const int64_t in[RT_TEST_FIXED_SWITCHES], int64_t out[2 + RT_TEST_FIXED_SWITCHES]) {
    if (!in || !out) return fail(nullptr, RT_ERR_INVALID_ARGUMENT, "null argument");
    using F = rt2::FixedSwitches;
    const rt2::FixedSwitchValues v{(uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2], (uint32_t)in[3], (uint32_t)in[4], (uint32_t)in[5],
                                   (uint32_t)in[6], (uint32_t)in[7], (int32_t)in[8], (int32_t)in[9], (uint32_t)in[10], (uint32_t)in[11],
                                   (uint32_t)in[12], (uint32_t)in[13], (uint32_t)in[14]};
    const int64_t constants[RT_TEST_FIXED_SWITCHES] = {F::stack_wide, F::forest_cull, F::roulette_skip, F::fast_miss, F::terminal_dark, F::pixel_cache,
                                                        F::primary, F::primary_complete, F::skybox, F::samples, F::spp_reciprocal, F::strip_world,
                                                        F::batch, F::batch_tile_major, F::grouped};
    out[0] = (rt2::fixed_switches_ok(v, true) ? 1 : 0) | (rt2::fixed_switches_ok(v, false) ? 2 : 0);
    out[1] = RT_FIXED_SWITCHES;
    for (int k = 0; k < RT_TEST_FIXED_SWITCHES; ++k) out[2 + k] = constants[k];
    return RT_OK;
}

// Test-only: the frame groups of handle `h` (RenderArgs::frame_group).  force >= 0 sets the group size of its later batches
// (0: rt2::frame_group_for decides, and rt2::frame_group_tapered_for for a launch that carries a taper table; an order or a
// launch sequence that takes no groups still gets 1, as does a library
// built with -DRT_FRAME_GROUP=1); last_out: the group size of the handle's last launch.
int rt_test_frame_group(rt_handle* h, int force, uint32_t* last_out) {
    if (!h || force > (int)RT_MAX_BATCH_FRAMES) return fail(h, RT_ERR_INVALID_ARGUMENT, "frame group: -1 (leave), 0 (the rule), 1..64");
    if (force >= 0) h->frame_group_forced = (uint32_t)force;
    if (last_out) *last_out = h->last_frame_group;
    return RT_OK;
}

// Test-only: the taper of handle `h` (RenderArgs::frame_taper).  n_segments >= 1 forces the segments {first_rank[k],
// size[k]} on its later grouped batches, bypassing the rule; 0 gives the rule its say again; < 0 changes nothing.
// table_out: the table the handle's last launch ran with, zeros if it ran untapered.
int rt_test_frame_taper(rt_handle* h, int n_segments, const uint32_t* first_rank, const uint32_t* size, uint32_t* table_out) {
    if (!h) return RT_ERR_INVALID_ARGUMENT;
    if (n_segments > (int)rt2::TAPER_MAX_SEGMENTS || (n_segments > 0 && (!first_rank || !size)))
        return fail(h, RT_ERR_INVALID_ARGUMENT, "frame taper: at most 8 segments, each with a first rank and a group size");
    if (n_segments >= 0) {
        std::vector<uint32_t> forced;
        for (int k = 0; k < n_segments; ++k) {
            if (first_rank[k] < (k ? first_rank[k - 1] : 0u) || (k == 0 && first_rank[0] != 0u) || size[k] < 1u || size[k] > RT_MAX_BATCH_FRAMES)
                return fail(h, RT_ERR_INVALID_ARGUMENT, "frame taper: first ranks ascending from 0, group sizes 1..64");
            forced.push_back(first_rank[k]);
            forced.push_back(size[k]);
        }
        h->taper_forced = forced;
    }
    if (table_out) {
        memset(table_out, 0, rt2::TAPER_WORDS * sizeof(uint32_t));
        if (int rc = rt_synchronize(h); rc != RT_OK) return rc;
        if (h->last_taper) HIP_TRY(h, hipMemcpy(table_out, h->last_taper, rt2::TAPER_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    return RT_OK;
}

// Test-only: the device's evaluation of the taper rule (rt_frame_taper_kernel) on n_tiles host-given tile costs -- what
// tile_feedback launches behind a new tile order, with every input the caller's.
int rt_test_frame_taper_rule(rt_handle* h, const uint32_t* cost, uint32_t n_tiles, uint32_t max_cost, uint32_t cost_floor, uint32_t n_batch,
                             uint32_t head, uint32_t waves, uint32_t alpha, uint32_t* table_out) {
    if (!h || !table_out || (n_tiles && !cost)) return fail(h, RT_ERR_INVALID_ARGUMENT, "null argument");
    if (n_tiles > (1u << 24) || head > RT_MAX_BATCH_FRAMES || n_batch > RT_MAX_BATCH_FRAMES)
        return fail(h, RT_ERR_INVALID_ARGUMENT, "frame taper rule: at most 2^24 tiles, 64 frames");
    HIP_TRY(h, hipSetDevice(h->device));
    uint32_t* dev = nullptr;
    HIP_TRY(h, hipMalloc((void**)&dev, ((size_t)n_tiles + rt2::TAPER_WORDS) * sizeof(uint32_t)));
    hipError_t e = n_tiles ? hipMemcpy(dev + rt2::TAPER_WORDS, cost, (size_t)n_tiles * sizeof(uint32_t), hipMemcpyHostToDevice) : hipSuccess;
    if (e == hipSuccess) e = launch_frame_taper(dev + rt2::TAPER_WORDS, n_tiles, max_cost, cost_floor, n_batch, head, waves, alpha, dev, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) e = hipMemcpy(table_out, dev, rt2::TAPER_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost);
    free_dev(dev);
    HIP_TRY(h, e);
    return RT_OK;
}

// Test-only: the rays per tile that the handle's last cost-recording launch counted (tile_feedback: the first frame of a
// batch, or the single frame), n_tiles of them, once everything queued on the handle is done.
int rt_test_tile_costs(rt_handle* h, uint32_t* out, uint32_t n_tiles) {
    if (!h || !out) return fail(h, RT_ERR_INVALID_ARGUMENT, "null argument");
    if (!h->tile_cost[h->tiles.cost_slot]) return fail(h, RT_ERR_INVALID_ARGUMENT, "the handle has no tile-cost tables");
    if (n_tiles > h->tile_capacity) return fail(h, RT_ERR_INVALID_ARGUMENT, "more tiles than the handle's frame size has");
    if (int rc = rt_synchronize(h); rc != RT_OK) return rc;
    HIP_TRY(h, hipMemcpy(out, h->tile_cost[h->tiles.cost_slot], (size_t)n_tiles * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RT_OK;
}

// Test-only: the grouped gather of rt_render_multi against the RCCL-shaped library at `lib_path`, on fake buffers and
// with no HIP call (so that it runs on a machine without a GPU): n_ranks communicators from ncclCommInitAll, one
// rccl_grouped_gather over them; on failure the communicators are aborted, as render_multi_impl does.  The error text
// goes to rt_last_error(NULL).  tests/test_rccl_group.py drives it against tests/cpp/fake_rccl.c.
int rt_test_rccl_gather(const char* lib_path, int n_ranks) {
    if (!lib_path || n_ranks < 1 || n_ranks > 64) return fail(nullptr, RT_ERR_INVALID_ARGUMENT, "bad arguments");
    RcclApi api;
    if (!api.load(lib_path)) return fail(nullptr, RT_ERR_IO, api.why);
    std::vector<ncclComm_t> comms((size_t)n_ranks);
    std::vector<int> devs((size_t)n_ranks);
    for (int r = 0; r < n_ranks; ++r) devs[(size_t)r] = r;
    ncclResult_t r0 = api.CommInitAll(comms.data(), n_ranks, devs.data());
    if (r0 != ncclSuccess) {
        const std::string why = std::string("ncclCommInitAll: ") + api.GetErrorString(r0);
        api.unload();
        return fail(nullptr, RT_ERR_DEVICE, why);
    }
    static float fake_send[64][4], fake_recv[64][4];
    std::vector<GatherLeg> legs;
    for (int r = 0; r < n_ranks; ++r)
        legs.push_back(GatherLeg{fake_send[r], fake_recv[r], 4, r, r, comms[(size_t)r], nullptr});
    std::string gerr;
    const bool ok = rccl_grouped_gather(api, legs, 0, comms[0], nullptr, [](int, std::string&) { return 0; }, gerr);
    for (ncclComm_t c : comms) {
        if (ok) (void)api.CommDestroy(c);
        else api.drop(c);
    }
    api.unload();
    return ok ? RT_OK : fail(nullptr, RT_ERR_DEVICE, "rt_render_multi gather: " + gerr);
}

// Test-only: find_best_split for host-given nodes through a LevelSearch -- the host one (device -1, no GPU needed) or
// the kernels of rt_bvh_search.hip --, the levels in turn through one search object, as bvh_build_levels drives it.
// tests/test_bvh_search_host.py, tests/test_gpu_bvh_search.py.
int rt_test_sah_search(int device, const float* tri9, uint64_t n, const uint32_t* order, const rt_test_sah_query* queries,
                       const uint32_t* level_counts, uint32_t n_levels, rt_test_sah_result* out) {
    if (device < -1) return fail(nullptr, RT_ERR_INVALID_ARGUMENT, "device must be -1 (host search) or a device ordinal");
    if (n == 0 || n > RT_MAX_TRIANGLES || !tri9 || !order) return fail(nullptr, RT_ERR_INVALID_ARGUMENT, "no triangles, or too many");
    if (n_levels && !level_counts) return fail(nullptr, RT_ERR_INVALID_ARGUMENT, "null level_counts");
    uint64_t total = 0;
    for (uint32_t l = 0; l < n_levels; ++l) total += level_counts[l];
    if (total && (!queries || !out)) return fail(nullptr, RT_ERR_INVALID_ARGUMENT, "null queries or results");
    for (uint64_t p = 0; p < n; ++p)
        if (order[p] >= n) return fail(nullptr, RT_ERR_INVALID_ARGUMENT, "order[" + std::to_string(p) + "] is not a triangle id");
    for (uint64_t k = 0; k < total; ++k) {
        if (queries[k].count < 2)
            return fail(nullptr, RT_ERR_INVALID_ARGUMENT, "query " + std::to_string(k) + ": count < 2 (the builder never searches such a node)");
        if ((uint64_t)queries[k].start + queries[k].count > n)
            return fail(nullptr, RT_ERR_INVALID_ARGUMENT, "query " + std::to_string(k) + ": start + count exceeds the " + std::to_string(n) + " triangles");
    }
    try {
        const rt2::LevelSearch search = device >= 0 ? rt2::make_device_level_search(device, tri9, (size_t)n)
                                                    : rt2::make_host_level_search(tri9, (size_t)n);
        std::vector<rt2::SplitQuery> qs;
        std::vector<rt2::SplitResult> rs;
        uint64_t base = 0;
        for (uint32_t l = 0; l < n_levels; ++l) {
            qs.resize(level_counts[l]);
            for (uint32_t k = 0; k < level_counts[l]; ++k) {
                const rt_test_sah_query& q = queries[base + k];
                qs[k].start = q.start;
                qs[k].count = q.count;
                memcpy(qs[k].aabb_min, q.aabb_min, 12);
                memcpy(qs[k].aabb_max, q.aabb_max, 12);
            }
            search(order, (size_t)n, qs, rs);
            for (uint32_t k = 0; k < level_counts[l]; ++k) out[base + k] = rt_test_sah_result{rs[k].axis, rs[k].pos, rs[k].cost};
            base += level_counts[l];
        }
    } catch (const std::exception& e) {   // (as rt_scene_build_device sorts them)
        return fail(nullptr, strncmp(e.what(), "HIP", 3) == 0 ? RT_ERR_DEVICE : RT_ERR_OUT_OF_MEMORY, e.what());
    }
    return RT_OK;
}
#endif  // RT_TEST_ENTRIES

void* rt_device_image(rt_handle* h) { return h ? (void*)h->image : nullptr; }
void* rt_stream(rt_handle* h) { return h ? (void*)h->stream : nullptr; }

}  // extern "C"
