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
#include "rt_display_api.h"  // (the display pass and the exposure meter: their argument rules and host restatements, host/display.cpp; their launches, rt_display.hip)
#include "rt_rccl.h"  // (types of <rccl/rccl.h>; the library itself is loaded on first multi-device use)
#include "rt_srgb_lut.h"
#include "rt_handle.h"  // (the handle, the launch declarations and what the four units of the ABI share)

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

}  // namespace
namespace rth {
int fail(rt_handle* h, int code, const std::string& msg) {
    if (h) h->err = msg;
    g_err = msg;
    return code;
}
}  // namespace rth
namespace {

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
}  // namespace
namespace rth {
// may the handle take `extra` more bytes (after giving back `freed` of what it holds)?
bool fits_cap(const rt_handle* h, size_t extra, size_t freed) {
    if (h->opt.max_device_mb == 0) return true;
    const size_t held = optional_bytes(h);
    return (held > freed ? held - freed : 0) + extra <= h->opt.max_device_bytes();
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
}  // namespace rth
namespace {

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

}  // namespace
namespace rth {
// Every launch enqueued so far on any of the handle's streams is complete (they all may read the blob).
int drain_streams(rt_handle* h) {
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (PipeSlot& ps : h->pipe)
        if (ps.stream) HIP_TRY(h, hipStreamSynchronize(ps.stream));
    return RT_OK;
}
}  // namespace rth
namespace {

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
extern "C++" int rth::wait_pending_copy(rt_handle* h) {
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
extern "C++" void rth::scene_args(const rt_handle* h, RenderArgs& a) {
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

// Device memory a host-memory call may stage through: at most 64 MB, within what option max_device_mb leaves.
extern "C++" size_t rth::staging_room(const rt_handle* h) {
    size_t room = (size_t)64 << 20;
    if (h->opt.max_device_mb != 0) {
        const size_t held = optional_bytes(h);
        room = std::min(room, h->opt.max_device_bytes() > held ? h->opt.max_device_bytes() - held : 0);
    }
    return room;
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

void* rt_device_image(rt_handle* h) { return h ? (void*)h->image : nullptr; }
void* rt_stream(rt_handle* h) { return h ? (void*)h->stream : nullptr; }

}  // extern "C"
