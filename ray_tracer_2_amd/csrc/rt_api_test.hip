// rt_api_test.hip -- the test library's entry points (include/rt_test_abi.h).  A unit of the device-side C ABI over
// rt_handle.h that every build compiles: to an empty object unless -DRT_TEST_ENTRIES=1.
#ifndef RT_TEST_ENTRIES
#define RT_TEST_ENTRIES 0
#endif
#if RT_TEST_ENTRIES
#include <cmath>
#include <cstring>
#include <exception>
#include <new>
#include <string>
#include <vector>

#include "host/bvh.h"  // (rt2::LevelSearch: rt_test_sah_search)
#include "rt_handle.h"
#include "rt_rccl.h"  // (rccl_grouped_gather: rt_test_rccl_gather)
#include "../../include/rt_test_abi.h"

namespace rtd {
hipError_t launch_units(int fn, const float* x, const float* y, float* out, unsigned long long n, hipStream_t stream);
hipError_t launch_sweep(int which, unsigned long long* out, hipStream_t stream);
hipError_t launch_test_intersect(const RenderArgs& a, const float* ro, const float* rd, const uint8_t* active,
                                 unsigned long long n, bool simple, bool stats, uint32_t* out, hipStream_t stream);
hipError_t launch_units_texture(const uint8_t* rgba8, uint32_t width, uint32_t height, const float* srgb_lut, const float* uv,
                                float* out, unsigned long long n, hipStream_t stream);
hipError_t launch_test_shade(const RenderArgs& a, int which, const uint32_t* cases, const uint8_t* active, unsigned long long n,
                             bool simple, bool fast_miss, bool total_lds, uint32_t* out, hipStream_t stream);
}  // namespace rtd

extern "C" {

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

}  // extern "C"
#endif  // RT_TEST_ENTRIES
