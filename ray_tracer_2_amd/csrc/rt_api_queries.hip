// rt_api_queries.hip -- the calls of include/rt_abi.h that trace rays the caller supplies, or a frame's first hits, on the
// uploaded scene: rt_intersect_rays, rt_occluded_rays, rt_pick, rt_render_gbuffer, rt_radiance_rays.  A unit of the
// device-side C ABI over rt_handle.h; rt_api.hip has the handle's lifecycle and the render path.
#include <algorithm>
#include <string>

#include "rt_handle.h"

extern "C" {

// ---- ray queries (include/rt_abi.h: rt_intersect_rays, rt_occluded_rays, rt_pick; rt_queries.inl: rt_query_kernel) ----
// A query launch takes the arguments a render of the scene takes (scene_args), no pixel memo, and the render's
// persistent grid (workgroups that fit the CUs' LDS).  It reads nothing but the scene and writes nothing but its output:
// the image, the tables, the pipeline slots and the counters are not touched.
static_assert(sizeof(rt_ray) == 32 && sizeof(rt_hit) == 64, "rt_ray / rt_hit layout");

// The arguments of a launch on the scene outside a render (queries, rt_pick, rt_render_gbuffer, the test probe): what a
// render of the scene takes (scene_args), the handle's camera, and the caller's frame parameters or none.
extern "C++" RenderArgs rth::query_args(const rt_handle* h, const rt_params* params) {
    RenderArgs a{};
    scene_args(h, a);
    a.params = params ? *params : rt_params{};
    a.camera = h->camera;
    return a;
}

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

}  // extern "C"
