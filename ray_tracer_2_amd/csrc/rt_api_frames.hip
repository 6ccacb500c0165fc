// rt_api_frames.hip -- the calls of include/rt_abi.h that work on a rendered frame and launch no render kernel: the
// denoisers, adaptive sampling, temporal accumulation, history rectification, guided upsampling, the display pass and the
// exposure meter, each with its _host restatement.  A unit of the device-side C ABI over rt_handle.h; rt_api.hip has the handle's lifecycle and the
// render path.
#include <new>
#include <string>

#include "rt_handle.h"
#include "rt_denoise_api.h"  // (the denoiser: its argument rules and host restatement, host/denoise.cpp; its launch, rt_denoise.hip)
#include "rt_upsample_api.h"  // (guided upsampling: its argument rules and host restatement, host/upsample.cpp; its launch, rt_upsample.hip)
#include "rt_display_api.h"  // (the display pass and the exposure meter: their argument rules and host restatements, host/display.cpp; their launches, rt_display.hip)
#include "rt_temporal_api.h"  // (temporal accumulation: its argument rules and host restatement, host/temporal.cpp; its launch, rt_temporal.hip)
#include "rt_rectify_api.h"  // (history rectification: its argument rules and host restatement, host/rectify.cpp; its launch, rt_rectify.hip)
#include "rt_vdenoise_api.h"  // (the variance-guided denoiser: its argument rules and host restatement, host/vdenoise.cpp; its launches, rt_vdenoise.hip)
#include "rt_adaptive_api.h"  // (adaptive sampling: its argument rules and host restatement, host/adaptive.cpp; its launches, rt_adaptive.hip)

extern "C" {

// ---- the passes over a rendered frame: rt_denoise, rt_denoise_variance / rt_luminance_moments, rt_adaptive_plan /
// rt_adaptive_merge, rt_temporal_accumulate / rt_temporal_accumulate_moving / rt_temporal_accumulate_deforming, rt_upsample,
// rt_display, rt_auto_exposure, rt_temporal_rectify ----
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
int rt_temporal_rectify_host(const rt_rectify_desc* desc) { return host_call(rt2::rectify_host, desc); }
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

// ---- history rectification (include/rt_abi.h: rt_temporal_rectify; rt_rectify.hip; host/rectify.cpp) ----
// No scratch is kept.  out, out_history and out_moments take the places of history, history_length and history_moments in
// the staging buffer.  A NULL color names the image read-only: `out` inside the texels the pass reads is refused like an
// `out` that overlaps the caller's own color.
int rt_temporal_rectify(rt_handle* h, const rt_rectify_desc* desc, int flags) {
    if (!h) return fail(h, RT_ERR_INVALID_ARGUMENT, "null handle");
    if (flags & ~RT_RECTIFY_HOST_MEMORY) return fail(h, RT_ERR_INVALID_ARGUMENT, "unknown flags");
    const bool host = (flags & RT_RECTIFY_HOST_MEMORY) != 0;
    std::string err;
    if (const int rc = rt2::rectify_check(desc, true, host, err); rc != RT_OK) return fail(h, rc, err);
    const size_t texels = (size_t)desc->width * desc->height;
    const float* color = desc->color;
    if (int rc = frame_color(h, color, texels); rc != RT_OK) return rc;
    if (!desc->color && rt2::rectify_overlap(desc->out, color, texels))
        return fail(h, RT_ERR_INVALID_ARGUMENT, "out overlaps the image, which color = NULL names and the neighbouring texels read");
    HIP_TRY(h, hipSetDevice(h->device));
    if (int rc = host ? RT_OK : image_access(h, color, desc->out); rc != RT_OK) return rc;
    const FramePlane planes[7] = {{color, nullptr, texels * 16u}, {desc->history, desc->out, texels * 16u},
                                  {desc->history_length, desc->out_history, texels * 4u}, {desc->object, nullptr, texels * 4u},
                                  {desc->moments, nullptr, texels * 16u}, {desc->history_moments, desc->out_moments, texels * 16u},
                                  {nullptr, desc->out_clipped, texels}};
    RectifyArgs a{};
    a.call = rt2::rectify_call(*desc);
    return frame_call(h, host, planes, "the staging planes of history rectification", "launch_rectify", [&](const void* const* in, void* const* out) {
        a.color = (const float*)in[0]; a.history = (const float*)in[1]; a.out = (float*)out[1];
        a.history_length = (const float*)in[2]; a.out_history = (float*)out[2]; a.object = (const uint32_t*)in[3];
        a.moments = (const float*)in[4]; a.history_moments = (const float*)in[5]; a.out_moments = (float*)out[5];
        a.out_clipped = (uint8_t*)out[6];
        return launch_rectify(a, h->stream);
    });
}

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

}  // extern "C"
