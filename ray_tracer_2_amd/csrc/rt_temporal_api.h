// rt_temporal_api.h -- what the units of temporal accumulation declare to each other (include/rt_abi.h:
// rt_temporal_accumulate, rt_temporal_accumulate_host and their _moving and _deforming forms): the kind of a call, the argument
// rules, the once-per-call numbers and the host restatement (host/temporal.cpp), and the one argument struct of the device
// launch (rt_temporal.hip), all called by the entry points in rt_api_frames.hip.  The arithmetic they share is csrc/rt_temporal.h.
#ifndef RT_TEMPORAL_API_H
#define RT_TEMPORAL_API_H

#include <stddef.h>
#include <stdint.h>

#include <string>

#include "rt_abi.h"
#include "rt_temporal.h"

namespace rt2 {
// The three calls are one call with optional parts: rt_temporal_motion_desc is rt_temporal_desc with the table behind it,
// rt_temporal_deform_desc that with the triangle side behind it.  Inside the units a desc of any kind is a zero-filled
// rt_temporal_deform_desc (temporal_check widens it) and the kind; a part the kind does not have is null or zero.
enum class TemporalKind { PLAIN, MOVING, DEFORMING };
static_assert(offsetof(rt_temporal_motion_desc, motions) == sizeof(rt_temporal_desc) && sizeof(rt_temporal_motion_desc) == sizeof(rt_temporal_desc) + 16,
              "rt_temporal_motion_desc is rt_temporal_desc and the table");
static_assert(offsetof(rt_temporal_deform_desc, primitive) == sizeof(rt_temporal_motion_desc) &&
                  sizeof(rt_temporal_deform_desc) == sizeof(rt_temporal_motion_desc) + 40,
              "rt_temporal_deform_desc is rt_temporal_motion_desc and the triangle side");
static_assert(sizeof(rt_object_motion) == 96 && sizeof(rttp::Motion) == 96 && offsetof(rt_object_motion, nt) == offsetof(rttp::Motion, nt) &&
              offsetof(rt_object_motion, moved) == offsetof(rttp::Motion, moved), "rttp::Motion is rt_object_motion");
static_assert(sizeof(rt_packed_triangle) == 96 && sizeof(rttp::Tri) == 96 && offsetof(rt_packed_triangle, v2) == offsetof(rttp::Tri, v2) &&
                  offsetof(rt_packed_triangle, n1) == offsetof(rttp::Tri, n1) && offsetof(rt_packed_triangle, n3) == offsetof(rttp::Tri, n3),
              "rttp::Tri is rt_packed_triangle");
static_assert(rttp::HIT_BACKFACE == RT_HIT_BACKFACE, "the flags plane's backface bit");

// RT_OK and `desc` -- the kind's rt_temporal_desc, rt_temporal_motion_desc or rt_temporal_deform_desc -- widened into
// `wide`, or the error of a desc that the kind's rt_temporal_accumulate* (device == true: host_memory says which path, color
// may be NULL without it) or rt_temporal_accumulate*_host (device == false) refuses, with its reason in `err`: the plain
// rules, then the table's (on device memory the table is 16-byte aligned), then the triangle side's (on device memory:
// primitive and bary 4-byte aligned, prev_triangles 16).  Nothing is dereferenced but the desc.
int temporal_check(const void* desc, TemporalKind kind, bool device, bool host_memory, rt_temporal_deform_desc& wide, std::string& err);
// The once-per-call numbers of a checked desc: V = mat4_inverse(prev_camera.cam_to_world) (host/glam_math.h), view_params.
rttp::Call temporal_call(const rt_temporal_deform_desc& d);
int temporal_host(const rt_temporal_desc* d, std::string& err);
int temporal_motion_host(const rt_temporal_motion_desc* d, std::string& err);
int temporal_deform_host(const rt_temporal_deform_desc* d, std::string& err);
}  // namespace rt2

namespace rtd {
// The arguments of the three kernels.  The table (16-byte aligned) is there for the moving and deforming kinds, the current
// G-buffer's triangle planes and the previous triangles [tri_first, tri_first + n_prev_triangles) of the uploaded array
// (16-byte aligned) for the deforming kind; a kernel reads the parts of its kind only.
struct TemporalArgs {
    rttp::Call call;
    const float* color;          // [h][w][4]
    const float* point;          // [h][w][3]
    const float* normal;         // [h][w][3]
    const uint32_t* object;      // [h][w]; may be null for the plain kind
    const float* prev_color;     // [h][w][4]
    const float* prev_history;   // [h][w]
    const float* prev_point;     // [h][w][3]
    const float* prev_normal;    // [h][w][3]
    const uint32_t* prev_object; // [h][w] or null
    float* out;                  // [h][w][4]; may be `color`
    float* out_history;          // [h][w]
    float* motion;               // [h][w][2] or null
    const rttp::Motion* motions;       // [n_objects]
    const uint32_t* primitive;         // [h][w]
    const float* bary;                 // [h][w][2]
    const uint8_t* flags;              // [h][w]
    const rttp::Tri* prev_triangles;   // [n_prev_triangles]
    uint32_t n_objects, tri_first, n_prev_triangles;
};
}  // namespace rtd

#endif
