// rt_temporal_api.h -- what the units of temporal accumulation declare to each other (include/rt_abi.h:
// rt_temporal_accumulate, rt_temporal_accumulate_host and their _moving and _deforming forms): the argument rules, the once-per-call
// numbers and the host restatement (host/temporal.cpp), and the arguments of the device launch (rt_temporal.hip), all called by the entry points
// in rt_api.hip.  The arithmetic they share is csrc/rt_temporal.h.
#ifndef RT_TEMPORAL_API_H
#define RT_TEMPORAL_API_H

#include <stddef.h>
#include <stdint.h>

#include <string>

#include "rt_abi.h"
#include "rt_temporal.h"

namespace rt2 {
// RT_OK, or the error of a desc that rt_temporal_accumulate (device == true: host_memory says which path, color may be NULL
// without it) or rt_temporal_accumulate_host (device == false) refuses, with its reason in `err`.  Nothing is dereferenced
// but the desc.
int temporal_check(const rt_temporal_desc* d, bool device, bool host_memory, std::string& err);
// The once-per-call numbers of a checked desc: V = mat4_inverse(prev_camera.cam_to_world) (host/glam_math.h), view_params.
rttp::Call temporal_call(const rt_temporal_desc* d);
int temporal_host(const rt_temporal_desc* d, std::string& err);

// The _moving forms.  rt_temporal_motion_desc is rt_temporal_desc with the table behind it: its head, as an rt_temporal_desc
// of its own (struct_bytes set), is what temporal_check and temporal_call are given.
static_assert(offsetof(rt_temporal_motion_desc, motions) == sizeof(rt_temporal_desc) && sizeof(rt_temporal_motion_desc) == sizeof(rt_temporal_desc) + 16,
              "rt_temporal_motion_desc is rt_temporal_desc and the table");
static_assert(sizeof(rt_object_motion) == 96 && sizeof(rttp::Motion) == 96 && offsetof(rt_object_motion, nt) == offsetof(rttp::Motion, nt) &&
              offsetof(rt_object_motion, moved) == offsetof(rttp::Motion, moved), "rttp::Motion is rt_object_motion");
rt_temporal_desc temporal_head(const rt_temporal_motion_desc* d);
// temporal_check on the head, then the table's own rules (on device memory the table is 16-byte aligned).
int temporal_motion_check(const rt_temporal_motion_desc* d, bool device, bool host_memory, std::string& err);
int temporal_motion_host(const rt_temporal_motion_desc* d, std::string& err);

// The _deforming forms.  rt_temporal_deform_desc is rt_temporal_motion_desc with the triangle side behind it: its head, as
// an rt_temporal_motion_desc of its own (struct_bytes set), is what temporal_motion_check is given.
static_assert(offsetof(rt_temporal_deform_desc, primitive) == sizeof(rt_temporal_motion_desc) &&
                  sizeof(rt_temporal_deform_desc) == sizeof(rt_temporal_motion_desc) + 40,
              "rt_temporal_deform_desc is rt_temporal_motion_desc and the triangle side");
static_assert(sizeof(rt_packed_triangle) == 96 && sizeof(rttp::Tri) == 96 && offsetof(rt_packed_triangle, v2) == offsetof(rttp::Tri, v2) &&
                  offsetof(rt_packed_triangle, n1) == offsetof(rttp::Tri, n1) && offsetof(rt_packed_triangle, n3) == offsetof(rttp::Tri, n3),
              "rttp::Tri is rt_packed_triangle");
static_assert(rttp::HIT_BACKFACE == RT_HIT_BACKFACE, "the flags plane's backface bit");
rt_temporal_motion_desc temporal_motion_head(const rt_temporal_deform_desc* d);
// temporal_motion_check on the head, then the triangle side's own rules (on device memory: primitive and bary 4-byte
// aligned, prev_triangles 16).
int temporal_deform_check(const rt_temporal_deform_desc* d, bool device, bool host_memory, std::string& err);
int temporal_deform_host(const rt_temporal_deform_desc* d, std::string& err);
}  // namespace rt2

namespace rtd {
struct TemporalArgs {
    rttp::Call call;
    const float* color;          // [h][w][4]
    const float* point;          // [h][w][3]
    const float* normal;         // [h][w][3]
    const uint32_t* object;      // [h][w] or null
    const float* prev_color;     // [h][w][4]
    const float* prev_history;   // [h][w]
    const float* prev_point;     // [h][w][3]
    const float* prev_normal;    // [h][w][3]
    const uint32_t* prev_object; // [h][w] or null
    float* out;                  // [h][w][4]; may be `color`
    float* out_history;          // [h][w]
    float* motion;               // [h][w][2] or null
};
// rt_temporal_accumulate_moving: the same planes (object is there) and the table, 16-byte aligned
struct TemporalMotionArgs {
    TemporalArgs t;
    const rttp::Motion* motions;   // [n_objects]
    uint32_t n_objects;
};
// rt_temporal_accumulate_deforming: those, the current G-buffer's triangle planes and the previous triangles [tri_first,
// tri_first + n_prev_triangles) of the uploaded array, 16-byte aligned
struct TemporalDeformArgs {
    TemporalMotionArgs m;
    const uint32_t* primitive;         // [h][w]
    const float* bary;                 // [h][w][2]
    const uint8_t* flags;              // [h][w]
    const rttp::Tri* prev_triangles;   // [n_prev_triangles]
    uint32_t tri_first, n_prev_triangles;
};
}  // namespace rtd

#endif
