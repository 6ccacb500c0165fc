// rt_temporal_api.h -- what the units of temporal accumulation declare to each other (include/rt_abi.h:
// rt_temporal_accumulate, rt_temporal_accumulate_host): the argument rules, the once-per-call numbers and the host
// restatement (host/temporal.cpp), and the arguments of the device launch (rt_temporal.hip), all called by the entry points
// in rt_api.hip.  The arithmetic they share is csrc/rt_temporal.h.
#ifndef RT_TEMPORAL_API_H
#define RT_TEMPORAL_API_H

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
}  // namespace rtd

#endif
