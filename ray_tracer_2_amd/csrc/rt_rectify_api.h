// rt_rectify_api.h -- what the units of history rectification declare to each other (include/rt_abi.h: rt_temporal_rectify,
// rt_temporal_rectify_host): the argument rules, the once-per-call numbers and the host restatement (host/rectify.cpp), and
// the argument struct of the device launch (rt_rectify.hip), all called by the entry points in rt_api_frames.hip.  The
// arithmetic they share is csrc/rt_rectify.h.
#ifndef RT_RECTIFY_API_H
#define RT_RECTIFY_API_H

#include <stdint.h>

#include <string>

#include "rt_abi.h"
#include "rt_rectify.h"

namespace rt2 {
// RT_OK, or the error of a desc that rt_temporal_rectify (device == true: host_memory says which path, color may be NULL
// without it) or rt_temporal_rectify_host (device == false) refuses, with its reason in `err`.  Nothing is dereferenced but
// the desc.
int rectify_check(const rt_rectify_desc* d, bool device, bool host_memory, std::string& err);
// Do the `texels` texels of the [4] planes at a and b share a byte?  (What the check refuses between out and color; the
// entry point asks it again for the handle's image.)
bool rectify_overlap(const float* a, const float* b, size_t texels);
// The once-per-call numbers of a checked desc.
rtrc::Call rectify_call(const rt_rectify_desc& d);
int rectify_host(const rt_rectify_desc* d, std::string& err);
}  // namespace rt2

namespace rtd {
struct RectifyArgs {
    rtrc::Call call;
    const float* color;             // [h][w][4]
    const float* history;           // [h][w][4]
    const float* history_length;    // [h][w]
    const uint32_t* object;         // [h][w] or null
    const float* moments;           // [h][w][4] or null (with history_moments and out_moments, or not at all)
    const float* history_moments;   // [h][w][4] or null
    float* out;                     // [h][w][4]
    float* out_history;             // [h][w]
    float* out_moments;             // [h][w][4] or null
    uint8_t* out_clipped;           // [h][w] or null
};
}  // namespace rtd

#endif
