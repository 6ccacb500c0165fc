// rt_upsample_api.h -- what the units of guided upsampling declare to each other (include/rt_abi.h: rt_upsample,
// rt_upsample_host): the argument rules, the once-per-call numbers and the host restatement (host/upsample.cpp), and the
// argument struct of the device launch (rt_upsample.hip), all called by the entry points in rt_api_frames.hip.  The arithmetic
// they share is csrc/rt_upsample.h.
#ifndef RT_UPSAMPLE_API_H
#define RT_UPSAMPLE_API_H

#include <stdint.h>

#include <string>

#include "rt_abi.h"
#include "rt_upsample.h"

namespace rt2 {
// RT_OK, or the error of a desc that rt_upsample (device == true: host_memory says which path, lo_color may be NULL
// without it) or rt_upsample_host (device == false) refuses, with its reason in `err`.  Nothing is dereferenced but the desc.
int upsample_check(const rt_upsample_desc* d, bool device, bool host_memory, std::string& err);
// The once-per-call numbers of a checked desc.
rtup::Call upsample_call(const rt_upsample_desc& d);
int upsample_host(const rt_upsample_desc* d, std::string& err);
}  // namespace rt2

namespace rtd {
struct UpsampleArgs {
    rtup::Call call;
    const float* lo_color;       // [h][w][4]
    const float* lo_point;       // [h][w][3]
    const float* lo_normal;      // [h][w][3]
    const uint32_t* lo_object;   // [h][w]
    const float* lo_albedo;      // [h][w][4] or null (with albedo, or not at all)
    const float* depth;          // [H][W]
    const float* point;          // [H][W][3]
    const float* normal;         // [H][W][3]
    const uint32_t* object;      // [H][W]
    const float* albedo;         // [H][W][4] or null
    const float* emission;       // [H][W][4] or null
    float* out;                  // [H][W][4]
    uint8_t* coverage;           // [H][W] or null
};
}  // namespace rtd

#endif
