// rt_denoise_api.h -- what the denoiser's units declare to each other (include/rt_abi.h: rt_denoise, rt_denoise_host): the
// argument rules and the host restatement (host/denoise.cpp), and the arguments of the device launch (rt_denoise.hip), both
// called by the entry points in rt_api_frames.hip.  The arithmetic they share is csrc/rt_denoise.h.
#ifndef RT_DENOISE_API_H
#define RT_DENOISE_API_H

#include <stdint.h>

#include <string>

#include "rt_abi.h"

namespace rt2 {
// RT_OK, or the error of a desc that rt_denoise (device == true: host_memory says which path, color may be NULL without
// it) or rt_denoise_host (device == false) refuses, with its reason in `err`.  Nothing is dereferenced but the desc.
int denoise_check(const rt_denoise_desc* d, bool device, bool host_memory, std::string& err);
int denoise_host(const rt_denoise_desc* d, std::string& err);
}  // namespace rt2

namespace rtd {
struct DenoiseArgs {
    uint32_t width, height;
    const float* color;        // [h][w][4]
    const float* normal;       // [h][w][3]
    const float* point;        // [h][w][3]
    const float* albedo;       // [h][w][4] or null
    const float* emission;     // [h][w][4] or null
    float* out;                // [h][w][4]; may be `color`
    void* guide;               // scratch: two float4 per texel -- (normal.xyz, filterable ? 1 : 0), (point.xyz, 0)
    void* ping[2];             // scratch: the demodulated colour c_i, one float4 per texel each
    int iterations;            // 1 .. 8
    float sigma_color, sigma_normal, sigma_point;
};
}  // namespace rtd

#endif
