// rt_vdenoise_api.h -- what the variance-guided denoiser's units declare to each other (include/rt_abi.h:
// rt_denoise_variance, rt_luminance_moments and their _host forms): the argument rules and the host restatement
// (host/vdenoise.cpp), and the arguments of the device launches (rt_vdenoise.hip), both called by the entry points in
// rt_api_frames.hip.  The arithmetic they share is csrc/rt_vdenoise.h.
#ifndef RT_VDENOISE_API_H
#define RT_VDENOISE_API_H

#include <stdint.h>

#include <string>

#include "rt_abi.h"

namespace rt2 {
// RT_OK, or the error of a desc that the device entry points (device == true: host_memory says which path, color may be
// NULL without it) or the host ones (device == false) refuse, with its reason in `err`.  moments_only: the rules of
// rt_luminance_moments, which examines neither the filter's parameters nor the moments planes.  Nothing is dereferenced
// but the desc.
int vdenoise_check(const rt_vdenoise_desc* d, bool moments_only, bool device, bool host_memory, std::string& err);
int vdenoise_host(const rt_vdenoise_desc* d, std::string& err);
int luminance_moments_host(const rt_vdenoise_desc* d, std::string& err);
}  // namespace rt2

namespace rtd {
struct VDenoiseArgs {
    uint32_t width, height;
    const float* color;        // [h][w][4]
    const float* normal;       // [h][w][3]
    const float* point;        // [h][w][3]
    const float* albedo;       // [h][w][4] or null
    const float* emission;     // [h][w][4] or null
    const float* moments;      // [h][w][4] or null
    const float* history;      // [h][w]; non-null exactly when moments is
    float* out;                // [h][w][4]; may be `color`
    float* out_variance;       // [h][w] or null
    void* guide;               // scratch: two float4 per texel -- (normal.xyz, filterable ? 1 : 0), (point.xyz, 0)
    void* ping[2];             // scratch: (c_i.rgb, var_i), one float4 per texel each
    int iterations;            // 1 .. 8
    float sigma_luminance, sigma_normal, sigma_point, min_history;
};
// (the scratch members are unused by launch_luminance_moments)
}  // namespace rtd

#endif
