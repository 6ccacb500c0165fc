// rt_display_api.h -- what the units of the display pass and the exposure meter declare to each other (include/rt_abi.h:
// rt_display, rt_auto_exposure, rt_snapshot_display and the _host forms): the argument rules, the once-per-call numbers and
// the host restatements (host/display.cpp), and the argument structs of the device launches (rt_display.hip), all called by
// the entry points in rt_api_frames.hip (rt_snapshot_display: rt_api.hip).  The arithmetic they share is csrc/rt_display.h.
#ifndef RT_DISPLAY_API_H
#define RT_DISPLAY_API_H

#include <stdint.h>

#include <string>

#include "rt_abi.h"
#include "rt_display.h"

namespace rt2 {
// Which entry point checks a rt_display_desc: rt_display_host; rt_display on host memory; rt_display on device memory
// (color may be NULL: the image; the planes' alignment); rt_snapshot_display (color and out must be NULL).
enum class DisplayPath { HOST, STAGED, DEVICE, SNAPSHOT };
// RT_OK, or the error of a desc that the entry point refuses, with its reason in `err`.  Nothing is dereferenced but the desc.
int display_check(const rt_display_desc* d, DisplayPath path, std::string& err);
int auto_exposure_check(const rt_auto_exposure_desc* d, bool device, bool host_memory, std::string& err);
// The once-per-call numbers of a checked desc.
rtdp::Call display_call(const rt_display_desc& d);
rtdp::MeterCall auto_exposure_call(const rt_auto_exposure_desc& d);
int display_host(const rt_display_desc* d, std::string& err);
int auto_exposure_host(const rt_auto_exposure_desc* d, std::string& err);
}  // namespace rt2

namespace rtd {
struct DisplayArgs {
    rtdp::Call call;
    const float* color;            // [h][w][4]
    const float* exposure_scale;   // one float or null
    uint32_t* out;                 // [h][w]: four bytes per texel
};
struct AutoExposureArgs {
    rtdp::MeterCall call;
    const float* color;        // [h][w][4]
    const float* prev_scale;   // one float or null
    uint32_t* bins;            // [256]: the handle's scratch, zeroed by the launch
    uint32_t* histogram;       // [256] or null
    float* scale;              // one float
};
}  // namespace rtd

#endif
