// rt_adaptive_api.h -- what adaptive sampling's units declare to each other (include/rt_abi.h: rt_adaptive_plan,
// rt_adaptive_merge and their _host forms): the argument rules and the host restatement (host/adaptive.cpp), and the
// arguments of the device launches (rt_adaptive.hip), both called by the entry points in rt_api_frames.hip.  The rules they share
// are csrc/rt_adaptive.h.
#ifndef RT_ADAPTIVE_API_H
#define RT_ADAPTIVE_API_H

#include <stddef.h>
#include <stdint.h>

#include <string>

#include "rt_abi.h"

namespace rt2 {
// RT_OK, or the error of a desc that the device entry points (device == true: host_memory says which path; merge's color
// may be NULL without it) or the host ones (device == false) refuse, with its reason in `err`.  Nothing is dereferenced
// but the desc.
int adaptive_plan_check(const rt_adaptive_plan_desc* d, bool device, bool host_memory, std::string& err);
int adaptive_merge_check(const rt_adaptive_merge_desc* d, bool device, bool host_memory, std::string& err);
int adaptive_plan_host(const rt_adaptive_plan_desc* d, std::string& err);
int adaptive_merge_host(const rt_adaptive_merge_desc* d, std::string& err);
}  // namespace rt2

namespace rtd {
// The plan's scans work on blocks of ADAPTIVE_BLOCK texels; the handle's scratch holds, per block, the sum of q (u64), its
// exclusive scan (u64), the sum of n, its exclusive scan, and the block's counts of texels above min_samples and of clamped
// ones (u32 each: 32 bytes), behind a header of ADAPTIVE_HEADER_BYTES (word 0: the maximum's bits; words 2 .. 3: S).
constexpr uint32_t ADAPTIVE_BLOCK = 1024u;
constexpr size_t ADAPTIVE_HEADER_BYTES = 256u, ADAPTIVE_BYTES_PER_BLOCK = 32u;
inline size_t adaptive_blocks(size_t texels) { return (texels + ADAPTIVE_BLOCK - 1) / ADAPTIVE_BLOCK; }
inline size_t adaptive_scratch_bytes(size_t texels) { return ADAPTIVE_HEADER_BYTES + adaptive_blocks(texels) * ADAPTIVE_BYTES_PER_BLOCK; }

struct AdaptivePlanArgs {
    uint32_t width, height, budget, min_samples, max_samples, first_frame;
    float origin[3];
    const float* variance;   // [h][w]
    const float* dir;        // [h][w][3]
    uint32_t* counts;        // [h][w]
    uint32_t* offsets;       // [h][w]
    void* rays;              // [budget] rt_path_ray
    uint32_t* totals;        // [4]
    void* scratch;           // adaptive_scratch_bytes(width * height)
};
struct AdaptiveMergeArgs {
    uint32_t width, height, budget;
    float max_history;
    const float* radiance;   // [budget][4]
    const uint32_t* counts;
    const uint32_t* offsets;
    const float* color;
    const float* history;
    const float* albedo;     // or null
    const float* moments;    // or null
    float* out;
    float* out_history;
    float* out_moments;      // non-null exactly when moments is
};
}  // namespace rtd

#endif
