// host/plane_check.h -- the alignment rule of a frame pass's device planes (host/denoise.cpp, vdenoise.cpp, temporal.cpp,
// adaptive.cpp): each call lists its planes once, with the least alignment its kernels read or write them at.
#ifndef RT_HOST_PLANE_CHECK_H
#define RT_HOST_PLANE_CHECK_H

#include <stdint.h>

#include <string>

#include "rt_abi.h"

namespace rt2 {

struct PlaneAlign {
    const void* p;     // (null: the plane is absent, and aligned)
    uintptr_t mask;    // alignment - 1
    const char* name;
};

// RT_OK, or RT_ERR_INVALID_ARGUMENT with the first misaligned plane of planes[0, n) named in `err`.
inline int misaligned(const PlaneAlign* planes, int n, std::string& err) {
    for (int i = 0; i < n; ++i)
        if (((uintptr_t)planes[i].p & planes[i].mask) != 0u) {
            err = std::string("device plane ") + planes[i].name + " is not aligned to " + std::to_string(planes[i].mask + 1u) + " bytes";
            return RT_ERR_INVALID_ARGUMENT;
        }
    return RT_OK;
}

}  // namespace rt2

#endif
