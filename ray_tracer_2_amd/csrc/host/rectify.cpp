// host/rectify.cpp -- history rectification's definition in executable form (include/rt_abi.h: rt_temporal_rectify_host;
// DESIGN.md section 2.20), the argument rules and the once-per-call numbers it shares with the device entry point.  Plain
// C++ over host pointers; the per-texel arithmetic is csrc/rt_rectify.h, which the device kernel evaluates too.  Compiled
// with -ffp-contract=off.
#if defined(__HIPCC__)
// (the build compiles this C++ unit with hipcc as well: rt_rectify.h then marks its functions __host__ __device__
// __forceinline__, which the runtime's headers define for plain C++)
#include <hip/hip_runtime_api.h>
#endif
#include <cstring>

#include "../rt_rectify_api.h"
#include "plane_check.h"

namespace rt2 {

bool rectify_overlap(const float* a, const float* b, size_t texels) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b, bytes = (uintptr_t)texels * 16u;
    return pa < pb ? pb - pa < bytes : pa - pb < bytes;
}

int rectify_check(const rt_rectify_desc* d, bool device, bool host_memory, std::string& err) {
    auto bad = [&](int code, const char* msg) {
        err = msg;
        return code;
    };
    if (!d) return bad(RT_ERR_INVALID_ARGUMENT, "null rt_rectify_desc");
    if (d->struct_bytes != sizeof(rt_rectify_desc)) return bad(RT_ERR_INVALID_ARGUMENT, "rt_rectify_desc.struct_bytes is not sizeof(rt_rectify_desc)");
    if (d->_p0 != 0u || d->_p1 != 0u) return bad(RT_ERR_INVALID_ARGUMENT, "rt_rectify_desc._p0 and _p1 must be 0");
    if (d->width == 0u || d->height == 0u) return bad(RT_ERR_INVALID_ARGUMENT, "zero width or height");
    if (d->radius < 1u || d->radius > (uint32_t)rtrc::MAX_RADIUS) return bad(RT_ERR_INVALID_ARGUMENT, "radius is not 1, 2 or 3");
    if (!(d->clip_sigma >= 0.0f)) return bad(RT_ERR_INVALID_ARGUMENT, "clip_sigma is NaN or negative");
    if (!(d->clip_history >= 1.0f)) return bad(RT_ERR_INVALID_ARGUMENT, "clip_history is NaN or below 1");
    if (!d->history || !d->history_length || !d->out || !d->out_history)
        return bad(RT_ERR_INVALID_ARGUMENT, "null history, history_length, out or out_history plane");
    if (!d->color && (!device || host_memory))
        return bad(RT_ERR_INVALID_ARGUMENT, "null color plane (only device planes may name the handle's image that way)");
    if ((d->moments == nullptr) != (d->history_moments == nullptr) || (d->moments == nullptr) != (d->out_moments == nullptr))
        return bad(RT_ERR_INVALID_ARGUMENT, "moments, history_moments and out_moments come together or not at all");
    if ((uint64_t)d->width * d->height > 0x7fffffffull) return bad(RT_ERR_CAPACITY, "more than 2^31 - 1 texels");
    if (d->color && rectify_overlap(d->out, d->color, (size_t)d->width * d->height))
        return bad(RT_ERR_INVALID_ARGUMENT, "out overlaps color, which the neighbouring texels read");
    if (device && !host_memory) {
        const PlaneAlign planes[10] = {
            {d->color, 15u, "color"}, {d->history, 15u, "history"}, {d->history_length, 3u, "history_length"}, {d->object, 3u, "object"},
            {d->moments, 15u, "moments"}, {d->history_moments, 15u, "history_moments"}, {d->out, 15u, "out"},
            {d->out_history, 3u, "out_history"}, {d->out_moments, 15u, "out_moments"}, {d->out_clipped, 0u, "out_clipped"}};
        return misaligned(planes, 10, err);
    }
    return RT_OK;
}

rtrc::Call rectify_call(const rt_rectify_desc& d) {
    rtrc::Call c{};
    c.width = d.width;
    c.height = d.height;
    c.radius = (int32_t)d.radius;
    c.clip_sigma = d.clip_sigma;
    c.clip_history = d.clip_history;
    return c;
}

int rectify_host(const rt_rectify_desc* d, std::string& err) {
    if (const int rc = rectify_check(d, false, false, err); rc != RT_OK) return rc;
    const rtrc::Call c = rectify_call(*d);
    const int64_t W = d->width, H = d->height, R = c.radius;
    const bool have_moments = d->moments != nullptr;
    for (int64_t y = 0; y < H; ++y)
        for (int64_t x = 0; x < W; ++x) {
            const size_t p = (size_t)(y * W + x);
            // (the texel's own reads come before its writes: out may be history, out_history history_length, out_moments
            // history_moments)
            float color[4], h[4], m[4] = {0.0f, 0.0f, 0.0f, 0.0f}, hm[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            std::memcpy(color, d->color + 4 * p, sizeof(color));
            std::memcpy(h, d->history + 4 * p, sizeof(h));
            const float n = d->history_length[p];
            if (have_moments) {
                std::memcpy(m, d->moments + 4 * p, sizeof(m));
                std::memcpy(hm, d->history_moments + 4 * p, sizeof(hm));
            }
            rtrc::Sums s;
            for (int64_t dy = -R; dy <= R; ++dy)
                for (int64_t dx = -R; dx <= R; ++dx) {
                    const int64_t qx = x + dx, qy = y + dy;
                    if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                    const size_t q = (size_t)(qy * W + qx);
                    const float* cq = d->color + 4 * q;
                    s.add(rttp::finite3(cq) && (!d->object || d->object[q] == d->object[p]), cq[0], cq[1], cq[2]);
                }
            const rtrc::Result r = rtrc::resolve(c, s, color, h, n, have_moments, m, hm);
            std::memcpy(d->out + 4 * p, r.out, sizeof(r.out));
            d->out_history[p] = r.history;
            if (have_moments) std::memcpy(d->out_moments + 4 * p, r.moments, sizeof(r.moments));
            if (d->out_clipped) d->out_clipped[p] = r.clipped;
        }
    return RT_OK;
}

}  // namespace rt2
