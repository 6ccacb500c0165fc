// host/upsample.cpp -- guided upsampling's definition in executable form (include/rt_abi.h: rt_upsample_host; DESIGN.md
// section 2.18), the argument rules and the once-per-call numbers it shares with the device entry point.  Plain C++ over
// host pointers; the per-texel arithmetic is csrc/rt_upsample.h, which the device kernel evaluates too.  Compiled with
// -ffp-contract=off.
#if defined(__HIPCC__)
// (the build compiles this C++ unit with hipcc as well: rt_upsample.h then marks its functions __host__ __device__
// __forceinline__, which the runtime's headers define for plain C++)
#include <hip/hip_runtime_api.h>
#endif
#include <cstring>

#include "../rt_upsample_api.h"
#include "plane_check.h"

namespace rt2 {

int upsample_check(const rt_upsample_desc* d, bool device, bool host_memory, std::string& err) {
    auto bad = [&](int code, const char* msg) {
        err = msg;
        return code;
    };
    if (!d) return bad(RT_ERR_INVALID_ARGUMENT, "null rt_upsample_desc");
    if (d->struct_bytes != sizeof(rt_upsample_desc)) return bad(RT_ERR_INVALID_ARGUMENT, "rt_upsample_desc.struct_bytes is not sizeof(rt_upsample_desc)");
    if (d->_p0 != 0u) return bad(RT_ERR_INVALID_ARGUMENT, "rt_upsample_desc._p0 must be 0");
    if (d->lo_width == 0u || d->lo_height == 0u || d->width == 0u || d->height == 0u) return bad(RT_ERR_INVALID_ARGUMENT, "zero width or height");
    if (!(d->point_tolerance > 0.0f) || !rttp::is_finite(d->point_tolerance))
        return bad(RT_ERR_INVALID_ARGUMENT, "point_tolerance is NaN, <= 0 or infinite");
    if (!(d->normal_cos >= -1.0f && d->normal_cos <= 1.0f)) return bad(RT_ERR_INVALID_ARGUMENT, "normal_cos is NaN or outside [-1, 1]");
    if (!d->lo_point || !d->lo_normal || !d->lo_object || !d->depth || !d->point || !d->normal || !d->object || !d->out)
        return bad(RT_ERR_INVALID_ARGUMENT, "null lo_point, lo_normal, lo_object, depth, point, normal, object or out plane");
    if (!d->lo_color && (!device || host_memory))
        return bad(RT_ERR_INVALID_ARGUMENT, "null lo_color plane (only device planes may name the handle's image that way)");
    if ((d->lo_albedo == nullptr) != (d->albedo == nullptr)) return bad(RT_ERR_INVALID_ARGUMENT, "lo_albedo and albedo come together or not at all");
    if ((uint64_t)d->lo_width * d->lo_height > 0x7fffffffull) return bad(RT_ERR_CAPACITY, "more than 2^31 - 1 texels in the low frame");
    if ((uint64_t)d->width * d->height > 0x7fffffffull) return bad(RT_ERR_CAPACITY, "more than 2^31 - 1 texels in the high frame");
    if (device && !host_memory) {
        const PlaneAlign planes[13] = {
            {d->lo_color, 15u, "lo_color"}, {d->lo_point, 3u, "lo_point"}, {d->lo_normal, 3u, "lo_normal"}, {d->lo_object, 3u, "lo_object"},
            {d->lo_albedo, 15u, "lo_albedo"}, {d->depth, 3u, "depth"}, {d->point, 3u, "point"}, {d->normal, 3u, "normal"},
            {d->object, 3u, "object"}, {d->albedo, 15u, "albedo"}, {d->emission, 15u, "emission"}, {d->out, 15u, "out"},
            {d->coverage, 0u, "coverage"}};
        return misaligned(planes, 13, err);
    }
    return RT_OK;
}

rtup::Call upsample_call(const rt_upsample_desc& d) {
    rtup::Call c{};
    c.lo_width = d.lo_width;
    c.lo_height = d.lo_height;
    c.width = d.width;
    c.height = d.height;
    c.rx = rtup::ratio(d.lo_width, d.width);
    c.ry = rtup::ratio(d.lo_height, d.height);
    c.point_tolerance = d.point_tolerance;
    c.normal_cos = d.normal_cos;
    return c;
}

namespace {
// The low texel (qx, qy), or the nearest one inside the frame when it is outside (and then refused).
rtup::Tap load_tap(const rt_upsample_desc* d, int64_t qx, int64_t qy) {
    const int64_t w = d->lo_width, h = d->lo_height;
    const bool inside = qx >= 0 && qx < w && qy >= 0 && qy < h;
    const int64_t cx = qx < 0 ? 0 : qx >= w ? w - 1 : qx, cy = qy < 0 ? 0 : qy >= h ? h - 1 : qy;
    const size_t q = (size_t)(cy * w + cx);
    float c[4], al[3] = {1.0f, 1.0f, 1.0f};
    std::memcpy(c, d->lo_color + 4 * q, sizeof(c));
    if (d->lo_albedo) std::memcpy(al, d->lo_albedo + 4 * q, sizeof(al));
    return rtup::make_tap(inside, c, d->lo_point + 3 * q, d->lo_normal + 3 * q, d->lo_object[q], d->lo_albedo != nullptr, al);
}
}  // namespace

int upsample_host(const rt_upsample_desc* d, std::string& err) {
    if (const int rc = upsample_check(d, false, false, err); rc != RT_OK) return rc;
    const rtup::Call c = upsample_call(*d);
    const int64_t W = d->width, H = d->height;
    for (int64_t Y = 0; Y < H; ++Y)
        for (int64_t X = 0; X < W; ++X) {
            const size_t p = (size_t)(Y * W + X);
            rtup::Texel P;
            for (int k = 0; k < 3; ++k) {
                P.n[k] = d->normal[3 * p + k];
                P.x[k] = d->point[3 * p + k];
            }
            P.depth = d->depth[p];
            P.obj = d->object[p];
            float em[3] = {0.0f, 0.0f, 0.0f};
            if (d->emission) std::memcpy(em, d->emission + 4 * p, sizeof(em));
            const bool is_guided = rtup::guided(P, em);
            const bool demod = is_guided && d->albedo != nullptr;
            const float reach = c.point_tolerance * P.depth;
            const rtup::Where w = rtup::locate(c, (uint32_t)X, (uint32_t)Y);
            float v[4];
            uint8_t cover = rtup::COVER_RING1;
            rtup::Sums s;
            for (int i = 0; i < 4; ++i)
                s.add(rttp::tap_weight(i, w.ax.t, w.ay.t), load_tap(d, (int64_t)w.ax.i0 + rttp::tap_dx(i), (int64_t)w.ay.i0 + rttp::tap_dy(i)),
                      P, is_guided, demod, reach, c.normal_cos);
            if (!s.have()) {
                cover = rtup::COVER_RING2;
                s = rtup::Sums{};
                for (int j = -1; j <= 2; ++j)
                    for (int i = -1; i <= 2; ++i)
                        s.add(rtup::ring2_weight(i, j, w.ax.t, w.ay.t), load_tap(d, (int64_t)w.ax.i0 + i, (int64_t)w.ay.i0 + j), P,
                              is_guided, demod, reach, c.normal_cos);
            }
            if (s.have()) {
                s.mean(v);
            } else {
                cover = rtup::COVER_HOLE;
                rtup::tap_color(load_tap(d, rtup::nearest(w.ax, c.lo_width), rtup::nearest(w.ay, c.lo_height)), demod, v);
            }
            float al[3] = {1.0f, 1.0f, 1.0f}, out[4];
            if (demod) std::memcpy(al, d->albedo + 4 * p, sizeof(al));
            rtup::finish(v, demod, al, out);
            std::memcpy(d->out + 4 * p, out, sizeof(out));
            if (d->coverage) d->coverage[p] = cover;
        }
    return RT_OK;
}

}  // namespace rt2
