// host/temporal.cpp -- temporal accumulation's definition in executable form (include/rt_abi.h:
// rt_temporal_accumulate_host and, with a motion table, rt_temporal_accumulate_moving_host and
// rt_temporal_accumulate_deforming_host -- one loop for the three), the argument rules and the once-per-call numbers it shares with
// the device entry point.  Plain C++ over host pointers; the per-texel arithmetic is csrc/rt_temporal.h, which the device
// kernel evaluates too.  Compiled with -ffp-contract=off.
#if defined(__HIPCC__)
// (the build compiles this C++ unit with hipcc as well: rt_temporal.h then marks its functions __host__ __device__
// __forceinline__, which the runtime's headers define for plain C++)
#include <hip/hip_runtime_api.h>
#endif
#include <cstring>

#include "../rt_temporal_api.h"
#include "glam_math.h"
#include "plane_check.h"

namespace rt2 {

int temporal_check(const void* desc, TemporalKind kind, bool device, bool host_memory, rt_temporal_deform_desc& wide, std::string& err) {
    auto bad = [&](int code, const char* msg) {
        err = msg;
        return code;
    };
    static const struct {
        uint32_t bytes;
        const char *null_desc, *bad_bytes;
    } KINDS[3] = {
        {sizeof(rt_temporal_desc), "null rt_temporal_desc", "rt_temporal_desc.struct_bytes is not sizeof(rt_temporal_desc)"},
        {sizeof(rt_temporal_motion_desc), "null rt_temporal_motion_desc", "rt_temporal_motion_desc.struct_bytes is not sizeof(rt_temporal_motion_desc)"},
        {sizeof(rt_temporal_deform_desc), "null rt_temporal_deform_desc", "rt_temporal_deform_desc.struct_bytes is not sizeof(rt_temporal_deform_desc)"}};
    const auto& k = KINDS[(int)kind];
    if (!desc) return bad(RT_ERR_INVALID_ARGUMENT, k.null_desc);
    uint32_t struct_bytes;   // (the first word of all three)
    std::memcpy(&struct_bytes, desc, sizeof(struct_bytes));
    if (struct_bytes != k.bytes) return bad(RT_ERR_INVALID_ARGUMENT, k.bad_bytes);
    // the kind's desc is a prefix of the widest (rt_temporal_api.h: the static_asserts); what lies behind it stays null or zero
    wide = rt_temporal_deform_desc{};
    std::memcpy(&wide, desc, struct_bytes);
    const rt_temporal_deform_desc* d = &wide;
    const bool device_planes = device && !host_memory;

    if (d->_p0 != 0u) return bad(RT_ERR_INVALID_ARGUMENT, "rt_temporal_desc._p0 must be 0");
    if (d->width == 0u || d->height == 0u) return bad(RT_ERR_INVALID_ARGUMENT, "zero width or height");
    if (!(d->max_history >= 1.0f)) return bad(RT_ERR_INVALID_ARGUMENT, "max_history is NaN or below 1");
    if (!(d->point_tolerance > 0.0f) || !rttp::is_finite(d->point_tolerance))
        return bad(RT_ERR_INVALID_ARGUMENT, "point_tolerance is NaN, <= 0 or infinite");
    if (!(d->normal_cos >= -1.0f && d->normal_cos <= 1.0f)) return bad(RT_ERR_INVALID_ARGUMENT, "normal_cos is NaN or outside [-1, 1]");
    if (!d->point || !d->normal || !d->prev_color || !d->prev_history || !d->prev_point || !d->prev_normal || !d->out || !d->out_history)
        return bad(RT_ERR_INVALID_ARGUMENT, "null point, normal, prev_color, prev_history, prev_point, prev_normal, out or out_history plane");
    if (!d->color && (!device || host_memory)) return bad(RT_ERR_INVALID_ARGUMENT, "null color plane (only device planes may name the handle's image that way)");
    if ((uint64_t)d->width * d->height > 0x7fffffffull) return bad(RT_ERR_CAPACITY, "more than 2^31 - 1 texels");
    if (device_planes) {
        const PlaneAlign planes[12] = {
            {d->color, 15u, "color"}, {d->point, 3u, "point"}, {d->normal, 3u, "normal"}, {d->object, 3u, "object"},
            {d->prev_color, 15u, "prev_color"}, {d->prev_history, 3u, "prev_history"}, {d->prev_point, 3u, "prev_point"},
            {d->prev_normal, 3u, "prev_normal"}, {d->prev_object, 3u, "prev_object"}, {d->out, 15u, "out"},
            {d->out_history, 3u, "out_history"}, {d->motion, 7u, "motion"}};
        if (const int rc = misaligned(planes, 12, err); rc != RT_OK) return rc;
    }
    if (kind == TemporalKind::PLAIN) return RT_OK;

    if (d->_p1 != 0u) return bad(RT_ERR_INVALID_ARGUMENT, "rt_temporal_motion_desc._p1 must be 0");
    if (!d->motions) return bad(RT_ERR_INVALID_ARGUMENT, "null motions table");
    if (d->n_objects == 0u) return bad(RT_ERR_INVALID_ARGUMENT, "n_objects is zero");
    if (!d->object) return bad(RT_ERR_INVALID_ARGUMENT, "null object plane (a motion table is indexed by it)");
    if (device_planes) {
        const PlaneAlign table[1] = {{d->motions, 15u, "motions"}};
        if (const int rc = misaligned(table, 1, err); rc != RT_OK) return rc;
    }
    if (kind == TemporalKind::MOVING) return RT_OK;

    if (!d->primitive || !d->bary || !d->flags) return bad(RT_ERR_INVALID_ARGUMENT, "null primitive, bary or flags plane (a deformed texel's triangle is named by them)");
    if (!d->prev_triangles) return bad(RT_ERR_INVALID_ARGUMENT, "null prev_triangles");
    if (d->n_prev_triangles == 0u) return bad(RT_ERR_INVALID_ARGUMENT, "n_prev_triangles is zero");
    if ((uint64_t)d->tri_first + d->n_prev_triangles > 0x100000000ull) return bad(RT_ERR_INVALID_ARGUMENT, "tri_first + n_prev_triangles is past 2^32");
    if (device_planes) {
        const PlaneAlign side[4] = {{d->primitive, 3u, "primitive"}, {d->bary, 3u, "bary"}, {d->flags, 0u, "flags"}, {d->prev_triangles, 15u, "prev_triangles"}};
        return misaligned(side, 4, err);
    }
    return RT_OK;
}

rttp::Call temporal_call(const rt_temporal_deform_desc& d) {
    Mat4 m;
    std::memcpy(&m, d.prev_camera.cam_to_world, sizeof(m));
    const Mat4 v = mat4_inverse(m);
    rttp::Call c{};
    for (int col = 0; col < 4; ++col)
        for (int k = 0; k < 3; ++k) c.v[col][k] = v.c[col][k];
    c.pw = d.prev_camera.view_params[0];
    c.ph = d.prev_camera.view_params[1];
    c.fd = d.prev_camera.view_params[2];
    c.max_history = d.max_history;
    c.point_tolerance = d.point_tolerance;
    c.normal_cos = d.normal_cos;
    c.width = d.width;
    c.height = d.height;
    return c;
}

// The three host entry points: the check, then their one loop.  Without a table (PLAIN) no texel is carried; with one and
// no triangle side (MOVING) every non-zero `moved` is carried rigidly.
static int accumulate(const void* desc, TemporalKind kind, std::string& err) {
    rt_temporal_deform_desc wide;
    if (const int rc = temporal_check(desc, kind, false, false, wide, err); rc != RT_OK) return rc;
    const rt_temporal_deform_desc* d = &wide;
    const rttp::Call c = temporal_call(wide);
    const int64_t W = d->width, H = d->height;
    const bool match_object = d->object && d->prev_object;
    const float nan = rttp::u2f(rttp::QUIET_NAN);
    for (int64_t y = 0; y < H; ++y)
        for (int64_t x = 0; x < W; ++x) {
            const size_t p = (size_t)(y * W + x);
            float color[4];   // (out may be color: the texel is read before it is written)
            std::memcpy(color, d->color + 4 * p, sizeof(color));
            const float* X = d->point + 3 * p;
            const float* n = d->normal + 3 * p;
            const uint32_t obj = d->object ? d->object[p] : 0u;
            rttp::Result r;
            std::memcpy(r.out, color, sizeof(color));
            r.history = 1.0f;
            float motion[2] = {nan, nan};
            bool go = rttp::reprojectable(n, X, d->object != nullptr, obj);
            float carried_x[3], carried_n[3];
            if (go && kind != TemporalKind::PLAIN) {
                // a word outside the table has no history; a still object's texel goes on as it is; a moved one's is carried
                // (three ways with the triangle side: still, deformed -- carried by its previous triangle --, rigid)
                go = rttp::in_table(obj, d->n_objects);
                if (go && d->motions[obj].moved != 0u) {
                    rttp::Motion m;
                    std::memcpy(&m, d->motions + obj, sizeof(m));
                    if (kind == TemporalKind::DEFORMING && m.moved == rttp::DEFORMED) {
                        const uint32_t t = d->primitive[p];
                        const float u = d->bary[2 * p], v = d->bary[2 * p + 1];
                        go = rttp::has_prev_triangle(t, d->tri_first, d->n_prev_triangles, u, v);
                        if (go) {
                            rttp::Tri tri;
                            std::memcpy(&tri, d->prev_triangles + (t - d->tri_first), sizeof(tri));
                            go = rttp::carry_deformed(m, tri, u, v, (d->flags[p] & rttp::HIT_BACKFACE) != 0u, carried_x, carried_n);
                        }
                    } else {
                        go = rttp::carry(m, X, n, carried_x, carried_n);
                    }
                    X = carried_x;
                    n = carried_n;
                }
            }
            if (go) {
                const rttp::Where w = rttp::locate(c, X, (uint32_t)x, (uint32_t)y);
                if (w.on_screen) {
                    rttp::Tap taps[4];
                    for (int i = 0; i < 4; ++i) {
                        const int64_t qx = (int64_t)w.ax.i0 + rttp::tap_dx(i), qy = (int64_t)w.ay.i0 + rttp::tap_dy(i);
                        rttp::Tap& t = taps[i];
                        t.inside = qx >= 0 && qx < W && qy >= 0 && qy < H;
                        // (a tap outside the frame reads the nearest texel inside, as the kernel does, and is refused)
                        const int64_t cx = qx < 0 ? 0 : qx >= W ? W - 1 : qx, cy = qy < 0 ? 0 : qy >= H ? H - 1 : qy;
                        const size_t q = (size_t)(cy * W + cx);
                        for (int k = 0; k < 3; ++k) {
                            t.n[k] = d->prev_normal[3 * q + k];
                            t.x[k] = d->prev_point[3 * q + k];
                        }
                        std::memcpy(t.c, d->prev_color + 4 * q, sizeof(t.c));
                        t.h = d->prev_history[q];
                        t.obj = match_object ? d->prev_object[q] : 0u;
                    }
                    r = rttp::resolve(c, w, X, n, match_object, obj, color, taps);
                    motion[0] = w.motion[0];
                    motion[1] = w.motion[1];
                }
            }
            std::memcpy(d->out + 4 * p, r.out, sizeof(r.out));
            d->out_history[p] = r.history;
            if (d->motion) std::memcpy(d->motion + 2 * p, motion, sizeof(motion));
        }
    return RT_OK;
}

int temporal_host(const rt_temporal_desc* d, std::string& err) { return accumulate(d, TemporalKind::PLAIN, err); }
int temporal_motion_host(const rt_temporal_motion_desc* d, std::string& err) { return accumulate(d, TemporalKind::MOVING, err); }
int temporal_deform_host(const rt_temporal_deform_desc* d, std::string& err) { return accumulate(d, TemporalKind::DEFORMING, err); }

}  // namespace rt2
