// rt_temporal.h -- the per-texel arithmetic of temporal accumulation (include/rt_abi.h: rt_temporal_accumulate,
// rt_temporal_accumulate_host), shared by the host restatement (host/temporal.cpp) and the device
// kernel (rt_temporal.hip) so that both produce the same bits.
//
// Everything here is binary32 and unfused (-ffp-contract=off), written in the order the definition gives.  A texel is
// worked in two steps with the caller's loads between them:
//   locate  -- is the texel reprojectable, where does its hit point fall in the previous frame (project), is that on
//              screen, and which texels and weights does the snapped position take (snap)?
//   resolve -- given the four taps' previous values: which of them are valid, what do they add, and the blend.
// With a motion table (rt_temporal_accumulate_moving) a moved object's texel goes through `carry` first, and locate and
// resolve then work on the carried point and normal.  A deformed mesh's texel (rt_temporal_accumulate_deforming) is
// carried by its previous triangle instead (`carry_deformed`).
// What an invalid tap adds is +0, chosen by a select after the tap's arithmetic: sum, hsum and wsum start at +0 and are
// never -0, so adding +0 leaves them as they are, bit for bit, and no branch stands between the taps' loads.
#ifndef RT_TEMPORAL_H
#define RT_TEMPORAL_H

#include <stdint.h>

#include "rt_transc.h"   // (rtm::sqrt_, the correctly rounded square root of host and device)

#if defined(__HIPCC__)
#define RT_TP_HD __host__ __device__ __forceinline__
#else
#define RT_TP_HD inline
#endif

namespace rttp {

constexpr float SNAP = 0.015625f;            // S = 1/64 texel
constexpr uint32_t QUIET_NAN = 0x7fc00000u;  // what `motion` holds where nothing was reprojected
constexpr uint32_t NO_OBJECT = 0xffffffffu;

// What the kernel and the host loop receive once per call: V = mat4_inverse(prev_camera.cam_to_world) (rows 0 .. 2 of its
// four columns), the previous camera's view_params and the desc's three numbers.
struct Call {
    float v[4][3];   // V[col][row]
    float pw, ph, fd;
    float max_history, point_tolerance, normal_cos;
    uint32_t width, height;
};

RT_TP_HD uint32_t f2u(float x) { return __builtin_bit_cast(uint32_t, x); }
RT_TP_HD float u2f(uint32_t u) { return __builtin_bit_cast(float, u); }
RT_TP_HD bool is_finite(float x) { return (f2u(x) & 0x7f800000u) != 0x7f800000u; }
RT_TP_HD bool finite3(const float a[3]) { return is_finite(a[0]) && is_finite(a[1]) && is_finite(a[2]); }
RT_TP_HD bool some_nonzero3(const float a[3]) { return !(a[0] == 0.0f && a[1] == 0.0f && a[2] == 0.0f); }   // (a NaN is non-zero)

// Is the current texel reprojectable?  obj: its object word, NO_OBJECT's complement of anything when there is no plane.
RT_TP_HD bool reprojectable(const float n[3], const float x[3], bool have_object, uint32_t obj) {
    return some_nonzero3(n) && finite3(n) && finite3(x) && !(have_object && obj == NO_OBJECT);
}

// One axis of the snap: f -> (i0, t), the texel and the weight of its upper neighbour.  f is in (-1, 2^31).
struct Axis {
    int32_t i0;
    float t;
};
RT_TP_HD Axis snap_axis(float f) {
    const float fl = __builtin_floorf(f);
    Axis a{(int32_t)fl, f - fl};   // (f32(i0) is fl again: |fl| < 2^31 is an integer a float holds)
    if (a.t <= SNAP) {
        a.t = 0.0f;
    } else if (a.t >= 1.0f - SNAP) {
        a.i0 += 1;
        a.t = 0.0f;
    }
    return a;
}

struct Where {
    bool on_screen;    // false: the "no history" result with NaN motion
    float l2;          // view depth in the previous frame
    Axis ax, ay;
    float motion[2];
};

// project + on screen + snap for the hit point X of texel (x, y)
RT_TP_HD Where locate(const Call& c, const float X[3], uint32_t x, uint32_t y) {
    float l[3];
    for (int k = 0; k < 3; ++k) l[k] = ((c.v[0][k] * X[0] + c.v[1][k] * X[1]) + c.v[2][k] * X[2]) + c.v[3][k];
    const float W = (float)c.width, H = (float)c.height;
    const float ux = ((l[0] / l[2]) * c.fd) / c.pw + 0.5f;
    const float uy = ((l[1] / l[2]) * c.fd) / c.ph + 0.5f;
    const float fx = ux * (W - 1.0f), fy = uy * (H - 1.0f);
    Where w{};
    w.l2 = l[2];
    w.on_screen = l[2] > 0.0f && fx > -1.0f && fx < W && fy > -1.0f && fy < H;
    if (!w.on_screen) return w;
    w.ax = snap_axis(fx);
    w.ay = snap_axis(fy);
    w.motion[0] = ((float)w.ax.i0 + w.ax.t) - (float)x;
    w.motion[1] = ((float)w.ay.i0 + w.ay.t) - (float)y;
    return w;
}

// Tap i of the four, in the defined order: its offset from (x0, y0) and its bilinear weight.
RT_TP_HD int tap_dx(int i) { return i & 1; }
RT_TP_HD int tap_dy(int i) { return i >> 1; }
RT_TP_HD float tap_weight(int i, float tx, float ty) {
    const float wx = tap_dx(i) ? tx : 1.0f - tx, wy = tap_dy(i) ? ty : 1.0f - ty;
    return wx * wy;
}

// The previous frame's values at one tap, as loaded (from a texel inside the frame: `inside` says whether it is q itself).
struct Tap {
    float n[3], x[3], c[4], h;
    uint32_t obj;
    bool inside;
};

RT_TP_HD bool tap_valid(float b, const Tap& t, const float X[3], const float n[3], bool match_object, uint32_t obj, float reach,
                        float normal_cos) {
    const float a[3] = {t.x[0] - X[0], t.x[1] - X[1], t.x[2] - X[2]};
    const float plane = (a[0] * n[0] + a[1] * n[1]) + a[2] * n[2];
    const float cosine = (n[0] * t.n[0] + n[1] * t.n[1]) + n[2] * t.n[2];
    const float dist = u2f(f2u(plane) & 0x7fffffffu);
    return b > 0.0f && t.inside && some_nonzero3(t.n) && finite3(t.n) && finite3(t.x) && is_finite(t.c[0]) && is_finite(t.c[1]) &&
           is_finite(t.c[2]) && is_finite(t.c[3]) && is_finite(t.h) && t.h >= 1.0f && !(match_object && t.obj != obj) &&
           dist <= reach && cosine >= normal_cos;
}

struct Result {
    float out[4], history;
};

// Taps -> sums -> blend.  color: the current sample; where: of locate (on screen).
RT_TP_HD Result resolve(const Call& c, const Where& where, const float X[3], const float n[3], bool match_object, uint32_t obj,
                        const float color[4], const Tap taps[4]) {
    const float reach = c.point_tolerance * where.l2;
    float sum[4] = {0.0f, 0.0f, 0.0f, 0.0f}, hsum = 0.0f, wsum = 0.0f;
    for (int i = 0; i < 4; ++i) {
        const float b = tap_weight(i, where.ax.t, where.ay.t);
        const bool take = tap_valid(b, taps[i], X, n, match_object, obj, reach, c.normal_cos);
        for (int k = 0; k < 4; ++k) sum[k] += take ? b * taps[i].c[k] : 0.0f;
        hsum += take ? b * taps[i].h : 0.0f;
        wsum += take ? b : 0.0f;
    }
    Result r;
    if (!(wsum > 0.0f)) {
        for (int k = 0; k < 4; ++k) r.out[k] = color[k];
        r.history = 1.0f;
        return r;
    }
    const float hist = hsum / wsum;
    const float n_c = hist < c.max_history ? hist : c.max_history;
    const float w = 1.0f / (n_c + 1.0f);
    const float rest = 1.0f - w;
    const bool sample_ok = is_finite(color[0]) && is_finite(color[1]) && is_finite(color[2]) && is_finite(color[3]);
    for (int k = 0; k < 4; ++k) {
        const float prev = sum[k] / wsum;
        r.out[k] = sample_ok ? prev * rest + color[k] * w : prev;
    }
    r.history = sample_ok ? n_c + 1.0f : n_c;
    return r;
}

// ---- moving objects (include/rt_abi.h: rt_temporal_accumulate_moving) ----
// A record of the motion table, rt_object_motion's 96 bytes as both units read them: the device table is 16-byte aligned
// (the entry point checks), the host loop copies a record into one of these.
struct alignas(16) Motion {
    float d[4][3];    // current world -> previous world, [col][row]
    float nt[3][3];   // [col][row]: the previous-world normal before normalisation
    uint32_t moved;
    uint32_t _p[2];
};

// Which way a reprojectable texel with object word `obj` goes under a table of n_objects records (`object` is required
// with a table, so a reprojectable texel's word is not NO_OBJECT): a word outside the table has no history; inside it, a
// record with moved == 0 leaves the texel as it is -- its matrices are not read -- and any other carries it (carry).
RT_TP_HD bool in_table(uint32_t obj, uint32_t n_objects) { return obj < n_objects; }

// X, n of the current world -> X', n' of the previous world by a moved object's record.  False: some component is not
// finite (a zero length included) and the texel has no history.
RT_TP_HD bool carry(const Motion& m, const float X[3], const float n[3], float Xp[3], float np[3]) {
    float v[3];
    for (int r = 0; r < 3; ++r) {
        Xp[r] = ((m.d[0][r] * X[0] + m.d[1][r] * X[1]) + m.d[2][r] * X[2]) + m.d[3][r];
        v[r] = (m.nt[0][r] * n[0] + m.nt[1][r] * n[1]) + m.nt[2][r] * n[2];
    }
    const float len = rtm::sqrt_((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    for (int r = 0; r < 3; ++r) np[r] = v[r] / len;
    return finite3(Xp) && finite3(np);
}

// ---- deforming meshes (include/rt_abi.h: rt_temporal_accumulate_deforming) ----
// A record whose `moved` is DEFORMED carries its texels by the previous frame's triangle, not by one map: m.d is the
// previous model_to_world and m.nt its 3 x 3 (rt_object_motions_deforming).
constexpr uint32_t DEFORMED = 2u;
constexpr uint32_t HIT_BACKFACE = 2u;   // RT_HIT_BACKFACE of the G-buffer's flags plane

// rt_packed_triangle's 96 bytes as both units read them: six 16-byte rows, v1|uv .. n3|uv.  The device array is 16-byte
// aligned (the entry point checks), the host loop copies a record into one of these.
struct alignas(16) Tri {
    float v1[3], uv10, v2[3], uv11, v3[3], uv20, n1[3], uv21, n2[3], uv30, n3[3], uv31;
};

// May the previous triangle of a deformed texel be read?  t: its primitive word, (u, v): its barycentrics.  The array is
// touched only after this says yes.
RT_TP_HD bool has_prev_triangle(uint32_t t, uint32_t tri_first, uint32_t n_prev_triangles, float u, float v) {
    return t >= tri_first && t - tri_first < n_prev_triangles && is_finite(u) && is_finite(v);
}

// The surface point (u, v) of the previous triangle T -> X', n' of the previous world by a deformed object's record: one
// interpolation of the vertices and one of the normals in the render kernel's order, one normalisation, the backface
// sign.  False: some component is not finite (normals that interpolate to zero length included) and the texel has no history.
RT_TP_HD bool carry_deformed(const Motion& m, const Tri& T, float u, float v, bool backface, float Xp[3], float np[3]) {
    const float w = (1.0f - u) - v;
    float xm[3], g[3], q[3];
    for (int r = 0; r < 3; ++r) {
        xm[r] = (T.v1[r] * w + T.v2[r] * u) + T.v3[r] * v;
        g[r] = (T.n1[r] * w + T.n2[r] * u) + T.n3[r] * v;
    }
    for (int r = 0; r < 3; ++r) {
        Xp[r] = ((m.d[0][r] * xm[0] + m.d[1][r] * xm[1]) + m.d[2][r] * xm[2]) + m.d[3][r];
        q[r] = (m.nt[0][r] * g[0] + m.nt[1][r] * g[1]) + m.nt[2][r] * g[2];
    }
    const float len = rtm::sqrt_((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]);
    const float s = backface ? -1.0f : 1.0f;
    for (int r = 0; r < 3; ++r) np[r] = (q[r] / len) * s;
    return finite3(Xp) && finite3(np);
}

}  // namespace rttp

#endif
