// rt_upsample.h -- the per-texel arithmetic of guided upsampling (include/rt_abi.h: rt_upsample, rt_upsample_host;
// DESIGN.md section 2.18), shared by the host restatement (host/upsample.cpp) and the device kernel (rt_upsample.hip) so
// that both produce the same bits.
//
// Everything here is binary32 and unfused (-ffp-contract=off), written in the order the definition gives.  The snap, the
// four bilinear taps' order and weights and the finite / non-zero tests are rt_temporal.h's, the albedo floor of the
// demodulation is rt_denoise.h's.  A texel is worked in steps with the caller's loads between them:
//   classify -- is the high texel GUIDED?
//   locate   -- where does it fall in the low frame (snap)?
//   make_tap -- what a low texel says about itself, whoever taps it (the tiled kernel does this once per tile).
//   Sums::add per tap of a ring -- is the tap valid, and what does it add?  An invalid tap adds +0, chosen by a select
//               after the tap's arithmetic: sum and wsum start at +0 and are never -0, so adding +0 leaves them as they
//               are, bit for bit, and no branch stands between the taps' loads.
//   finish   -- v = sum / wsum, or the nearest texel's c(q), remodulated.
#ifndef RT_UPSAMPLE_H
#define RT_UPSAMPLE_H

#include <stdint.h>

#include "rt_denoise.h"    // (rtdn::albedo_floor)
#include "rt_temporal.h"   // (rttp::snap_axis, tap_weight, tap_dx / tap_dy, is_finite, finite3, some_nonzero3)

#if defined(__HIPCC__)
#define RT_UP_HD __host__ __device__ __forceinline__
#else
#define RT_UP_HD inline
#endif

namespace rtup {

constexpr uint8_t COVER_RING1 = 2, COVER_RING2 = 1, COVER_HOLE = 0;

// What the kernel and the host loop receive once per call.
struct Call {
    uint32_t lo_width, lo_height, width, height;
    float rx, ry;   // low texels per high texel, per axis
    float point_tolerance, normal_cos;
};

// rx of one axis: (f32(lo) - 1) / (f32(hi) - 1), 0 for a high frame one texel wide
RT_UP_HD float ratio(uint32_t lo, uint32_t hi) { return hi == 1u ? 0.0f : ((float)lo - 1.0f) / ((float)hi - 1.0f); }

// The high texel P as loaded.
struct Texel {
    float n[3], x[3], depth;
    uint32_t obj;
};

// em: the rgb of emission(P), zeros when there is no emission plane
RT_UP_HD bool guided(const Texel& p, const float em[3]) {
    return rttp::some_nonzero3(p.n) && rttp::finite3(p.n) && rttp::finite3(p.x) && rttp::is_finite(p.depth) && p.depth > 0.0f &&
           p.obj != rttp::NO_OBJECT && em[0] == 0.0f && em[1] == 0.0f && em[2] == 0.0f;
}

struct Where {
    rttp::Axis ax, ay;
};
RT_UP_HD Where locate(const Call& c, uint32_t X, uint32_t Y) {
    return Where{rttp::snap_axis((float)X * c.rx), rttp::snap_axis((float)Y * c.ry)};
}

// One low texel q as a tap holds it (made from a texel inside the frame: `inside` says whether it is q itself): what it
// says about itself is settled once -- plain_ok: inside the frame with a finite colour; geom_ok: a hit with a finite normal
// and point; d: the colour's rgb demodulated by lo_albedo(q), there when the call has the albedo planes.
struct Tap {
    float c[4], d[3], x[3], n[3];
    uint32_t obj;
    bool plain_ok, geom_ok;
};
// al: lo_albedo(q).rgb, read only when have_albedo
RT_UP_HD Tap make_tap(bool inside, const float c[4], const float x[3], const float n[3], uint32_t obj, bool have_albedo, const float al[3]) {
    Tap t;
    for (int k = 0; k < 3; ++k) {
        t.c[k] = c[k];
        t.d[k] = have_albedo ? c[k] / rtdn::albedo_floor(al[k]) : c[k];
        t.x[k] = x[k];
        t.n[k] = n[k];
    }
    t.c[3] = c[3];
    t.obj = obj;
    t.plain_ok = inside && rttp::is_finite(c[0]) && rttp::is_finite(c[1]) && rttp::is_finite(c[2]) && rttp::is_finite(c[3]);
    t.geom_ok = rttp::some_nonzero3(n) && rttp::finite3(n) && rttp::finite3(x);
    return t;
}

// Weight of ring 2's tap (i, j), i, j = -1 .. 2
RT_UP_HD float tent(int i, float t) {
    const float d = (float)i - t;
    return 1.0f - rttp::u2f(rttp::f2u(d) & 0x7fffffffu) * 0.5f;
}
RT_UP_HD float ring2_weight(int i, int j, float tx, float ty) { return tent(i, tx) * tent(j, ty); }

RT_UP_HD bool tap_valid(float b, const Tap& t, const Texel& p, bool is_guided, float reach, float normal_cos) {
    const float a[3] = {t.x[0] - p.x[0], t.x[1] - p.x[1], t.x[2] - p.x[2]};
    const float plane = (a[0] * p.n[0] + a[1] * p.n[1]) + a[2] * p.n[2];
    const float cosine = (p.n[0] * t.n[0] + p.n[1] * t.n[1]) + p.n[2] * t.n[2];
    const float dist = rttp::u2f(rttp::f2u(plane) & 0x7fffffffu);
    const bool geometry = t.geom_ok && dist <= reach && cosine >= normal_cos;
    return b > 0.0f && t.plain_ok && t.obj == p.obj && (!is_guided || geometry);
}

// c(q): demod says P is GUIDED and both albedo planes are given
RT_UP_HD void tap_color(const Tap& t, bool demod, float c[4]) {
    for (int k = 0; k < 3; ++k) c[k] = demod ? t.d[k] : t.c[k];
    c[3] = t.c[3];
}

struct Sums {
    float sum[4] = {0.0f, 0.0f, 0.0f, 0.0f}, wsum = 0.0f;
    RT_UP_HD void add(float b, const Tap& t, const Texel& p, bool is_guided, bool demod, float reach, float normal_cos) {
        const bool take = tap_valid(b, t, p, is_guided, reach, normal_cos);
        float c[4];
        tap_color(t, demod, c);
        for (int k = 0; k < 4; ++k) sum[k] += take ? b * c[k] : 0.0f;
        wsum += take ? b : 0.0f;
    }
    RT_UP_HD bool have() const { return wsum > 0.0f; }
    RT_UP_HD void mean(float v[4]) const {
        for (int k = 0; k < 4; ++k) v[k] = sum[k] / wsum;
    }
};

// The nearest low texel of a hole, per axis, clamped into [0, n)
RT_UP_HD uint32_t nearest(const rttp::Axis& a, uint32_t n) {
    const int32_t q = a.i0 + (a.t > 0.5f ? 1 : 0);
    return q < 0 ? 0u : (uint32_t)q >= n ? n - 1u : (uint32_t)q;
}

// out(P) from v: al = albedo(P).rgb, read only when the call demodulates
RT_UP_HD void finish(const float v[4], bool demod, const float al[3], float out[4]) {
    for (int k = 0; k < 3; ++k) out[k] = demod ? v[k] * al[k] : v[k];
    out[3] = v[3];
}

}  // namespace rtup

#endif
