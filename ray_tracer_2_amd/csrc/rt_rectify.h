// rt_rectify.h -- the per-texel arithmetic of history rectification (include/rt_abi.h: rt_temporal_rectify,
// rt_temporal_rectify_host), shared by the host restatement (host/rectify.cpp) and the device
// kernel (rt_rectify.hip) so that both produce the same bits.
//
// Everything here is binary32 and unfused (-ffp-contract=off), written in the order the definition gives.  A texel is
// worked in two steps with the caller's loads between them:
//   Sums::add -- one tap of the window, in the defined order (dy outer, dx inner);
//   resolve   -- the box of the sums, the clamp of the history, the cut of its length and the blend.
// What a tap that does not count adds is +0, chosen by a select: s1 starts at +0 and is never -0 (a sum is -0 only when
// both terms are), s2 adds squares, so adding +0 leaves both as they are, bit for bit, and no branch stands between the
// taps' reads.
#ifndef RT_RECTIFY_H
#define RT_RECTIFY_H

#include <stdint.h>

#include "rt_temporal.h"   // (rttp::is_finite, f2u; rtm::sqrt_, the correctly rounded square root of host and device)

namespace rtrc {

constexpr int MAX_RADIUS = 3;
constexpr uint8_t KEPT = 1, CLIPPED = 2;   // the bytes of out_clipped (0: the texel had no history)

// What the kernel and the host loop receive once per call.
struct Call {
    uint32_t width, height;
    int32_t radius;
    float clip_sigma, clip_history;
};

RT_TP_HD bool finite4(const float a[4]) { return rttp::finite3(a) && rttp::is_finite(a[3]); }

// Has texel p a history?  h: history(p), n: history_length(p).
RT_TP_HD bool has_history(const float h[4], float n) { return finite4(h) && rttp::is_finite(n) && n >= 1.0f; }

// The window's sums.  add: tap q's rgb, counted (`take`: inside the frame, rgb finite, the object words equal) or not.
struct Sums {
    float s1[3] = {0.0f, 0.0f, 0.0f}, s2[3] = {0.0f, 0.0f, 0.0f};
    uint32_t c = 0u;
    RT_TP_HD void add(bool take, float r, float g, float b) {
        const float v[3] = {r, g, b};
        for (int k = 0; k < 3; ++k) {
            const float x = take ? v[k] : 0.0f;
            s1[k] += x;
            s2[k] += x * x;
        }
        c += take ? 1u : 0u;
    }
    // The same for a tap whose reader has already put zeros in the place of an rgb that does not count (the device
    // kernel's LDS records without an object plane): `counted` is 1 or 0, and what a 0 adds is add's +0.
    RT_TP_HD void add_staged(float r, float g, float b, uint32_t counted) {
        const float v[3] = {r, g, b};
        for (int k = 0; k < 3; ++k) {
            s1[k] += v[k];
            s2[k] += v[k] * v[k];
        }
        c += counted;
    }
};

struct Result {
    float out[4], history, moments[4];
    uint8_t clipped;
};

// Sums -> box -> clamp -> length -> blend.  color: this frame's sample; h, n: the reprojected history and its length; m, hm:
// this frame's moments and the reprojected ones (read only with have_moments).
RT_TP_HD Result resolve(const Call& c, const Sums& s, const float color[4], const float h[4], float n, bool have_moments,
                        const float m[4], const float hm[4]) {
    Result r;
    if (!has_history(h, n)) {
        for (int k = 0; k < 4; ++k) r.out[k] = color[k], r.moments[k] = have_moments ? m[k] : 0.0f;
        r.history = 1.0f;
        r.clipped = 0u;
        return r;
    }
    float hp[4] = {h[0], h[1], h[2], h[3]};
    bool clipped = false;
    if (s.c >= 2u && rttp::is_finite(c.clip_sigma)) {   // (clip_sigma is >= 0 and not NaN: not finite is +INF)
        const float cnt = (float)s.c;
        for (int k = 0; k < 3; ++k) {
            const float mu = s.s1[k] / cnt, m2 = s.s2[k] / cnt;
            float v = m2 - mu * mu;
            v = v > 0.0f ? v : 0.0f;
            const float sd = rtm::sqrt_(v);
            const float lo = mu - c.clip_sigma * sd, hi = mu + c.clip_sigma * sd;
            hp[k] = h[k] < lo ? lo : (h[k] > hi ? hi : h[k]);
            clipped = clipped || rttp::f2u(hp[k]) != rttp::f2u(h[k]);
        }
    }
    const float n_c = clipped && c.clip_history < n ? c.clip_history : n;
    const float w = 1.0f / (n_c + 1.0f);
    const float rest = 1.0f - w;
    const bool sample_ok = finite4(color);
    for (int k = 0; k < 4; ++k) r.out[k] = sample_ok ? hp[k] * rest + color[k] * w : hp[k];
    r.history = sample_ok ? n_c + 1.0f : n_c;
    r.clipped = clipped ? CLIPPED : KEPT;
    if (have_moments) {
        const bool hm_ok = finite4(hm), m_ok = finite4(m);
        for (int k = 0; k < 4; ++k) r.moments[k] = !hm_ok ? m[k] : !m_ok ? hm[k] : hm[k] * rest + m[k] * w;
    } else {
        for (int k = 0; k < 4; ++k) r.moments[k] = 0.0f;
    }
    return r;
}

}  // namespace rtrc

#endif
