// rt_vdenoise.h -- the per-texel and per-tap arithmetic of the variance-guided a-trous denoiser (include/rt_abi.h:
// rt_denoise_variance, rt_luminance_moments and their _host forms), shared by the host restatement
// (host/vdenoise.cpp) and the device kernels (rt_vdenoise.hip) so that both produce the same bits.  What the filter has in
// common with rt_denoise -- filterable, albedo_floor, d2, kernel_h, k_of_sigma, is_finite -- is csrc/rt_denoise.h.
//
// Everything here is binary32 and unfused (-ffp-contract=off; the only fused operations are the explicit fma of
// rtm::exp_), written in the order the definition gives:
//   l(c)   = (0.2126 c0 + 0.7152 c1) + 0.0722 c2
//   var_0  = (m2 - m1 m1) / history                 where the accumulated moments serve (temporal_serves), otherwise
//            m2 - m1 m1 with m1 = s1 / sw, m2 = s2 / sw of the 7 x 7 window weighted by u = exp_(-(d2(normal) k_n + d2(point) k_x));
//            either way clamped: v > 0 ? v : 0
//   D      = sigma_luminance sqrt_(G) + 2^-30,      G the 3 x 3 mean of var_i under g = {1/4, 1/2, 1/4}
//   e      = (|l_p - l_q| / D + d2(normal) k_n) + d2(point) k_x
//   w      = (h[dx] h[dy]) exp_(-e)
//   c_i+1  = sum(w c_i) / sum(w),   var_i+1 = sum((w w) var_i) / (sum(w) sum(w))
// A tap whose weight is not > 0 (zero after the exponential's underflow, or NaN) is skipped.
#ifndef RT_VDENOISE_H
#define RT_VDENOISE_H

#include "rt_denoise.h"

namespace rtvd {

RT_DN_HD float luminance(float c0, float c1, float c2) { return (0.2126f * c0 + 0.7152f * c1) + 0.0722f * c2; }

// g[d + 1] for d = -1 .. 1: the prefilter of the variance
RT_DN_HD float kernel_g(int d) { return d == 0 ? 0.5f : 0.25f; }

// Do the accumulated moments of a texel give its variance?  (history: frames accumulated in them)
RT_DN_HD bool temporal_serves(float m1, float m2, float history, float min_history) {
    return rtdn::is_finite(history) && history >= min_history && rtdn::is_finite(m1) && rtdn::is_finite(m2);
}
RT_DN_HD float temporal_variance(float m1, float m2, float history) { return (m2 - m1 * m1) / history; }
RT_DN_HD float spatial_variance(float s1, float s2, float sw) {
    const float m1 = s1 / sw, m2 = s2 / sw;
    return m2 - m1 * m1;
}
RT_DN_HD float clamp_variance(float v) { return v > 0.0f ? v : 0.0f; }   // (a NaN gives 0)

// u of one tap of the 7 x 7 window: the geometry terms alone
RT_DN_HD float window_weight(const float np[3], const float nq[3], const float xp[3], const float xq[3], float k_n, float k_x) {
    const float e = rtdn::d2(np[0], np[1], np[2], nq[0], nq[1], nq[2]) * k_n + rtdn::d2(xp[0], xp[1], xp[2], xq[0], xq[1], xq[2]) * k_x;
    return rtm::exp_(-e);
}

// D of a texel in one pass, from the prefiltered variance G
RT_DN_HD float luminance_scale(float sigma_luminance, float G) { return sigma_luminance * rtm::sqrt_(G) + 0x1p-30f; }

// w of one tap: hw = h[dx] h[dy]; lp / lq the luminances of c_i at p and q
RT_DN_HD float tap_weight(float hw, float lp, float lq, float D, const float np[3], const float nq[3], const float xp[3],
                          const float xq[3], float k_n, float k_x) {
    const float e = (rtm::abs_(lp - lq) / D + rtdn::d2(np[0], np[1], np[2], nq[0], nq[1], nq[2]) * k_n) +
                    rtdn::d2(xp[0], xp[1], xp[2], xq[0], xq[1], xq[2]) * k_x;
    return hw * rtm::exp_(-e);
}

}  // namespace rtvd

#endif
