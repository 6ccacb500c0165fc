// rt_denoise.h -- the per-texel and per-tap arithmetic of the G-buffer-guided a-trous denoiser (include/rt_abi.h:
// rt_denoise, rt_denoise_host), shared by the host restatement (host/denoise.cpp) and the device
// kernels (rt_denoise.hip) so that both produce the same bits.
//
// Everything here is binary32 and unfused (-ffp-contract=off; the only fused operations are the explicit fma of
// rtm::exp_), written in the order the definition gives:
//   d2(a)  = ((a0 a0 + a1 a1) + a2 a2)                       of a componentwise difference p - q
//   e      = (d2(c) k_c + d2(normal) k_n) + d2(point) k_x
//   w      = (h[dx] h[dy]) exp_(-e),  h = {1/16, 1/4, 3/8, 1/4, 1/16} -- powers of two and 3/8: the product is exact
// A tap whose w is not > 0 (zero after the exponential's underflow, or NaN from an overflowed difference) is skipped.
#ifndef RT_DENOISE_H
#define RT_DENOISE_H

#include <stdint.h>

#include "rt_transc.h"

#if defined(__HIPCC__)
#define RT_DN_HD __host__ __device__ __forceinline__
#else
#define RT_DN_HD inline
#endif

namespace rtdn {

RT_DN_HD bool is_finite(float x) { return (rtm::f2u(x) & 0x7f800000u) != 0x7f800000u; }

// h[d + 2] for d = -2 .. 2
RT_DN_HD float kernel_h(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }

// Is the texel filtered (and a tap of its neighbours)?  normal: some component non-zero (a miss has zeros); normal, point and
// the colour's rgb finite; no emission (em: the texel's rgb, zeros when there is no emission plane).
RT_DN_HD bool filterable(const float n[3], const float x[3], const float c[3], const float em[3]) {
    if (n[0] == 0.0f && n[1] == 0.0f && n[2] == 0.0f) return false;   // (a NaN component is "non-zero" here and fails below)
    for (int k = 0; k < 3; ++k)
        if (!is_finite(n[k]) || !is_finite(x[k]) || !is_finite(c[k])) return false;
    return em[0] == 0.0f && em[1] == 0.0f && em[2] == 0.0f;
}

// a' of the demodulation: the albedo component, floored at 2^-10 (a NaN albedo takes the floor)
RT_DN_HD float albedo_floor(float a) { return a > 0x1p-10f ? a : 0x1p-10f; }

RT_DN_HD float d2(float p0, float p1, float p2, float q0, float q1, float q2) {
    const float a0 = p0 - q0, a1 = p1 - q1, a2 = p2 - q2;
    return ((a0 * a0 + a1 * a1) + a2 * a2);
}

// w of one tap: hw = h[dx] h[dy]; cp / cq, np / nq, xp / xq: demodulated colour, normal and point of p and q
RT_DN_HD float tap_weight(float hw, const float cp[3], const float cq[3], const float np[3], const float nq[3], const float xp[3],
                       const float xq[3], float k_c, float k_n, float k_x) {
    const float e = (d2(cp[0], cp[1], cp[2], cq[0], cq[1], cq[2]) * k_c + d2(np[0], np[1], np[2], nq[0], nq[1], nq[2]) * k_n) +
                    d2(xp[0], xp[1], xp[2], xq[0], xq[1], xq[2]) * k_x;
    return hw * rtm::exp_(-e);
}

// 1 / sigma^2 (sigma = +INF: 0)
RT_DN_HD float k_of_sigma(float sigma) { return 1.0f / (sigma * sigma); }
// k_c of pass i: k_c 4^i, an exact scaling
RT_DN_HD float k_c_of_pass(float k_c, int i) { return k_c * (float)(1u << (2 * i)); }

}  // namespace rtdn

#endif
