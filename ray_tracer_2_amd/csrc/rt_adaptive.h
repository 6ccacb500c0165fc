// rt_adaptive.h -- the per-texel rules of adaptive sampling (include/rt_abi.h: rt_adaptive_plan, rt_adaptive_merge and their
// _host forms), shared by the host restatement (host/adaptive.cpp) and the device kernels
// (rt_adaptive.hip) so that both produce the same bits.
//
// The plan has one float step, binary32 and unfused (-ffp-contract=off):
//   q(p) = (u32)((sqrt_(v(p)) / sqrt_(M)) * 2^20)     for a finite v(p) > 0, M the largest such v; 0 otherwise
// and everything after it is integer arithmetic, so it does not depend on the order of evaluation:
//   F(c) = floor(c R / S) = mul_div_floor(c, R, S),   e(p) = F(C(p) + q(p)) - F(C(p)),   n(p) = min(min + e(p), max)
// The merge is the shader's blend (two products, then the sum) one sample at a time: Merge below.
#ifndef RT_ADAPTIVE_H
#define RT_ADAPTIVE_H

#include "rt_vdenoise.h"

namespace rtad {

constexpr float Q_ONE = 1048576.0f;      // 2^20: q of the texel that holds the maximum
constexpr uint32_t SEED_STRIDE = 719393u;   // (wgsl:475)

// The bits of a variance that takes part (finite and > 0), 0 for one that does not.  For these values the order of the bit
// patterns as u32 is the order of the floats: the maximum is an integer maximum.
RT_DN_HD uint32_t variance_key(float v) { return (rtdn::is_finite(v) && v > 0.0f) ? rtm::f2u(v) : 0u; }

// q of a texel; max_key: the maximum of variance_key over the frame (0: no texel takes part)
RT_DN_HD uint32_t quantise(float v, uint32_t max_key) {
    if (variance_key(v) == 0u || max_key == 0u) return 0u;
    return (uint32_t)((rtm::sqrt_(v) / rtm::sqrt_(rtm::u2f(max_key))) * Q_ONE);   // (in 0 .. 2^20: v <= M)
}

// floor(a b / d) exactly, for d > 0 and a quotient below 2^64 (a <= d gives a quotient <= b): a 64 x 64 -> 128 multiply
// in 32-bit pieces, then a restoring division, one bit of the product per step from its highest set bit down.
RT_DN_HD uint64_t mul_div_floor(uint64_t a, uint64_t b, uint64_t d) {
    const uint64_t a0 = a & 0xffffffffull, a1 = a >> 32, b0 = b & 0xffffffffull, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (p01 & 0xffffffffull) + (p10 & 0xffffffffull);   // (< 3 * 2^32)
    const uint64_t lo = (p00 & 0xffffffffull) | (mid << 32);
    const uint64_t hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
    const int bits = hi != 0u ? 128 - __builtin_clzll(hi) : lo != 0u ? 64 - __builtin_clzll(lo) : 0;
    uint64_t rem = 0u, quo = 0u;
    for (int i = bits - 1; i >= 0; --i) {
        const uint64_t bit = i >= 64 ? (hi >> (i - 64)) & 1u : (lo >> i) & 1u;
        const bool carry = (rem >> 63) != 0u;   // (rem < d; twice that may pass 2^64, and then certainly holds d)
        rem = (rem << 1) | bit;
        quo <<= 1;
        if (carry || rem >= d) {
            rem -= d;
            quo |= 1u;
        }
    }
    return quo;
}

// n of a texel from F at its two ends of the scan; over: did max_samples clamp it
RT_DN_HD uint32_t samples_of(uint64_t f_begin, uint64_t f_end, uint32_t min_samples, uint32_t max_samples, bool& over) {
    const uint64_t want = (uint64_t)min_samples + (f_end - f_begin);
    over = want > (uint64_t)max_samples;
    return over ? max_samples : (uint32_t)want;
}

// the seed of texel `index` (y * width + x) in frame first_frame + k, in u32 arithmetic
RT_DN_HD uint32_t sample_seed(uint32_t index, uint32_t first_frame, uint32_t k) { return index + (first_frame + k) * SEED_STRIDE; }

RT_DN_HD bool finite4(const float c[4]) {
    return rtdn::is_finite(c[0]) && rtdn::is_finite(c[1]) && rtdn::is_finite(c[2]) && rtdn::is_finite(c[3]);
}

// A texel's accumulation while its samples are merged.  al: a' of the texel (ones with no albedo plane); with_moments: is m kept.
struct Merge {
    float acc[4], m[4], hl;
    RT_DN_HD void start(const float color[4], float history, const float moments[4]) {
        for (int k = 0; k < 4; ++k) {
            acc[k] = color[k];
            m[k] = moments[k];
        }
        hl = (rtdn::is_finite(history) && history >= 1.0f && finite4(color)) ? history : 0.0f;
    }
    RT_DN_HD void sample(const float c[4], const float al[3], float max_history, bool with_moments) {
        if (!finite4(c)) return;
        float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (with_moments) {
            const float l = rtvd::luminance(c[0] / al[0], c[1] / al[1], c[2] / al[2]);
            s[0] = l;
            s[1] = l * l;
        }
        if (hl == 0.0f) {
            for (int k = 0; k < 4; ++k) {
                acc[k] = c[k];
                m[k] = s[k];
            }
            hl = 1.0f;
            return;
        }
        const float n_c = hl < max_history ? hl : max_history;
        const float w = 1.0f / (n_c + 1.0f);
        const float rest = 1.0f - w;
        for (int k = 0; k < 4; ++k) {
            acc[k] = acc[k] * rest + c[k] * w;
            if (with_moments) m[k] = m[k] * rest + s[k] * w;
        }
        hl = n_c + 1.0f;
    }
};

}  // namespace rtad

#endif
