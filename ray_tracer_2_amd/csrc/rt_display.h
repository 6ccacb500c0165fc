// rt_display.h -- the per-texel arithmetic of the display pass and the exposure meter (include/rt_abi.h: rt_display,
// rt_auto_exposure and their _host forms), shared by the host restatement (host/display.cpp) and
// the device kernels (rt_display.hip) so that both produce the same bits.  Everything is binary32, every operation rounded
// once (-ffp-contract=off), and no transcendental function is called: the sRGB transfer is a search of 255 thresholds
// (rt_srgb_encode_lut.h), the meter's logarithm the float's own exponent and top three mantissa bits.
//
//   e      = exposure, or exposure * scale for a scale that is finite and > 0
//   m      = v >= 0 ? min(v, 2^64) : 0                   with v = color_k * e, k = 0 .. 2 (NaN and negatives: 0)
//   t      = m (CLAMP), or (m * (1 + m / (white * white))) / (1 + m) (REINHARD)
//   byte   = #{k in 1 .. 255: t >= T[k]} (SRGB), or (uint32)(l * 255 + 0.5) with l = t > 0 ? min(t, 1) : 0 (LINEAR; alpha,
//            always, on color_3 as it is)
//   bin(Y) = clamp((bits(Y) >> 20) - 888, 0, 255)         for Y > 0 and < +inf, Y = rtvd::luminance(color)
#ifndef RT_DISPLAY_H
#define RT_DISPLAY_H

#include <stdint.h>

#include "rt_srgb_encode_lut.h"
#include "rt_vdenoise.h"   // (rtvd::luminance; rtm::f2u / u2f through rt_transc.h)

namespace rtdp {

constexpr uint32_t TONE_CLAMP = 0u, TONE_REINHARD = 1u, TRANSFER_SRGB = 0u, TRANSFER_LINEAR = 1u;
constexpr uint32_t LAYOUT_BGRA = 1u, LAYOUT_TOP_FIRST = 2u;
constexpr uint32_t T_COUNT = RT_SRGB_ENCODE_T_COUNT, BUCKETS = RT_SRGB_ENCODE_BUCKETS, STEPS = RT_SRGB_ENCODE_STEPS;
constexpr uint32_t BINS = 256u;
constexpr int32_t BIN_FIRST = 888;   // (bits(2^-16) >> 20: eight bins per octave from there)

// The once-per-call numbers of rt_display (host/display.cpp: display_call).
struct Call {
    uint32_t width, height;
    uint32_t tone, transfer, layout;
    float exposure;   // (before the scale)
    float white2;     // white * white
};

RT_HD uint32_t bits_of(float x) { return rtm::f2u(x); }
RT_HD float float_of(uint32_t u) { return rtm::u2f(u); }
// finite and > 0 (NaN fails the first comparison)
RT_HD bool positive_finite(float x) { return x > 0.0f && x < __builtin_huge_valf(); }

RT_HD float exposure_of(float exposure, bool have_scale, float scale) {
    return have_scale && positive_finite(scale) ? exposure * scale : exposure;
}

RT_HD float tone_input(float c, float e) {
    const float v = c * e;
    return v >= 0.0f ? (v < 0x1p64f ? v : 0x1p64f) : 0.0f;
}

RT_HD float tone(uint32_t which, float m, float white2) {
    if (which == TONE_CLAMP) return m;
    return (m * (1.0f + m / white2)) / (1.0f + m);
}

// LINEAR: NaN and everything not > 0 give 0
RT_HD uint32_t linear_byte(float t) {
    const float l = t > 0.0f ? (t < 1.0f ? t : 1.0f) : 0.0f;
    return (uint32_t)(l * 255.0f + 0.5f);
}

// SRGB: the number of thresholds <= t, through the coarse index (T: RT_SRGB_ENCODE_T_VALUES, base:
// RT_SRGB_ENCODE_BASE_VALUES, wherever the caller keeps them).  t is searched as clamp(t) -- NaN and negatives as 0, what is
// above 1 (+inf too) as 1, which changes no comparison with a threshold, all of them in (0, 1) -- so that the bucket is one
// of the table's: below 2^-13 bucket 0, which holds no threshold.
template <class TP, class BP>
RT_HD uint32_t srgb_byte(float t, TP T, BP base) {
    const float c = t >= 1.0f ? 1.0f : t > 0.0f ? t : 0.0f;
    const uint32_t q = bits_of(c) >> RT_SRGB_ENCODE_SHIFT;
    const uint32_t k = base[q < RT_SRGB_ENCODE_FIRST ? 0u : q - RT_SRGB_ENCODE_FIRST];
    uint32_t n = k;
    for (uint32_t j = 1; j <= STEPS; ++j) n += c >= T[k + j] ? 1u : 0u;
    return n;
}

template <class TP, class BP>
RT_HD uint32_t channel_byte(const Call& c, float color, float e, TP T, BP base) {
    const float t = tone(c.tone, tone_input(color, e), c.white2);
    return c.transfer == TRANSFER_SRGB ? srgb_byte(t, T, base) : linear_byte(t);
}

// The four bytes of a texel as one little-endian word, layout bit 0 applied.
template <class TP, class BP>
RT_HD uint32_t texel_word(const Call& c, const float rgba[4], float e, TP T, BP base) {
    const uint32_t r = channel_byte(c, rgba[0], e, T, base), g = channel_byte(c, rgba[1], e, T, base),
                   b = channel_byte(c, rgba[2], e, T, base), a = linear_byte(rgba[3]);
    const bool swap = (c.layout & LAYOUT_BGRA) != 0u;
    return (swap ? b : r) | (g << 8) | ((swap ? r : b) << 16) | (a << 24);
}

// The row of the output that input row y goes to.
RT_HD uint32_t out_row(const Call& c, uint32_t y) { return (c.layout & LAYOUT_TOP_FIRST) != 0u ? c.height - 1u - y : y; }

// ---- the exposure meter ----
// The bin of a texel, or -1 for one that is not counted (Y NaN, <= 0 or +inf).
RT_HD int32_t luminance_bin(float c0, float c1, float c2) {
    const float Y = rtvd::luminance(c0, c1, c2);
    if (!positive_finite(Y)) return -1;
    const int32_t b = (int32_t)(bits_of(Y) >> 20) - BIN_FIRST;
    return b < 0 ? 0 : b > 255 ? 255 : b;
}

// The once-per-call numbers of rt_auto_exposure.
struct MeterCall {
    uint32_t width, height;
    uint32_t low_permille, high_permille;
    float key, min_scale, max_scale, rate;
};

// What of bin b's rank interval [start, start + n) lies in [lo, hi).
RT_HD uint32_t kept(uint32_t start, uint32_t n, uint32_t lo, uint32_t hi) {
    const uint32_t a = start > lo ? start : lo, e = start + n < hi ? start + n : hi;
    return e > a ? e - a : 0u;
}

// The scale from the trimmed sums N' = kept_n and S = kept_sum (both exact in a double).
RT_HD float meter_scale(const MeterCall& c, uint32_t kept_n, uint64_t kept_sum, bool have_prev, float prev) {
    float target = 1.0f;
    if (kept_n != 0u) {
        const float mbar = (float)(double)kept_sum / (float)(double)kept_n;
        const float Ybar = float_of((uint32_t)((mbar + 888.5f) * 1048576.0f));
        const float q = c.key / Ybar;
        target = q > c.min_scale ? q : c.min_scale;
        target = target < c.max_scale ? target : c.max_scale;
    }
    if (have_prev && positive_finite(prev)) return prev + (target - prev) * c.rate;
    return target;
}

}  // namespace rtdp

#endif
