// host/display.cpp -- the display pass's and the exposure meter's definitions in executable form (include/rt_abi.h:
// rt_display_host, rt_auto_exposure_host), the argument rules and the once-per-call numbers they
// share with the device entry points.  Plain C++ over host pointers; the per-texel arithmetic is csrc/rt_display.h, which
// the device kernels evaluate too.  Compiled with -ffp-contract=off.
#if defined(__HIPCC__)
// (the build compiles this C++ unit with hipcc as well: rt_display.h then marks its functions __host__ __device__
// __forceinline__, which the runtime's headers define for plain C++)
#include <hip/hip_runtime_api.h>
#endif
#include <cstring>

#include "../rt_display_api.h"
#include "plane_check.h"

namespace rt2 {

namespace {
const float ENCODE_T[rtdp::T_COUNT] = {RT_SRGB_ENCODE_T_VALUES};
const uint8_t ENCODE_BASE[rtdp::BUCKETS] = {RT_SRGB_ENCODE_BASE_VALUES};
}  // namespace

int display_check(const rt_display_desc* d, DisplayPath path, std::string& err) {
    auto bad = [&](int code, const char* msg) {
        err = msg;
        return code;
    };
    if (!d) return bad(RT_ERR_INVALID_ARGUMENT, "null rt_display_desc");
    if (d->struct_bytes != sizeof(rt_display_desc)) return bad(RT_ERR_INVALID_ARGUMENT, "rt_display_desc.struct_bytes is not sizeof(rt_display_desc)");
    if (d->_p0 != 0u || d->_p1 != 0u) return bad(RT_ERR_INVALID_ARGUMENT, "rt_display_desc._p0 and _p1 must be 0");
    if (d->width == 0u || d->height == 0u) return bad(RT_ERR_INVALID_ARGUMENT, "zero width or height");
    if (d->tone > RT_DISPLAY_TONE_REINHARD) return bad(RT_ERR_INVALID_ARGUMENT, "unknown tone");
    if (d->transfer > RT_DISPLAY_LINEAR) return bad(RT_ERR_INVALID_ARGUMENT, "unknown transfer");
    if (d->layout & ~(uint32_t)(RT_DISPLAY_LAYOUT_BGRA | RT_DISPLAY_LAYOUT_TOP_FIRST)) return bad(RT_ERR_INVALID_ARGUMENT, "unknown layout bits");
    if (!rtdp::positive_finite(d->exposure)) return bad(RT_ERR_INVALID_ARGUMENT, "exposure is NaN, <= 0 or infinite");
    if (d->tone == RT_DISPLAY_TONE_REINHARD && !(d->white > 0.0f)) return bad(RT_ERR_INVALID_ARGUMENT, "white is NaN or <= 0");
    if (path == DisplayPath::SNAPSHOT) {
        if (d->color || d->out) return bad(RT_ERR_INVALID_ARGUMENT, "rt_snapshot_display takes the image and writes its own buffer: color and out must be NULL");
    } else {
        if (!d->out) return bad(RT_ERR_INVALID_ARGUMENT, "null out plane");
        if (!d->color && path != DisplayPath::DEVICE)
            return bad(RT_ERR_INVALID_ARGUMENT, "null color plane (only device planes may name the handle's image that way)");
    }
    if ((uint64_t)d->width * d->height > 0x7fffffffull) return bad(RT_ERR_CAPACITY, "more than 2^31 - 1 texels");
    if (path == DisplayPath::DEVICE || path == DisplayPath::SNAPSHOT) {
        const PlaneAlign planes[3] = {{d->color, 15u, "color"}, {d->exposure_scale, 3u, "exposure_scale"}, {d->out, 3u, "out"}};
        return misaligned(planes, 3, err);
    }
    return RT_OK;
}

rtdp::Call display_call(const rt_display_desc& d) {
    rtdp::Call c{};
    c.width = d.width;
    c.height = d.height;
    c.tone = d.tone;
    c.transfer = d.transfer;
    c.layout = d.layout;
    c.exposure = d.exposure;
    c.white2 = d.tone == RT_DISPLAY_TONE_REINHARD ? d.white * d.white : 1.0f;
    return c;
}

int display_host(const rt_display_desc* d, std::string& err) {
    if (const int rc = display_check(d, DisplayPath::HOST, err); rc != RT_OK) return rc;
    const rtdp::Call c = display_call(*d);
    const float e = rtdp::exposure_of(c.exposure, d->exposure_scale != nullptr, d->exposure_scale ? *d->exposure_scale : 1.0f);
    const size_t W = d->width, H = d->height;
    for (size_t y = 0; y < H; ++y) {
        uint8_t* row = d->out + 4u * W * (size_t)rtdp::out_row(c, (uint32_t)y);
        for (size_t x = 0; x < W; ++x) {
            float rgba[4];
            std::memcpy(rgba, d->color + 4u * (y * W + x), sizeof(rgba));
            const uint32_t word = rtdp::texel_word(c, rgba, e, ENCODE_T, ENCODE_BASE);
            for (int k = 0; k < 4; ++k) row[4u * x + k] = (uint8_t)(word >> (8 * k));
        }
    }
    return RT_OK;
}

int auto_exposure_check(const rt_auto_exposure_desc* d, bool device, bool host_memory, std::string& err) {
    auto bad = [&](int code, const char* msg) {
        err = msg;
        return code;
    };
    if (!d) return bad(RT_ERR_INVALID_ARGUMENT, "null rt_auto_exposure_desc");
    if (d->struct_bytes != sizeof(rt_auto_exposure_desc))
        return bad(RT_ERR_INVALID_ARGUMENT, "rt_auto_exposure_desc.struct_bytes is not sizeof(rt_auto_exposure_desc)");
    if (d->_p0 != 0u) return bad(RT_ERR_INVALID_ARGUMENT, "rt_auto_exposure_desc._p0 must be 0");
    if (d->width == 0u || d->height == 0u) return bad(RT_ERR_INVALID_ARGUMENT, "zero width or height");
    if (!(d->low_permille < d->high_permille && d->high_permille <= 1000u))
        return bad(RT_ERR_INVALID_ARGUMENT, "low_permille and high_permille must be 0 <= low < high <= 1000");
    if (!rtdp::positive_finite(d->key)) return bad(RT_ERR_INVALID_ARGUMENT, "key is NaN, <= 0 or infinite");
    if (!rtdp::positive_finite(d->min_scale) || !rtdp::positive_finite(d->max_scale) || !(d->min_scale <= d->max_scale))
        return bad(RT_ERR_INVALID_ARGUMENT, "min_scale and max_scale must be finite with 0 < min_scale <= max_scale");
    if (!(d->rate > 0.0f && d->rate <= 1.0f)) return bad(RT_ERR_INVALID_ARGUMENT, "rate is NaN or outside (0, 1]");
    if (!d->scale) return bad(RT_ERR_INVALID_ARGUMENT, "null scale");
    if (!d->color && (!device || host_memory))
        return bad(RT_ERR_INVALID_ARGUMENT, "null color plane (only device planes may name the handle's image that way)");
    if ((uint64_t)d->width * d->height > 0x7fffffffull) return bad(RT_ERR_CAPACITY, "more than 2^31 - 1 texels");
    if (device && !host_memory) {
        const PlaneAlign planes[4] = {{d->color, 15u, "color"}, {d->prev_scale, 3u, "prev_scale"}, {d->histogram, 3u, "histogram"}, {d->scale, 3u, "scale"}};
        return misaligned(planes, 4, err);
    }
    return RT_OK;
}

rtdp::MeterCall auto_exposure_call(const rt_auto_exposure_desc& d) {
    rtdp::MeterCall c{};
    c.width = d.width;
    c.height = d.height;
    c.low_permille = d.low_permille;
    c.high_permille = d.high_permille;
    c.key = d.key;
    c.min_scale = d.min_scale;
    c.max_scale = d.max_scale;
    c.rate = d.rate;
    return c;
}

int auto_exposure_host(const rt_auto_exposure_desc* d, std::string& err) {
    if (const int rc = auto_exposure_check(d, false, false, err); rc != RT_OK) return rc;
    const rtdp::MeterCall c = auto_exposure_call(*d);
    uint32_t n[rtdp::BINS] = {};
    const size_t texels = (size_t)d->width * d->height;
    for (size_t p = 0; p < texels; ++p) {
        const int32_t b = rtdp::luminance_bin(d->color[4 * p], d->color[4 * p + 1], d->color[4 * p + 2]);
        if (b >= 0) n[b] += 1u;
    }
    uint64_t N = 0;
    for (uint32_t b = 0; b < rtdp::BINS; ++b) N += n[b];
    const uint32_t lo = (uint32_t)(N * c.low_permille / 1000u), hi = (uint32_t)(N * c.high_permille / 1000u);
    uint32_t start = 0, kept_n = 0;
    uint64_t kept_sum = 0;
    for (uint32_t b = 0; b < rtdp::BINS; ++b) {
        const uint32_t k = rtdp::kept(start, n[b], lo, hi);
        kept_n += k;
        kept_sum += (uint64_t)k * b;
        start += n[b];
    }
    const float prev = d->prev_scale ? *d->prev_scale : 0.0f;   // (read before anything is written: scale may be prev_scale)
    if (d->histogram) std::memcpy(d->histogram, n, sizeof(n));
    *d->scale = rtdp::meter_scale(c, kept_n, kept_sum, d->prev_scale != nullptr, prev);
    return RT_OK;
}

}  // namespace rt2
