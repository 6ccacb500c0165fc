// host/vdenoise.cpp -- the variance-guided denoiser's definition in executable form (include/rt_abi.h:
// rt_denoise_variance_host, rt_luminance_moments_host) and the argument rules it shares with the
// device entry points.  Plain C++ over host pointers; the per-texel and per-tap arithmetic is csrc/rt_vdenoise.h, which the
// device kernels evaluate too.  Compiled with -ffp-contract=off.
#if defined(__HIPCC__)
// (the build compiles this C++ unit with hipcc as well: rt_transc.h then marks its functions __host__ __device__
// __forceinline__, which the runtime's headers define for plain C++)
#include <hip/hip_runtime_api.h>
#endif
#include <cstring>
#include <new>
#include <vector>

#include "../rt_vdenoise.h"
#include "../rt_vdenoise_api.h"
#include "plane_check.h"

namespace rt2 {

int vdenoise_check(const rt_vdenoise_desc* d, bool moments_only, bool device, bool host_memory, std::string& err) {
    auto bad = [&](int code, const char* msg) {
        err = msg;
        return code;
    };
    if (!d) return bad(RT_ERR_INVALID_ARGUMENT, "null rt_vdenoise_desc");
    if (d->struct_bytes != sizeof(rt_vdenoise_desc)) return bad(RT_ERR_INVALID_ARGUMENT, "rt_vdenoise_desc.struct_bytes is not sizeof(rt_vdenoise_desc)");
    if (d->_p0 != 0u) return bad(RT_ERR_INVALID_ARGUMENT, "rt_vdenoise_desc._p0 must be 0");
    if (d->_p1 != 0u) return bad(RT_ERR_INVALID_ARGUMENT, "rt_vdenoise_desc._p1 must be 0");
    if (d->width == 0u || d->height == 0u) return bad(RT_ERR_INVALID_ARGUMENT, "zero width or height");
    if (!moments_only) {
        if (d->iterations < 1u || d->iterations > 8u) return bad(RT_ERR_INVALID_ARGUMENT, "iterations outside 1 .. 8");
        if (!(d->sigma_luminance > 0.0f) || !(d->sigma_normal > 0.0f) || !(d->sigma_point > 0.0f))
            return bad(RT_ERR_INVALID_ARGUMENT, "a sigma is NaN or <= 0");
        if (!rtdn::is_finite(d->sigma_luminance) || !rtdn::is_finite(d->sigma_normal) || !rtdn::is_finite(d->sigma_point))
            return bad(RT_ERR_INVALID_ARGUMENT, "sigma_luminance, sigma_normal and sigma_point must be finite");
        if (!(d->min_history >= 1.0f) || !rtdn::is_finite(d->min_history))
            return bad(RT_ERR_INVALID_ARGUMENT, "min_history is NaN, infinite or below 1");
        if ((d->moments != nullptr) != (d->history != nullptr))
            return bad(RT_ERR_INVALID_ARGUMENT, "the moments and history planes go together: one is null and the other is not");
    }
    if (!d->normal || !d->point || !d->out) return bad(RT_ERR_INVALID_ARGUMENT, "null normal, point or out plane");
    if (!d->color && (!device || host_memory)) return bad(RT_ERR_INVALID_ARGUMENT, "null color plane (only device planes may name the handle's image that way)");
    if ((uint64_t)d->width * d->height > 0x7fffffffull) return bad(RT_ERR_CAPACITY, "more than 2^31 - 1 texels");
    if (device && !host_memory) {
        const PlaneAlign planes[9] = {{d->color, 15u, "color"}, {d->normal, 3u, "normal"}, {d->point, 3u, "point"},
                                      {d->albedo, 15u, "albedo"}, {d->emission, 15u, "emission"}, {d->out, 15u, "out"},
                                      {d->moments, 15u, "moments"}, {d->history, 3u, "history"}, {d->out_variance, 3u, "out_variance"}};
        return misaligned(planes, moments_only ? 6 : 9, err);
    }
    return RT_OK;
}

namespace {

struct Guide {       // what the device's prepare kernel packs per texel
    float n[3];
    float ok;        // 1: filterable
    float x[3];
    float _p;
};

float albedo_of(const rt_vdenoise_desc* d, size_t p, int c) { return d->albedo ? rtdn::albedo_floor(d->albedo[4 * p + c]) : 1.0f; }

// classifies texel p into g and demodulates its colour into c[3]
void prepare(const rt_vdenoise_desc* d, size_t p, Guide& g, float c[3]) {
    static const float no_emission[3] = {0.0f, 0.0f, 0.0f};
    for (int k = 0; k < 3; ++k) {
        g.n[k] = d->normal[3 * p + k];
        g.x[k] = d->point[3 * p + k];
    }
    g._p = 0.0f;
    g.ok = rtdn::filterable(g.n, g.x, d->color + 4 * p, d->emission ? d->emission + 4 * p : no_emission) ? 1.0f : 0.0f;
    for (int k = 0; k < 3; ++k) c[k] = d->color[4 * p + k] / albedo_of(d, p, k);
}

}  // namespace

int luminance_moments_host(const rt_vdenoise_desc* d, std::string& err) {
    if (const int rc = vdenoise_check(d, true, false, false, err); rc != RT_OK) return rc;
    const size_t texels = (size_t)d->width * d->height;
    for (size_t p = 0; p < texels; ++p) {
        // (out may be color: texel by texel, read before the write)
        Guide one;
        float c[3];
        prepare(d, p, one, c);
        float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (one.ok != 0.0f) {
            const float l = rtvd::luminance(c[0], c[1], c[2]);
            o[0] = l;
            o[1] = l * l;
        }
        std::memcpy(d->out + 4 * p, o, sizeof(o));
    }
    return RT_OK;
}

int vdenoise_host(const rt_vdenoise_desc* d, std::string& err) {
    if (const int rc = vdenoise_check(d, false, false, false, err); rc != RT_OK) return rc;
    const int W = (int)d->width, H = (int)d->height;
    const size_t texels = (size_t)W * (size_t)H;
    std::vector<Guide> guide;
    std::vector<float> ping[2];   // (c_i.rgb, var_i), four floats per texel
    std::vector<float> lum;       // l(c_i) of every texel, per pass
    try {
        guide.resize(texels);
        ping[0].resize(texels * 4);
        ping[1].resize(texels * 4);
        lum.resize(texels);
    } catch (const std::bad_alloc&) {
        err = "out of host memory";
        return RT_ERR_OUT_OF_MEMORY;
    }
    const float k_n = rtdn::k_of_sigma(d->sigma_normal), k_x = rtdn::k_of_sigma(d->sigma_point);
    auto inside = [&](long qx, long qy) { return qx >= 0 && qx < W && qy >= 0 && qy < H; };

    // classify and demodulate
    for (size_t p = 0; p < texels; ++p) {
        prepare(d, p, guide[p], &ping[0][4 * p]);
        ping[0][4 * p + 3] = 0.0f;
        lum[p] = rtvd::luminance(ping[0][4 * p], ping[0][4 * p + 1], ping[0][4 * p + 2]);
    }

    // the variance of the input
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t p = (size_t)y * W + x;
            if (guide[p].ok == 0.0f) continue;
            float v;
            if (d->moments && rtvd::temporal_serves(d->moments[4 * p], d->moments[4 * p + 1], d->history[p], d->min_history)) {
                v = rtvd::temporal_variance(d->moments[4 * p], d->moments[4 * p + 1], d->history[p]);
            } else {
                float s1 = 0.0f, s2 = 0.0f, sw = 0.0f;
                for (int dy = -3; dy <= 3; ++dy)
                    for (int dx = -3; dx <= 3; ++dx) {
                        const long qx = (long)x + dx, qy = (long)y + dy;
                        if (!inside(qx, qy)) continue;
                        const size_t q = (size_t)qy * W + (size_t)qx;
                        if (guide[q].ok == 0.0f) continue;
                        const float u = rtvd::window_weight(guide[p].n, guide[q].n, guide[p].x, guide[q].x, k_n, k_x);
                        if (!(u > 0.0f)) continue;
                        s1 += u * lum[q];
                        s2 += u * (lum[q] * lum[q]);
                        sw += u;
                    }
                v = rtvd::spatial_variance(s1, s2, sw);
            }
            ping[0][4 * p + 3] = rtvd::clamp_variance(v);
        }

    // the passes
    const int n = (int)d->iterations;
    for (int i = 0; i < n; ++i) {
        const int s = 1 << i;
        const float* src = ping[i & 1].data();
        float* dst = ping[(i + 1) & 1].data();
        if (i > 0)
            for (size_t p = 0; p < texels; ++p)
                if (guide[p].ok != 0.0f) lum[p] = rtvd::luminance(src[4 * p], src[4 * p + 1], src[4 * p + 2]);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const size_t p = (size_t)y * W + x;
                if (guide[p].ok == 0.0f) continue;
                float gs = 0.0f, gw = 0.0f;
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        const long qx = (long)x + dx, qy = (long)y + dy;
                        if (!inside(qx, qy)) continue;
                        const size_t q = (size_t)qy * W + (size_t)qx;
                        if (guide[q].ok == 0.0f) continue;
                        const float g = rtvd::kernel_g(dx) * rtvd::kernel_g(dy);
                        gs += g * src[4 * q + 3];
                        gw += g;
                    }
                const float D = rtvd::luminance_scale(d->sigma_luminance, gs / gw);
                float sum[3] = {0.0f, 0.0f, 0.0f}, vsum = 0.0f, wsum = 0.0f;
                for (int dy = -2; dy <= 2; ++dy)
                    for (int dx = -2; dx <= 2; ++dx) {
                        const long qx = (long)x + (long)s * dx, qy = (long)y + (long)s * dy;
                        if (!inside(qx, qy)) continue;
                        const size_t q = (size_t)qy * W + (size_t)qx;
                        if (guide[q].ok == 0.0f) continue;
                        const float w = rtvd::tap_weight(rtdn::kernel_h(dx) * rtdn::kernel_h(dy), lum[p], lum[q], D, guide[p].n, guide[q].n,
                                                         guide[p].x, guide[q].x, k_n, k_x);
                        if (!(w > 0.0f)) continue;
                        for (int c = 0; c < 3; ++c) sum[c] += w * src[4 * q + c];
                        vsum += (w * w) * src[4 * q + 3];
                        wsum += w;
                    }
                for (int c = 0; c < 3; ++c) dst[4 * p + c] = sum[c] / wsum;
                dst[4 * p + 3] = vsum / (wsum * wsum);
            }
    }

    // remodulate; every other texel is copied (out may be color: texel by texel, the alpha read before the write)
    const float* c_n = ping[n & 1].data();
    for (size_t p = 0; p < texels; ++p) {
        float o[4], var = 0.0f;
        if (guide[p].ok != 0.0f) {
            for (int c = 0; c < 3; ++c) o[c] = c_n[4 * p + c] * albedo_of(d, p, c);
            o[3] = d->color[4 * p + 3];
            var = c_n[4 * p + 3];
        } else {
            std::memcpy(o, d->color + 4 * p, sizeof(o));
        }
        std::memcpy(d->out + 4 * p, o, sizeof(o));
        if (d->out_variance) d->out_variance[p] = var;
    }
    return RT_OK;
}

}  // namespace rt2
