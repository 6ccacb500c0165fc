// host/denoise.cpp -- the denoiser's definition in executable form (include/rt_abi.h: rt_denoise_host; DESIGN.md section
// 2.13) and the argument rules it shares with the device entry point.  Plain C++ over host pointers; the per-texel and
// per-tap arithmetic is csrc/rt_denoise.h, which the device kernels evaluate too.  Compiled with -ffp-contract=off.
#if defined(__HIPCC__)
// (the build compiles this C++ unit with hipcc as well: rt_transc.h then marks its functions __host__ __device__
// __forceinline__, which the runtime's headers define for plain C++)
#include <hip/hip_runtime_api.h>
#endif
#include <cstring>
#include <new>
#include <vector>

#include "../rt_denoise.h"
#include "../rt_denoise_api.h"
#include "plane_check.h"

namespace rt2 {

int denoise_check(const rt_denoise_desc* d, bool device, bool host_memory, std::string& err) {
    auto bad = [&](int code, const char* msg) {
        err = msg;
        return code;
    };
    if (!d) return bad(RT_ERR_INVALID_ARGUMENT, "null rt_denoise_desc");
    if (d->struct_bytes != sizeof(rt_denoise_desc)) return bad(RT_ERR_INVALID_ARGUMENT, "rt_denoise_desc.struct_bytes is not sizeof(rt_denoise_desc)");
    if (d->_p0 != 0u) return bad(RT_ERR_INVALID_ARGUMENT, "rt_denoise_desc._p0 must be 0");
    if (d->width == 0u || d->height == 0u) return bad(RT_ERR_INVALID_ARGUMENT, "zero width or height");
    if (d->iterations < 1u || d->iterations > 8u) return bad(RT_ERR_INVALID_ARGUMENT, "iterations outside 1 .. 8");
    if (!(d->sigma_color > 0.0f) || !(d->sigma_normal > 0.0f) || !(d->sigma_point > 0.0f))
        return bad(RT_ERR_INVALID_ARGUMENT, "a sigma is NaN or <= 0");
    if (!rtdn::is_finite(d->sigma_normal) || !rtdn::is_finite(d->sigma_point))
        return bad(RT_ERR_INVALID_ARGUMENT, "sigma_normal and sigma_point must be finite");
    if (!d->normal || !d->point || !d->out) return bad(RT_ERR_INVALID_ARGUMENT, "null normal, point or out plane");
    if (!d->color && (!device || host_memory)) return bad(RT_ERR_INVALID_ARGUMENT, "null color plane (only device planes may name the handle's image that way)");
    if ((uint64_t)d->width * d->height > 0x7fffffffull) return bad(RT_ERR_CAPACITY, "more than 2^31 - 1 texels");
    if (device && !host_memory) {
        const PlaneAlign planes[6] = {{d->color, 15u, "color"}, {d->normal, 3u, "normal"}, {d->point, 3u, "point"},
                                      {d->albedo, 15u, "albedo"}, {d->emission, 15u, "emission"}, {d->out, 15u, "out"}};
        return misaligned(planes, 6, err);
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

}  // namespace

int denoise_host(const rt_denoise_desc* d, std::string& err) {
    if (const int rc = denoise_check(d, false, false, err); rc != RT_OK) return rc;
    const int W = (int)d->width, H = (int)d->height;
    const size_t texels = (size_t)W * (size_t)H;
    std::vector<Guide> guide;
    std::vector<float> ping[2];   // c_i, three floats per texel
    try {
        guide.resize(texels);
        ping[0].resize(texels * 3);
        ping[1].resize(texels * 3);
    } catch (const std::bad_alloc&) {
        err = "out of host memory";
        return RT_ERR_OUT_OF_MEMORY;
    }
    const float k_c = rtdn::k_of_sigma(d->sigma_color), k_n = rtdn::k_of_sigma(d->sigma_normal), k_x = rtdn::k_of_sigma(d->sigma_point);
    auto albedo_of = [&](size_t p, int c) { return d->albedo ? rtdn::albedo_floor(d->albedo[4 * p + c]) : 1.0f; };

    // classify and demodulate
    static const float no_emission[3] = {0.0f, 0.0f, 0.0f};
    for (size_t p = 0; p < texels; ++p) {
        Guide& g = guide[p];
        for (int c = 0; c < 3; ++c) {
            g.n[c] = d->normal[3 * p + c];
            g.x[c] = d->point[3 * p + c];
        }
        g._p = 0.0f;
        g.ok = rtdn::filterable(g.n, g.x, d->color + 4 * p, d->emission ? d->emission + 4 * p : no_emission) ? 1.0f : 0.0f;
        for (int c = 0; c < 3; ++c) ping[0][3 * p + c] = d->color[4 * p + c] / albedo_of(p, c);
    }

    // the passes
    const int n = (int)d->iterations;
    for (int i = 0; i < n; ++i) {
        const int s = 1 << i;
        const float k_ci = rtdn::k_c_of_pass(k_c, i);
        const float* src = ping[i & 1].data();
        float* dst = ping[(i + 1) & 1].data();
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const size_t p = (size_t)y * W + x;
                if (guide[p].ok == 0.0f) continue;
                float sum[3] = {0.0f, 0.0f, 0.0f}, wsum = 0.0f;
                for (int dy = -2; dy <= 2; ++dy)
                    for (int dx = -2; dx <= 2; ++dx) {
                        const long qx = (long)x + (long)s * dx, qy = (long)y + (long)s * dy;
                        if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                        const size_t q = (size_t)qy * W + (size_t)qx;
                        if (guide[q].ok == 0.0f) continue;
                        const float w = rtdn::tap_weight(rtdn::kernel_h(dx) * rtdn::kernel_h(dy), src + 3 * p, src + 3 * q, guide[p].n,
                                                         guide[q].n, guide[p].x, guide[q].x, k_ci, k_n, k_x);
                        if (!(w > 0.0f)) continue;
                        for (int c = 0; c < 3; ++c) sum[c] += w * src[3 * q + c];
                        wsum += w;
                    }
                for (int c = 0; c < 3; ++c) dst[3 * p + c] = sum[c] / wsum;
            }
    }

    // remodulate; every other texel is copied (out may be color: texel by texel, the alpha read before the write)
    const float* c_n = ping[n & 1].data();
    for (size_t p = 0; p < texels; ++p) {
        float o[4];
        if (guide[p].ok != 0.0f) {
            for (int c = 0; c < 3; ++c) o[c] = c_n[3 * p + c] * albedo_of(p, c);
            o[3] = d->color[4 * p + 3];
        } else {
            std::memcpy(o, d->color + 4 * p, sizeof(o));
        }
        std::memcpy(d->out + 4 * p, o, sizeof(o));
    }
    return RT_OK;
}

}  // namespace rt2
