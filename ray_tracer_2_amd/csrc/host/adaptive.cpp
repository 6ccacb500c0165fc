// host/adaptive.cpp -- adaptive sampling's definitions in executable form (include/rt_abi.h: rt_adaptive_plan_host,
// rt_adaptive_merge_host) and the argument rules they share with the device entry points.  Plain
// C++ over host pointers, no working memory; the per-texel rules are csrc/rt_adaptive.h, which the device kernels evaluate
// too.  Compiled with -ffp-contract=off.
#if defined(__HIPCC__)
// (the build compiles this C++ unit with hipcc as well: rt_transc.h then marks its functions __host__ __device__
// __forceinline__, which the runtime's headers define for plain C++)
#include <hip/hip_runtime_api.h>
#endif
#include <cstring>

#include "../rt_adaptive.h"
#include "../rt_adaptive_api.h"
#include "plane_check.h"

namespace rt2 {

int adaptive_plan_check(const rt_adaptive_plan_desc* d, bool device, bool host_memory, std::string& err) {
    auto bad = [&](int code, const char* msg) {
        err = msg;
        return code;
    };
    if (!d) return bad(RT_ERR_INVALID_ARGUMENT, "null rt_adaptive_plan_desc");
    if (d->struct_bytes != sizeof(rt_adaptive_plan_desc)) return bad(RT_ERR_INVALID_ARGUMENT, "rt_adaptive_plan_desc.struct_bytes is not sizeof(rt_adaptive_plan_desc)");
    if (d->_p0 != 0u) return bad(RT_ERR_INVALID_ARGUMENT, "rt_adaptive_plan_desc._p0 must be 0");
    if (d->_p1 != 0u) return bad(RT_ERR_INVALID_ARGUMENT, "rt_adaptive_plan_desc._p1 must be 0");
    if (d->width == 0u || d->height == 0u) return bad(RT_ERR_INVALID_ARGUMENT, "zero width or height");
    if (d->budget == 0u || d->budget > 0x7fffffffu) return bad(RT_ERR_INVALID_ARGUMENT, "budget outside 1 .. 2^31 - 1");
    if (d->max_samples == 0u || d->max_samples > 65535u) return bad(RT_ERR_INVALID_ARGUMENT, "max_samples outside 1 .. 65535");
    if (d->min_samples > d->max_samples) return bad(RT_ERR_INVALID_ARGUMENT, "min_samples is larger than max_samples");
    if (!d->variance || !d->dir || !d->counts || !d->offsets || !d->rays || !d->totals)
        return bad(RT_ERR_INVALID_ARGUMENT, "null variance, dir, counts, offsets, rays or totals");
    const uint64_t texels = (uint64_t)d->width * d->height;
    if (texels > 0x7fffffffull) return bad(RT_ERR_CAPACITY, "more than 2^31 - 1 texels");
    if ((uint64_t)d->min_samples * texels > (uint64_t)d->budget)
        return bad(RT_ERR_INVALID_ARGUMENT, "min_samples * width * height is larger than the budget");
    if (device && !host_memory) {
        const PlaneAlign planes[6] = {{d->variance, 3u, "variance"}, {d->dir, 3u, "dir"}, {d->counts, 3u, "counts"},
                                      {d->offsets, 3u, "offsets"}, {d->rays, 15u, "rays"}, {d->totals, 3u, "totals"}};
        return misaligned(planes, 6, err);
    }
    return RT_OK;
}

int adaptive_merge_check(const rt_adaptive_merge_desc* d, bool device, bool host_memory, std::string& err) {
    auto bad = [&](int code, const char* msg) {
        err = msg;
        return code;
    };
    if (!d) return bad(RT_ERR_INVALID_ARGUMENT, "null rt_adaptive_merge_desc");
    if (d->struct_bytes != sizeof(rt_adaptive_merge_desc)) return bad(RT_ERR_INVALID_ARGUMENT, "rt_adaptive_merge_desc.struct_bytes is not sizeof(rt_adaptive_merge_desc)");
    if (d->_p0 != 0u) return bad(RT_ERR_INVALID_ARGUMENT, "rt_adaptive_merge_desc._p0 must be 0");
    if (d->width == 0u || d->height == 0u) return bad(RT_ERR_INVALID_ARGUMENT, "zero width or height");
    if (d->budget == 0u || d->budget > 0x7fffffffu) return bad(RT_ERR_INVALID_ARGUMENT, "budget outside 1 .. 2^31 - 1");
    if (!(d->max_history >= 1.0f)) return bad(RT_ERR_INVALID_ARGUMENT, "max_history is NaN or below 1");
    if (!d->radiance || !d->counts || !d->offsets || !d->history || !d->out || !d->out_history)
        return bad(RT_ERR_INVALID_ARGUMENT, "null radiance, counts, offsets, history, out or out_history");
    if (!d->color && (!device || host_memory)) return bad(RT_ERR_INVALID_ARGUMENT, "null color plane (only device planes may name the handle's image that way)");
    if ((d->moments != nullptr) != (d->out_moments != nullptr))
        return bad(RT_ERR_INVALID_ARGUMENT, "the moments and out_moments planes go together: one is null and the other is not");
    if ((uint64_t)d->width * d->height > 0x7fffffffull) return bad(RT_ERR_CAPACITY, "more than 2^31 - 1 texels");
    if (device && !host_memory) {
        const PlaneAlign planes[10] = {{d->radiance, 15u, "radiance"}, {d->counts, 3u, "counts"}, {d->offsets, 3u, "offsets"},
                                       {d->color, 15u, "color"}, {d->history, 3u, "history"}, {d->albedo, 15u, "albedo"},
                                       {d->moments, 15u, "moments"}, {d->out, 15u, "out"}, {d->out_history, 3u, "out_history"},
                                       {d->out_moments, 15u, "out_moments"}};
        return misaligned(planes, 10, err);
    }
    return RT_OK;
}

int adaptive_plan_host(const rt_adaptive_plan_desc* d, std::string& err) {
    if (const int rc = adaptive_plan_check(d, false, false, err); rc != RT_OK) return rc;
    const size_t texels = (size_t)d->width * d->height;
    // the maximum, then S
    uint32_t max_key = 0u;
    for (size_t p = 0; p < texels; ++p) {
        const uint32_t k = rtad::variance_key(d->variance[p]);
        max_key = k > max_key ? k : max_key;
    }
    uint64_t S = 0u;
    for (size_t p = 0; p < texels; ++p) S += rtad::quantise(d->variance[p], max_key);
    const uint64_t R = (uint64_t)d->budget - (uint64_t)d->min_samples * texels;
    // the scan: C and F(C) carried from texel to texel
    uint64_t C = 0u, f_begin = 0u;
    uint32_t offset = 0u, above = 0u, clamped = 0u;
    for (size_t p = 0; p < texels; ++p) {
        const uint32_t q = rtad::quantise(d->variance[p], max_key);
        C += q;
        const uint64_t f_end = (S != 0u && q != 0u) ? rtad::mul_div_floor(C, R, S) : f_begin;
        bool over;
        const uint32_t n = rtad::samples_of(f_begin, f_end, d->min_samples, d->max_samples, over);
        f_begin = f_end;
        d->counts[p] = n;
        d->offsets[p] = offset;
        above += n > d->min_samples ? 1u : 0u;
        clamped += over ? 1u : 0u;
        for (uint32_t k = 0; k < n; ++k) {
            rt_path_ray r;
            std::memcpy(r.origin, d->origin, sizeof(r.origin));
            r.seed = rtad::sample_seed((uint32_t)p, d->first_frame, k);
            std::memcpy(r.dir, d->dir + 3 * p, sizeof(r.dir));
            r._p0 = 0u;
            std::memcpy(d->rays + offset + k, &r, sizeof(r));
        }
        offset += n;   // (<= budget: the e(p) sum to at most R)
    }
    if (offset < d->budget) std::memset(d->rays + offset, 0, (size_t)(d->budget - offset) * sizeof(rt_path_ray));
    d->totals[0] = offset;
    d->totals[1] = above;
    d->totals[2] = clamped;
    d->totals[3] = 0u;
    return RT_OK;
}

int adaptive_merge_host(const rt_adaptive_merge_desc* d, std::string& err) {
    if (const int rc = adaptive_merge_check(d, false, false, err); rc != RT_OK) return rc;
    const size_t texels = (size_t)d->width * d->height;
    static const float no_moments[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (size_t p = 0; p < texels; ++p) {
        // (the outputs may be the inputs: texel by texel, read before the write)
        float al[3] = {1.0f, 1.0f, 1.0f};
        if (d->albedo)
            for (int k = 0; k < 3; ++k) al[k] = rtdn::albedo_floor(d->albedo[4 * p + k]);
        rtad::Merge t;
        t.start(d->color + 4 * p, d->history[p], d->moments ? d->moments + 4 * p : no_moments);
        const uint32_t n = d->counts[p];
        const uint64_t first = d->offsets[p];
        for (uint32_t k = 0; k < n && first + k < (uint64_t)d->budget; ++k)
            t.sample(d->radiance + 4 * (first + k), al, d->max_history, d->moments != nullptr);
        std::memcpy(d->out + 4 * p, t.acc, sizeof(t.acc));
        d->out_history[p] = t.hl;
        if (d->out_moments) std::memcpy(d->out_moments + 4 * p, t.m, sizeof(t.m));
    }
    return RT_OK;
}

}  // namespace rt2
