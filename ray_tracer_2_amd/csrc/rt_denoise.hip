// rt_denoise.hip -- the device kernels of the G-buffer-guided a-trous denoiser (include/rt_abi.h: rt_denoise; DESIGN.md
// section 2.13).
//
//   prepare -- one lane per texel: classifies the texel (rtdn::filterable), packs (normal.xyz, filterable) and
//              (point.xyz, 0) into two float4 of the guide record, and writes the demodulated colour c_0 as a float4;
//              from here on every tap of every pass is three 16-byte loads.
//   pass i  -- one lane per texel, a workgroup per tile of 32 x 8 texels (a wave: 32 x 2): the 25 taps in the defined
//              order, dy outer and dx inner, a row of five at a time -- the row's loads first, then its weights.  Steps
//              1 and 2 read them from an LDS copy of the tile and its halo, larger steps straight from global memory --
//              each step has the form that was faster at 1920 x 1080; the forms share the
//              tap's code and agree bit for bit.  The last pass remodulates and writes `out` with streaming stores;
//              there a texel that is not filterable copies its colour through.
// The per-tap arithmetic is csrc/rt_denoise.h, shared with the host restatement (host/denoise.cpp); this file is compiled
// with -ffp-contract=off, so the result is the host's bit for bit.
//
// Bounds: a lane outside the frame takes part in filling the LDS tile (from texels inside the frame only) and leaves
// before any access of its own; a tap outside the frame reads the lane's own texel instead (direct form) or an LDS slot
// filled as "not filterable" (tiled form: every tap lies inside the halo) and adds nothing; texel indices are < 2^31 (the
// entry point checks), the guide index 2 p + 1 < 2^32, and every address is formed in 64 bits.
#include <hip/hip_runtime.h>

#include "rt_denoise.h"
#include "rt_denoise_api.h"

namespace rtd {
namespace {

constexpr uint32_t TILE_W = 32, TILE_H = 8, DENOISE_THREADS = TILE_W * TILE_H;

typedef float v4f __attribute__((ext_vector_type(4)));
#define RT_GLOBAL(T, p) ((__attribute__((address_space(1))) T*)(void*)(p))

// written once and read by nobody in the launch (the G-buffer kernel's streaming stores)
__device__ __forceinline__ void store_out(float* out, size_t p, float4 v) {
    __builtin_nontemporal_store(v4f{v.x, v.y, v.z, v.w}, RT_GLOBAL(v4f, reinterpret_cast<float4*>(out) + p));
}

__global__ void __launch_bounds__(DENOISE_THREADS) rt_denoise_prepare_kernel(const DenoiseArgs a) {
    const size_t p = (size_t)blockIdx.x * DENOISE_THREADS + threadIdx.x;
    if (p >= (size_t)a.width * a.height) return;
    const float4 c = reinterpret_cast<const float4*>(a.color)[p];
    const float n[3] = {a.normal[3 * p], a.normal[3 * p + 1], a.normal[3 * p + 2]};
    const float x[3] = {a.point[3 * p], a.point[3 * p + 1], a.point[3 * p + 2]};
    const float col[3] = {c.x, c.y, c.z};
    float4 e = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (a.emission) e = reinterpret_cast<const float4*>(a.emission)[p];
    const float em[3] = {e.x, e.y, e.z};
    const bool ok = rtdn::filterable(n, x, col, em);
    float4 al = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    if (a.albedo) {
        const float4 v = reinterpret_cast<const float4*>(a.albedo)[p];
        al = make_float4(rtdn::albedo_floor(v.x), rtdn::albedo_floor(v.y), rtdn::albedo_floor(v.z), 1.0f);
    }
    float4* guide = static_cast<float4*>(a.guide);
    guide[2 * p] = make_float4(n[0], n[1], n[2], ok ? 1.0f : 0.0f);
    guide[2 * p + 1] = make_float4(x[0], x[1], x[2], 0.0f);
    static_cast<float4*>(a.ping[0])[p] = make_float4(c.x / al.x, c.y / al.y, c.z / al.z, 0.0f);
}

// One tap's texel as the passes hold it: (normal.xyz, filterable flag), (point.xyz, colour.x), (colour.y, colour.z) -- ten
// live words in 16 + 16 + 8 bytes, which is how the tiled form lays them out in LDS.
struct Tap {
    float4 n, xc;
    float2 c;
    bool in;
};

// What a texel gathers over its taps.  A tap that the definition skips adds +0, which leaves sum and wsum (never -0: they
// start at +0) as they are, bit for bit: what a tap adds is selected after its weight.
struct Gather {
    float np[3], xp[3], cp[3];
    float k_ci, k_n, k_x;
    float sum[3] = {0.0f, 0.0f, 0.0f}, wsum = 0.0f;
    __device__ __forceinline__ void tap(int dx, int dy, const Tap& t) {
        const float nq[3] = {t.n.x, t.n.y, t.n.z}, xq[3] = {t.xc.x, t.xc.y, t.xc.z}, cq[3] = {t.xc.w, t.c.x, t.c.y};
        const float w = rtdn::tap_weight(rtdn::kernel_h(dx) * rtdn::kernel_h(dy), cp, cq, np, nq, xp, xq, k_ci, k_n, k_x);
        const bool take = t.in && t.n.w != 0.0f && w > 0.0f;
        sum[0] += take ? w * cq[0] : 0.0f;
        sum[1] += take ? w * cq[1] : 0.0f;
        sum[2] += take ? w * cq[2] : 0.0f;
        wsum += take ? w : 0.0f;
    }
};

// One pass.  src: c_i; dst: c_{i+1} (unused by the last pass, which writes a.out).
// The exponential's range checks are branches (rtm::exp_ and scale2 return early), and the compiler moves no load across
// them.  So the taps are taken a ROW of five at a time: the row's loads -- 15 global loads, or 15 LDS reads -- are issued
// together, then its five weights are evaluated (measured against one tap at a time, a row ahead, and all rows unrolled:
// DESIGN.md section 2.13).
// LDS_STEP == 0, the direct form, for any step: every tap loads from an address inside the frame -- its own texel q, or p in
// place of a q outside -- so that no branch stands between the loads of a row either.
// LDS_STEP == s > 0 (1 and 2 are instantiated), the tiled form for step s: the workgroup first copies its tile and a halo of 2 s texels on every side,
// (32 + 4 s) x (8 + 4 s) texels, into LDS as the three planes of Tap (40 bytes per texel; 16-byte global loads, two
// ds_write_b128 and a ds_write_b64), texels outside the frame as "not filterable"; a tap is two ds_read_b128 and a
// ds_read_b64 with every component live.  The lanes one LDS cycle serves lie in one tile row and read consecutive
// elements: no two of them share a bank.
template <bool LAST, int LDS_STEP>
__global__ void __launch_bounds__(DENOISE_THREADS) rt_denoise_pass_kernel(const DenoiseArgs a, const int step, const float k_ci, const float k_n, const float k_x,
                                                                          const float4* __restrict__ src, float4* __restrict__ dst) {
    constexpr uint32_t S = (uint32_t)LDS_STEP, RW = TILE_W + 4 * S, RH = TILE_H + 4 * S, R = RW * RH;
    __shared__ float4 tile_n[LDS_STEP ? R : 1], tile_xc[LDS_STEP ? R : 1];
    __shared__ float2 tile_c[LDS_STEP ? R : 1];
    const uint32_t tiles_x = (a.width + TILE_W - 1) / TILE_W;
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const uint32_t lx = threadIdx.x & (TILE_W - 1), ly = threadIdx.x / TILE_W;
    const uint32_t x = tx * TILE_W + lx, y = ty * TILE_H + ly;   // (< 2^31 + 32)
    const float4* guide = static_cast<const float4*>(a.guide);
    if constexpr (LDS_STEP != 0) {
        for (uint32_t r = threadIdx.x; r < R; r += DENOISE_THREADS) {
            const uint32_t ry = r / RW, rx = r - ry * RW;
            // (unsigned: left of column 0 or below row 0 wraps to at least 2^32 - 2 s and fails the comparison)
            const uint32_t gx = tx * TILE_W + rx - 2 * S, gy = ty * TILE_H + ry - 2 * S;
            float4 qn = make_float4(0.0f, 0.0f, 0.0f, 0.0f), qg = qn, qc = qn;
            if (gx < a.width && gy < a.height) {
                const size_t q = (size_t)gy * a.width + (size_t)gx;
                qn = guide[2 * q];
                qg = guide[2 * q + 1];
                qc = src[q];
            }
            tile_n[r] = qn;
            tile_xc[r] = make_float4(qg.x, qg.y, qg.z, qc.x);
            tile_c[r] = make_float2(qc.y, qc.z);
        }
        __syncthreads();
    }
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * a.width + (size_t)x;
    const uint32_t centre = (ly + 2 * S) * RW + lx + 2 * S;   // (the tiled form: this texel in the LDS planes)
    const float4 gn = LDS_STEP ? tile_n[centre] : guide[2 * p];
    if (gn.w == 0.0f) {
        if (LAST) store_out(a.out, p, reinterpret_cast<const float4*>(a.color)[p]);
        return;
    }
    // the five taps of row dy: loads only
    auto load_row = [&](int dy, Tap (&t)[5]) {
        // (unsigned: y < 2^31 and |step * dy| <= 256, so a row above the frame stays below 2^32 and one below row 0 wraps
        // to at least 2^32 - 256: both fail the one comparison; the columns likewise)
        const uint32_t qy = y + (uint32_t)(step * dy);
        const bool in_y = qy < a.height;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            if constexpr (LDS_STEP != 0) {
                const uint32_t i = (uint32_t)((int)centre + LDS_STEP * dy * (int)RW + LDS_STEP * dx);   // (inside the halo)
                t[dx + 2] = Tap{tile_n[i], tile_xc[i], tile_c[i], true};
            } else {
                const uint32_t qx = x + (uint32_t)(step * dx);
                const bool in = in_y && qx < a.width;
                const size_t q = in ? (size_t)qy * a.width + (size_t)qx : p;
                const float4 qg = guide[2 * q + 1], qc = src[q];
                t[dx + 2] = Tap{guide[2 * q], make_float4(qg.x, qg.y, qg.z, qc.x), make_float2(qc.y, qc.z), in};
            }
        }
    };
    Tap cur[5];
    load_row(-2, cur);
    Gather g;
    {
        // this texel's own values
        float4 gx, cc;
        if constexpr (LDS_STEP != 0) {
            const float4 xc = tile_xc[centre];
            const float2 c2 = tile_c[centre];
            gx = make_float4(xc.x, xc.y, xc.z, 0.0f);
            cc = make_float4(xc.w, c2.x, c2.y, 0.0f);
        } else {
            gx = guide[2 * p + 1];
            cc = src[p];
        }
        g = Gather{{gn.x, gn.y, gn.z}, {gx.x, gx.y, gx.z}, {cc.x, cc.y, cc.z}, k_ci, k_n, k_x};
    }
    // The loop over the rows stays a loop: unrolled, the compiler issued the loads of all five rows first (254 VGPRs in the
    // tiled form, 2 waves per SIMD) and ran slower; as a loop a pass holds one row (95 - 127 VGPRs, 4 - 5 waves).  The next
    // row's loads are issued at the end of an iteration, behind this row's arithmetic.
#pragma unroll 1
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) g.tap(dx, dy, cur[dx + 2]);
        if (dy < 2) load_row(dy + 1, cur);
    }
    const float4 c = make_float4(g.sum[0] / g.wsum, g.sum[1] / g.wsum, g.sum[2] / g.wsum, 0.0f);
    if (!LAST) {
        dst[p] = c;
        return;
    }
    float4 al = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    if (a.albedo) {
        const float4 v = reinterpret_cast<const float4*>(a.albedo)[p];
        al = make_float4(rtdn::albedo_floor(v.x), rtdn::albedo_floor(v.y), rtdn::albedo_floor(v.z), 1.0f);
    }
    const float alpha = a.color[4 * p + 3];
    store_out(a.out, p, make_float4(c.x * al.x, c.y * al.y, c.z * al.z, alpha));
}

template <int LDS_STEP>
void launch_pass(bool last, uint32_t tiles, hipStream_t stream, const DenoiseArgs& a, int step, float k_ci, float k_n, float k_x,
                 const float4* src, float4* dst) {
    if (last)
        hipLaunchKernelGGL((rt_denoise_pass_kernel<true, LDS_STEP>), dim3(tiles), dim3(DENOISE_THREADS), 0, stream, a, step, k_ci, k_n, k_x, src, dst);
    else
        hipLaunchKernelGGL((rt_denoise_pass_kernel<false, LDS_STEP>), dim3(tiles), dim3(DENOISE_THREADS), 0, stream, a, step, k_ci, k_n, k_x, src, dst);
}

}  // namespace

// prepare, then a.iterations passes over the two colour images; the last one writes a.out.
hipError_t launch_denoise(const DenoiseArgs& a, hipStream_t stream) {
    const size_t texels = (size_t)a.width * a.height;
    const float k_c = rtdn::k_of_sigma(a.sigma_color), k_n = rtdn::k_of_sigma(a.sigma_normal), k_x = rtdn::k_of_sigma(a.sigma_point);
    const uint32_t tiles = ((a.width + TILE_W - 1) / TILE_W) * ((a.height + TILE_H - 1) / TILE_H);   // (<= 2^31 / 8 + ...: fits)
    hipLaunchKernelGGL(rt_denoise_prepare_kernel, dim3((uint32_t)((texels + DENOISE_THREADS - 1) / DENOISE_THREADS)), dim3(DENOISE_THREADS),
                       0, stream, a);
    for (int i = 0; i < a.iterations; ++i) {
        const float4* src = static_cast<const float4*>(a.ping[i & 1]);
        float4* dst = static_cast<float4*>(a.ping[(i + 1) & 1]);
        const float k_ci = rtdn::k_c_of_pass(k_c, i);
        const bool last = i + 1 == a.iterations;
        const int step = 1 << i;
        // steps 1 and 2 tiled, every larger step direct: measured (profiles/denoise_bench.txt)
        if (step == 1) launch_pass<1>(last, tiles, stream, a, step, k_ci, k_n, k_x, src, dst);
        else if (step == 2) launch_pass<2>(last, tiles, stream, a, step, k_ci, k_n, k_x, src, dst);
        else launch_pass<0>(last, tiles, stream, a, step, k_ci, k_n, k_x, src, dst);
    }
    return hipGetLastError();
}

}  // namespace rtd
