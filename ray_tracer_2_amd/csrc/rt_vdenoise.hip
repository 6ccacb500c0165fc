// rt_vdenoise.hip -- the device kernels of the variance-guided a-trous denoiser (include/rt_abi.h: rt_denoise_variance,
// rt_luminance_moments).
//
//   moments  -- one lane per texel: (l, l l, 0, 0) of the demodulated colour, zeros where the texel is not filterable.
//   prepare  -- one lane per texel: classifies the texel (rtdn::filterable), packs (normal.xyz, filterable) and
//               (point.xyz, 0) into two float4 of the guide record -- rt_denoise's layout, in rt_denoise's scratch -- and
//               writes (c_0, var_0) as a float4: the variance rides in the component rt_denoise leaves 0.  Where the
//               accumulated moments serve, var_0 is final here; where they do not, the texel is marked (NEEDS_WINDOW); a
//               texel that is not filterable is marked too (NOT_FILTERABLE), here and by every pass but the last.
//   window   -- the 7 x 7 spatial estimate for the marked texels: a workgroup per tile of 32 x 8 texels with a halo of 3
//               in LDS, (normal.xyz, flag) and (point.xyz, l(c_0)) per texel.  A workgroup without a marked texel leaves
//               before it fills the tile: a frame whose moments serve everywhere pays one load per texel.
//   pass i   -- rt_denoise's pass with the luminance edge term: one lane per texel, a workgroup per 32 x 8 tile, the 3 x 3
//               prefilter of the variance first, then the 25 taps a row of five at a time -- the row's loads, then its
//               weights.  Steps 1 and 2 read an LDS copy of the tile and its halo (the 3 x 3 window lies inside it),
//               larger steps global memory.  The last pass remodulates and writes `out` and `out_variance`.
// The per-tap arithmetic is csrc/rt_vdenoise.h, shared with the host restatement (host/vdenoise.cpp); this file is compiled
// with -ffp-contract=off, so the result is the host's bit for bit.
//
// Bounds: as rt_denoise.hip.  A lane outside the frame takes part in filling the LDS tile (from texels inside the frame
// only) and in the workgroup's vote, and leaves before any access of its own; a tap outside the frame reads the lane's own
// texel instead (direct form) or an LDS slot filled as "not filterable" (tiled forms: every tap lies inside the halo) and
// adds nothing; texel indices are < 2^31 (the entry point checks), and every address is formed in 64 bits.
#include <hip/hip_runtime.h>

#include "rt_vdenoise.h"
#include "rt_vdenoise_api.h"

namespace rtd {
namespace {

constexpr uint32_t TILE_W = 32, TILE_H = 8, VDENOISE_THREADS = TILE_W * TILE_H;
// What the fourth component of a (colour, variance) texel holds in place of a variance, which is never negative (+0, a
// positive number or a NaN): NOT_FILTERABLE on a texel that is no tap -- the prefilter tells by it alone, one load per
// neighbour --, NEEDS_WINDOW on a filterable texel whose variance the window kernel has yet to estimate.
constexpr float NOT_FILTERABLE = -1.0f, NEEDS_WINDOW = -2.0f;

typedef float v4f __attribute__((ext_vector_type(4)));
#define RT_GLOBAL(T, p) ((__attribute__((address_space(1))) T*)(void*)(p))

// written once and read by nobody in the launch
__device__ __forceinline__ void store_out(float* out, size_t p, float4 v) {
    __builtin_nontemporal_store(v4f{v.x, v.y, v.z, v.w}, RT_GLOBAL(v4f, reinterpret_cast<float4*>(out) + p));
}

// What prepare and moments read of a texel: is it filterable, its a' and its demodulated colour.
struct Texel {
    bool ok;
    float4 color, al, c0;
    float n[3], x[3];
};
__device__ __forceinline__ Texel read_texel(const VDenoiseArgs& a, size_t p) {
    Texel t;
    t.color = reinterpret_cast<const float4*>(a.color)[p];
    for (int k = 0; k < 3; ++k) {
        t.n[k] = a.normal[3 * p + k];
        t.x[k] = a.point[3 * p + k];
    }
    const float col[3] = {t.color.x, t.color.y, t.color.z};
    float4 e = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (a.emission) e = reinterpret_cast<const float4*>(a.emission)[p];
    const float em[3] = {e.x, e.y, e.z};
    t.ok = rtdn::filterable(t.n, t.x, col, em);
    t.al = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    if (a.albedo) {
        const float4 v = reinterpret_cast<const float4*>(a.albedo)[p];
        t.al = make_float4(rtdn::albedo_floor(v.x), rtdn::albedo_floor(v.y), rtdn::albedo_floor(v.z), 1.0f);
    }
    t.c0 = make_float4(t.color.x / t.al.x, t.color.y / t.al.y, t.color.z / t.al.z, 0.0f);
    return t;
}

__global__ void __launch_bounds__(VDENOISE_THREADS) rt_vdenoise_moments_kernel(const VDenoiseArgs a) {
    const size_t p = (size_t)blockIdx.x * VDENOISE_THREADS + threadIdx.x;
    if (p >= (size_t)a.width * a.height) return;
    const Texel t = read_texel(a, p);
    const float l = rtvd::luminance(t.c0.x, t.c0.y, t.c0.z);
    store_out(a.out, p, t.ok ? make_float4(l, l * l, 0.0f, 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f));
}

__global__ void __launch_bounds__(VDENOISE_THREADS) rt_vdenoise_prepare_kernel(const VDenoiseArgs a) {
    const size_t p = (size_t)blockIdx.x * VDENOISE_THREADS + threadIdx.x;
    if (p >= (size_t)a.width * a.height) return;
    const Texel t = read_texel(a, p);
    float var = t.ok ? NEEDS_WINDOW : NOT_FILTERABLE;
    if (t.ok && a.moments) {
        const float4 m = reinterpret_cast<const float4*>(a.moments)[p];
        const float hist = a.history[p];
        if (rtvd::temporal_serves(m.x, m.y, hist, a.min_history)) var = rtvd::clamp_variance(rtvd::temporal_variance(m.x, m.y, hist));
    }
    float4* guide = static_cast<float4*>(a.guide);
    guide[2 * p] = make_float4(t.n[0], t.n[1], t.n[2], t.ok ? 1.0f : 0.0f);
    guide[2 * p + 1] = make_float4(t.x[0], t.x[1], t.x[2], 0.0f);
    static_cast<float4*>(a.ping[0])[p] = make_float4(t.c0.x, t.c0.y, t.c0.z, var);
}

// The 7 x 7 spatial estimate of var_0, for the texels prepare marked.  c0v: a.ping[0], whose fourth component this kernel
// completes; the other three, which the neighbours' workgroups read meanwhile, it leaves alone (a 4-byte store).
__global__ void __launch_bounds__(VDENOISE_THREADS) rt_vdenoise_window_kernel(const VDenoiseArgs a, const float k_n, const float k_x) {
    constexpr uint32_t HALO = 3, RW = TILE_W + 2 * HALO, RH = TILE_H + 2 * HALO, R = RW * RH;
    __shared__ float4 tile_n[R], tile_xl[R];
    const uint32_t tiles_x = (a.width + TILE_W - 1) / TILE_W;
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const uint32_t lx = threadIdx.x & (TILE_W - 1), ly = threadIdx.x / TILE_W;
    const uint32_t x = tx * TILE_W + lx, y = ty * TILE_H + ly;
    const bool in_frame = x < a.width && y < a.height;
    const size_t p = in_frame ? (size_t)y * a.width + (size_t)x : 0;
    float* c0v = static_cast<float*>(a.ping[0]);
    const bool need = in_frame && c0v[4 * p + 3] == NEEDS_WINDOW;
    if (!__syncthreads_or(need ? 1 : 0)) return;   // (uniform over the workgroup)
    const float4* guide = static_cast<const float4*>(a.guide);
    for (uint32_t r = threadIdx.x; r < R; r += VDENOISE_THREADS) {
        const uint32_t ry = r / RW, rx = r - ry * RW;
        // (unsigned: left of column 0 or below row 0 wraps to at least 2^32 - 3 and fails the comparison)
        const uint32_t gx = tx * TILE_W + rx - HALO, gy = ty * TILE_H + ry - HALO;
        float4 qn = make_float4(0.0f, 0.0f, 0.0f, 0.0f), qx = qn;
        if (gx < a.width && gy < a.height) {
            const size_t q = (size_t)gy * a.width + (size_t)gx;
            qn = guide[2 * q];
            const float4 g1 = guide[2 * q + 1];
            const float* c = c0v + 4 * q;
            qx = make_float4(g1.x, g1.y, g1.z, rtvd::luminance(c[0], c[1], c[2]));
        }
        tile_n[r] = qn;
        tile_xl[r] = qx;
    }
    __syncthreads();
    if (!need) return;
    const uint32_t centre = (ly + HALO) * RW + lx + HALO;
    const float4 pn = tile_n[centre], px = tile_xl[centre];
    const float np[3] = {pn.x, pn.y, pn.z}, xp[3] = {px.x, px.y, px.z};
    float s1 = 0.0f, s2 = 0.0f, sw = 0.0f;
    // (a loop over the rows, a row's seven taps unrolled: the loads of a row before its weights, as in the passes)
#pragma unroll 1
    for (int dy = -3; dy <= 3; ++dy) {
        float4 qn[7], qx[7];
#pragma unroll
        for (int dx = -3; dx <= 3; ++dx) {
            const uint32_t i = (uint32_t)((int)centre + dy * (int)RW + dx);   // (inside the halo)
            qn[dx + 3] = tile_n[i];
            qx[dx + 3] = tile_xl[i];
        }
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const float nq[3] = {qn[k].x, qn[k].y, qn[k].z}, xq[3] = {qx[k].x, qx[k].y, qx[k].z};
            const float u = rtvd::window_weight(np, nq, xp, xq, k_n, k_x);
            const bool take = qn[k].w != 0.0f && u > 0.0f;
            const float l = qx[k].w;
            s1 += take ? u * l : 0.0f;
            s2 += take ? u * (l * l) : 0.0f;
            sw += take ? u : 0.0f;
        }
    }
    c0v[4 * p + 3] = rtvd::clamp_variance(rtvd::spatial_variance(s1, s2, sw));
}

// One tap's texel as the passes hold it: (normal.xyz, the guide's flag -- read at the lane's own texel only, so that a tap's
// is never kept), (point.xyz, colour.x), (colour.y, colour.z, variance or NOT_FILTERABLE, luminance -- in the tiled forms) --
// three 16-byte LDS planes.
struct Tap {
    float4 n, xc, cv;
    bool in;
};

// What a texel gathers over its taps.  A tap that the definition skips adds +0, which leaves the sums (never -0: they
// start at +0) as they are, bit for bit: what a tap adds is selected after its weight.
struct Gather {
    float np[3], xp[3];
    float lp, D, k_n, k_x;
    float sum[3] = {0.0f, 0.0f, 0.0f}, vsum = 0.0f, wsum = 0.0f;
    // HAS_LUM: t.cv.w holds the tap's luminance (the tiled forms evaluate it once per texel, when they fill the tile)
    template <bool HAS_LUM>
    __device__ __forceinline__ void tap(int dx, int dy, const Tap& t) {
        const float nq[3] = {t.n.x, t.n.y, t.n.z}, xq[3] = {t.xc.x, t.xc.y, t.xc.z}, cq[3] = {t.xc.w, t.cv.x, t.cv.y};
        const float lq = HAS_LUM ? t.cv.w : rtvd::luminance(cq[0], cq[1], cq[2]);
        const float w = rtvd::tap_weight(rtdn::kernel_h(dx) * rtdn::kernel_h(dy), lp, lq, D, np, nq, xp, xq, k_n, k_x);
        const bool take = t.in && !(t.cv.z < 0.0f) && w > 0.0f;   // (a texel that is no tap holds NOT_FILTERABLE there)
        sum[0] += take ? w * cq[0] : 0.0f;
        sum[1] += take ? w * cq[1] : 0.0f;
        sum[2] += take ? w * cq[2] : 0.0f;
        vsum += take ? (w * w) * t.cv.z : 0.0f;
        wsum += take ? w : 0.0f;
    }
};

// One pass.  src: (c_i, var_i); dst: (c_{i+1}, var_{i+1}) (unused by the last pass, which writes a.out and a.out_variance).
// LDS_STEP == 0, the direct form, for any step; LDS_STEP == s > 0 (1 and 2 are instantiated), the tiled form for step s, with
// a halo of 2 s texels: rt_denoise.hip's two forms, with 48 bytes per texel in LDS instead of 40 (the variance and the
// luminance, evaluated once per texel when the tile is filled instead of once per tap).
template <bool LAST, int LDS_STEP>
__global__ void __launch_bounds__(VDENOISE_THREADS) rt_vdenoise_pass_kernel(const VDenoiseArgs a, const int step, const float k_n, const float k_x,
                                                                            const float4* __restrict__ src, float4* __restrict__ dst) {
    constexpr uint32_t S = (uint32_t)LDS_STEP, RW = TILE_W + 4 * S, RH = TILE_H + 4 * S, R = RW * RH;
    __shared__ float4 tile_n[LDS_STEP ? R : 1], tile_xc[LDS_STEP ? R : 1], tile_cv[LDS_STEP ? R : 1];
    const uint32_t tiles_x = (a.width + TILE_W - 1) / TILE_W;
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const uint32_t lx = threadIdx.x & (TILE_W - 1), ly = threadIdx.x / TILE_W;
    const uint32_t x = tx * TILE_W + lx, y = ty * TILE_H + ly;   // (< 2^31 + 32)
    const float4* guide = static_cast<const float4*>(a.guide);
    if constexpr (LDS_STEP != 0) {
        for (uint32_t r = threadIdx.x; r < R; r += VDENOISE_THREADS) {
            const uint32_t ry = r / RW, rx = r - ry * RW;
            // (unsigned: left of column 0 or below row 0 wraps to at least 2^32 - 2 s and fails the comparison)
            const uint32_t gx = tx * TILE_W + rx - 2 * S, gy = ty * TILE_H + ry - 2 * S;
            float4 qn = make_float4(0.0f, 0.0f, 0.0f, 0.0f), qg = qn, qc = make_float4(0.0f, 0.0f, 0.0f, NOT_FILTERABLE);
            if (gx < a.width && gy < a.height) {
                const size_t q = (size_t)gy * a.width + (size_t)gx;
                qn = guide[2 * q];
                qg = guide[2 * q + 1];
                qc = src[q];
            }
            tile_n[r] = qn;
            tile_xc[r] = make_float4(qg.x, qg.y, qg.z, qc.x);
            tile_cv[r] = make_float4(qc.y, qc.z, qc.w, rtvd::luminance(qc.x, qc.y, qc.z));
        }
        __syncthreads();
    }
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * a.width + (size_t)x;
    const uint32_t centre = (ly + 2 * S) * RW + lx + 2 * S;   // (the tiled form: this texel in the LDS planes)
    const float4 gn = LDS_STEP ? tile_n[centre] : guide[2 * p];
    if (gn.w == 0.0f) {
        if (LAST) {
            store_out(a.out, p, reinterpret_cast<const float4*>(a.color)[p]);
            if (a.out_variance) a.out_variance[p] = 0.0f;
        } else {
            dst[p] = make_float4(0.0f, 0.0f, 0.0f, NOT_FILTERABLE);   // (the next pass's prefilter reads it)
        }
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
                t[dx + 2] = Tap{tile_n[i], tile_xc[i], tile_cv[i], true};
            } else {
                const uint32_t qx = x + (uint32_t)(step * dx);
                const bool in = in_y && qx < a.width;
                const size_t q = in ? (size_t)qy * a.width + (size_t)qx : p;
                const float4 qg = guide[2 * q + 1], qc = src[q];
                t[dx + 2] = Tap{guide[2 * q], make_float4(qg.x, qg.y, qg.z, qc.x), make_float4(qc.y, qc.z, qc.w, 0.0f), in};
            }
        }
    };
    // the prefilter: the 3 x 3 mean of the variance over the filterable texels, at unit spacing whatever the step
    float gs = 0.0f, gw = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            float var;
            bool in = true;
            if constexpr (LDS_STEP != 0) {
                var = tile_cv[(uint32_t)((int)centre + dy * (int)RW + dx)].z;   // (the halo is at least 2 wide)
            } else {
                const uint32_t qx = x + (uint32_t)dx, qy = y + (uint32_t)dy;   // (unsigned: -1 wraps and fails the comparison)
                in = qx < a.width && qy < a.height;
                const size_t q = in ? (size_t)qy * a.width + (size_t)qx : p;
                var = reinterpret_cast<const float*>(src)[4 * q + 3];
            }
            const bool take = in && !(var < 0.0f);   // (NOT_FILTERABLE is the one negative value; a NaN variance counts)
            const float g = rtvd::kernel_g(dx) * rtvd::kernel_g(dy);
            gs += take ? g * var : 0.0f;
            gw += take ? g : 0.0f;
        }
    Tap cur[5];
    load_row(-2, cur);
    Gather g;
    {
        // this texel's own values
        float4 gx, cc;
        if constexpr (LDS_STEP != 0) {
            const float4 xc = tile_xc[centre], cv = tile_cv[centre];
            gx = make_float4(xc.x, xc.y, xc.z, 0.0f);
            cc = make_float4(xc.w, cv.x, cv.y, 0.0f);
        } else {
            gx = guide[2 * p + 1];
            cc = src[p];
        }
        g = Gather{{gn.x, gn.y, gn.z}, {gx.x, gx.y, gx.z}, rtvd::luminance(cc.x, cc.y, cc.z), rtvd::luminance_scale(a.sigma_luminance, gs / gw), k_n, k_x};
    }
    // (the loop over the rows stays a loop, the next row's loads issued behind this row's arithmetic: rt_denoise.hip)
#pragma unroll 1
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) g.template tap<LDS_STEP != 0>(dx, dy, cur[dx + 2]);
        if (dy < 2) load_row(dy + 1, cur);
    }
    const float4 c = make_float4(g.sum[0] / g.wsum, g.sum[1] / g.wsum, g.sum[2] / g.wsum, g.vsum / (g.wsum * g.wsum));
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
    if (a.out_variance) a.out_variance[p] = c.w;
}

template <int LDS_STEP>
void launch_pass(bool last, uint32_t tiles, hipStream_t stream, const VDenoiseArgs& a, int step, float k_n, float k_x, const float4* src,
                 float4* dst) {
    if (last)
        hipLaunchKernelGGL((rt_vdenoise_pass_kernel<true, LDS_STEP>), dim3(tiles), dim3(VDENOISE_THREADS), 0, stream, a, step, k_n, k_x, src, dst);
    else
        hipLaunchKernelGGL((rt_vdenoise_pass_kernel<false, LDS_STEP>), dim3(tiles), dim3(VDENOISE_THREADS), 0, stream, a, step, k_n, k_x, src, dst);
}

}  // namespace

hipError_t launch_luminance_moments(const VDenoiseArgs& a, hipStream_t stream) {
    const size_t texels = (size_t)a.width * a.height;
    hipLaunchKernelGGL(rt_vdenoise_moments_kernel, dim3((uint32_t)((texels + VDENOISE_THREADS - 1) / VDENOISE_THREADS)), dim3(VDENOISE_THREADS),
                       0, stream, a);
    return hipGetLastError();
}

// prepare, the window estimate, then a.iterations passes over the two (colour, variance) images; the last one writes
// a.out and a.out_variance.
hipError_t launch_vdenoise(const VDenoiseArgs& a, hipStream_t stream) {
    const size_t texels = (size_t)a.width * a.height;
    const float k_n = rtdn::k_of_sigma(a.sigma_normal), k_x = rtdn::k_of_sigma(a.sigma_point);
    const uint32_t tiles = ((a.width + TILE_W - 1) / TILE_W) * ((a.height + TILE_H - 1) / TILE_H);   // (<= 2^31 / 8 + ...: fits)
    hipLaunchKernelGGL(rt_vdenoise_prepare_kernel, dim3((uint32_t)((texels + VDENOISE_THREADS - 1) / VDENOISE_THREADS)), dim3(VDENOISE_THREADS),
                       0, stream, a);
    hipLaunchKernelGGL(rt_vdenoise_window_kernel, dim3(tiles), dim3(VDENOISE_THREADS), 0, stream, a, k_n, k_x);
    for (int i = 0; i < a.iterations; ++i) {
        const float4* src = static_cast<const float4*>(a.ping[i & 1]);
        float4* dst = static_cast<float4*>(a.ping[(i + 1) & 1]);
        const bool last = i + 1 == a.iterations;
        const int step = 1 << i;
        if (step == 1) launch_pass<1>(last, tiles, stream, a, step, k_n, k_x, src, dst);
        else if (step == 2) launch_pass<2>(last, tiles, stream, a, step, k_n, k_x, src, dst);
        else launch_pass<0>(last, tiles, stream, a, step, k_n, k_x, src, dst);
    }
    return hipGetLastError();
}

}  // namespace rtd
