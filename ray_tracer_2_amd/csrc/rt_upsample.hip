// rt_upsample.hip -- the device kernel of guided upsampling (include/rt_abi.h: rt_upsample).
//
// One lane per HIGH texel, a workgroup per tile of 32 x 8 of them (a wave: 32 x 2, the denoiser's map), so that the taps
// of neighbouring lanes fall into neighbouring -- at a ratio above one, the same -- texels of the low frame.  A lane reads
// its own texel's depth, point, normal, object word and, where the planes are there, emission and albedo, classifies itself,
// takes ring 1's four bilinear taps a row of two at a time (the row's reads first, then its validations: what a tap adds
// is selected afterwards, rtup::Sums::add, so no branch stands between the reads) and writes `out` and `coverage` with
// streaming stores.  Ring 2 and the hole are a branch behind ring 1 that a texel with a valid tap does not enter: a loop
// over the sixteen taps that is not unrolled, one tap's loads at a time, so that the rare path adds no registers to the
// common one.
// Ring 1 reads its taps from LDS: the workgroup first copies the low texels its tile can reach in ring 1 -- columns
// x0(X_first) .. x0(X_last) + 1 and the rows likewise: at most (ceil(31 rx) + 3) x (ceil(7 ry) + 3) -- each made into its tap
// record once (rtup::make_tap: the finite / non-zero tests and the demodulation's three divisions are then done per low
// texel, not per tap -- at a ratio of 2 sixteen high texels tap a low one), as three float4 planes (colour; point.xyz,
// object; normal.xyz, flags) and, with the albedo planes, a float2 and a float plane of the demodulated rgb: no dead words,
// a tap is three ds_read_b128 (and a b64 and a b32).  The lanes one LDS cycle serves lie in one tile row and read
// consecutive or equal elements.  A tile whose reach does not fit LDS_TEXELS (downscaling) loads its taps from global
// memory instead -- 44 bytes a tap, 60 with the albedo planes, a tap outside the low frame from the nearest texel inside --
// a decision that is uniform in the workgroup; ring 2 and the hole always load that way.  Loading every tap directly was
// measured against this and lost; the two agree bit for bit.
// The per-texel arithmetic is csrc/rt_upsample.h, shared with the host restatement (host/upsample.cpp); this file is
// compiled with -ffp-contract=off, so the result is the host's bit for bit.
//
// Bounds: a lane outside the high frame takes part in filling the LDS tile and leaves before any access of its own.  A
// lane's own index p < W * H and every low index q -- both coordinates clamped into the low frame -- < w * h, both
// <= 2^31 - 1 (the entry point checks), and every address is formed in 64 bits.  fx = f32(X) * rx >= 0, so the snapped
// origin x0 is in [0, w] (rx <= (w - 1) / (W - 1) up to rounding, and a position past w - 1 by rounding snaps down to it)
// and ring 2's columns x0 - 1 .. x0 + 2 fit an int32; likewise the rows.  The LDS tile is written at r < rw * rh <=
// LDS_TEXELS (checked in the kernel before the fill) and read at (qx - x_lo) + (qy - y_lo) * rw with x_lo <= x0 and
// x0 + 1 <= x_hi for every lane of the tile (x0 is monotone in X), the rows likewise.
#include <hip/hip_runtime.h>

#include "rt_upsample.h"
#include "rt_upsample_api.h"

namespace rtd {
namespace {

constexpr uint32_t TILE_W = 32, TILE_H = 8, UPSAMPLE_THREADS = TILE_W * TILE_H;
// The low texels a workgroup may hold in LDS: 60 bytes each, 20,400 bytes in all, so that LDS never bounds the occupancy --
// eight workgroups fit a CU's 160 KiB, and the kernel's 69 registers allow seven.  Ratio 1 reaches 34 x 10 = 340 texels,
// ratio 2 19 x 7 = 133.
constexpr uint32_t LDS_TEXELS = 340;

typedef float v4f __attribute__((ext_vector_type(4)));
#define RT_GLOBAL(T, p) ((__attribute__((address_space(1))) T*)(void*)(p))

constexpr uint32_t FLAG_PLAIN = 1u, FLAG_GEOM = 2u;

// The low texel (qx, qy) from global memory, or the nearest one inside the frame when it is outside (and then refused).
__device__ __forceinline__ rtup::Tap load_tap(const UpsampleArgs& a, int32_t qx, int32_t qy) {
    const uint32_t w = a.call.lo_width, h = a.call.lo_height;
    // (as unsigned, -1 wraps past w and fails the one comparison, like w and w + 1)
    const bool inside = (uint32_t)qx < w && (uint32_t)qy < h;
    const uint32_t cx = qx < 0 ? 0u : (uint32_t)qx >= w ? w - 1u : (uint32_t)qx;
    const uint32_t cy = qy < 0 ? 0u : (uint32_t)qy >= h ? h - 1u : (uint32_t)qy;
    const size_t q = (size_t)cy * w + (size_t)cx;
    const float4 pc = reinterpret_cast<const float4*>(a.lo_color)[q];
    const float c[4] = {pc.x, pc.y, pc.z, pc.w};
    const float x[3] = {a.lo_point[3 * q], a.lo_point[3 * q + 1], a.lo_point[3 * q + 2]};
    const float n[3] = {a.lo_normal[3 * q], a.lo_normal[3 * q + 1], a.lo_normal[3 * q + 2]};
    float al[3] = {1.0f, 1.0f, 1.0f};
    if (a.lo_albedo) {
        const float4 v = reinterpret_cast<const float4*>(a.lo_albedo)[q];
        al[0] = v.x; al[1] = v.y; al[2] = v.z;
    }
    return rtup::make_tap(inside, c, x, n, a.lo_object[q], a.lo_albedo != nullptr, al);
}

__global__ void __launch_bounds__(UPSAMPLE_THREADS) rt_upsample_kernel(const UpsampleArgs a) {
    __shared__ float4 tile_c[LDS_TEXELS], tile_xo[LDS_TEXELS], tile_nf[LDS_TEXELS];
    __shared__ float2 tile_d01[LDS_TEXELS];
    __shared__ float tile_d2[LDS_TEXELS];
    const rtup::Call& c = a.call;
    const uint32_t W = c.width, H = c.height;
    const uint32_t tiles_x = (W + TILE_W - 1) / TILE_W;
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const uint32_t X0 = tx * TILE_W, Y0 = ty * TILE_H;
    const uint32_t X = X0 + (threadIdx.x & (TILE_W - 1)), Y = Y0 + threadIdx.x / TILE_W;   // (< 2^31 + 32)
    const bool have_albedo = a.albedo != nullptr;   // (and lo_albedo: the entry point checks)

    // the low columns and rows that ring 1 of this tile's texels (those inside the frame) can touch
    const uint32_t X1 = X0 + TILE_W - 1 < W ? X0 + TILE_W - 1 : W - 1, Y1 = Y0 + TILE_H - 1 < H ? Y0 + TILE_H - 1 : H - 1;
    const int32_t x_lo = rttp::snap_axis((float)X0 * c.rx).i0, y_lo = rttp::snap_axis((float)Y0 * c.ry).i0;
    const uint32_t rw = (uint32_t)(rttp::snap_axis((float)X1 * c.rx).i0 + 1 - x_lo) + 1u;
    const uint32_t rh = (uint32_t)(rttp::snap_axis((float)Y1 * c.ry).i0 + 1 - y_lo) + 1u;
    const bool tiled = rw <= LDS_TEXELS && rh <= LDS_TEXELS && rw * rh <= LDS_TEXELS;   // (uniform in the workgroup)
    if (tiled) {
        const uint32_t R = rw * rh;
        for (uint32_t r = threadIdx.x; r < R; r += UPSAMPLE_THREADS) {
            const uint32_t ry = r / rw, rx = r - ry * rw;
            const rtup::Tap t = load_tap(a, x_lo + (int32_t)rx, y_lo + (int32_t)ry);
            tile_c[r] = make_float4(t.c[0], t.c[1], t.c[2], t.c[3]);
            tile_xo[r] = make_float4(t.x[0], t.x[1], t.x[2], __uint_as_float(t.obj));
            tile_nf[r] = make_float4(t.n[0], t.n[1], t.n[2], __uint_as_float((t.plain_ok ? FLAG_PLAIN : 0u) | (t.geom_ok ? FLAG_GEOM : 0u)));
            if (have_albedo) {
                tile_d01[r] = make_float2(t.d[0], t.d[1]);
                tile_d2[r] = t.d[2];
            }
        }
        __syncthreads();
    }
    if (X >= W || Y >= H) return;
    const size_t p = (size_t)Y * W + (size_t)X;

    rtup::Texel P;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        P.n[k] = a.normal[3 * p + k];
        P.x[k] = a.point[3 * p + k];
    }
    P.depth = a.depth[p];
    P.obj = a.object[p];
    float em[3] = {0.0f, 0.0f, 0.0f};
    if (a.emission) {
        const float4 e = reinterpret_cast<const float4*>(a.emission)[p];
        em[0] = e.x; em[1] = e.y; em[2] = e.z;
    }
    float al[3] = {1.0f, 1.0f, 1.0f};
    if (have_albedo) {
        const float4 v = reinterpret_cast<const float4*>(a.albedo)[p];
        al[0] = v.x; al[1] = v.y; al[2] = v.z;
    }
    const bool is_guided = rtup::guided(P, em);
    const bool demod = is_guided && have_albedo;
    const float reach = c.point_tolerance * P.depth;
    const rtup::Where w = rtup::locate(c, X, Y);

    // a tap of ring 1
    auto ring1_tap = [&](int i) {
        const int32_t qx = w.ax.i0 + rttp::tap_dx(i), qy = w.ay.i0 + rttp::tap_dy(i);
        if (tiled) {
            const uint32_t r = (uint32_t)(qy - y_lo) * rw + (uint32_t)(qx - x_lo);   // (inside the tile: see the head)
            const float4 tc = tile_c[r], txo = tile_xo[r], tnf = tile_nf[r];
            const uint32_t flags = __float_as_uint(tnf.w);
            rtup::Tap t{{tc.x, tc.y, tc.z, tc.w}, {tc.x, tc.y, tc.z}, {txo.x, txo.y, txo.z}, {tnf.x, tnf.y, tnf.z},
                        __float_as_uint(txo.w), (flags & FLAG_PLAIN) != 0u, (flags & FLAG_GEOM) != 0u};
            if (have_albedo) {
                const float2 d01 = tile_d01[r];
                t.d[0] = d01.x; t.d[1] = d01.y; t.d[2] = tile_d2[r];
            }
            return t;
        }
        return load_tap(a, qx, qy);
    };

    rtup::Sums s;
    uint8_t cover = rtup::COVER_RING1;
#pragma unroll
    for (int row = 0; row < 2; ++row) {
        const rtup::Tap t0 = ring1_tap(2 * row), t1 = ring1_tap(2 * row + 1);
        s.add(rttp::tap_weight(2 * row, w.ax.t, w.ay.t), t0, P, is_guided, demod, reach, c.normal_cos);
        s.add(rttp::tap_weight(2 * row + 1, w.ax.t, w.ay.t), t1, P, is_guided, demod, reach, c.normal_cos);
    }
    float v[4];
    if (s.have()) {
        s.mean(v);
    } else {
        // the rare path: ring 2, one tap at a time, then the hole
        s = rtup::Sums{};
#pragma unroll 1
        for (int j = -1; j <= 2; ++j) {
#pragma unroll 1
            for (int i = -1; i <= 2; ++i)
                s.add(rtup::ring2_weight(i, j, w.ax.t, w.ay.t), load_tap(a, w.ax.i0 + i, w.ay.i0 + j), P, is_guided, demod, reach, c.normal_cos);
        }
        if (s.have()) {
            cover = rtup::COVER_RING2;
            s.mean(v);
        } else {
            cover = rtup::COVER_HOLE;
            rtup::tap_color(load_tap(a, (int32_t)rtup::nearest(w.ax, c.lo_width), (int32_t)rtup::nearest(w.ay, c.lo_height)), demod, v);
        }
    }
    float out[4];
    rtup::finish(v, demod, al, out);
    // written once and read by nobody in the launch: streaming stores
    __builtin_nontemporal_store(v4f{out[0], out[1], out[2], out[3]}, RT_GLOBAL(v4f, reinterpret_cast<float4*>(a.out) + p));
    if (a.coverage) __builtin_nontemporal_store(cover, RT_GLOBAL(uint8_t, a.coverage + p));
}

}  // namespace

hipError_t launch_upsample(const UpsampleArgs& a, hipStream_t stream) {
    const uint32_t tiles = ((a.call.width + TILE_W - 1) / TILE_W) * ((a.call.height + TILE_H - 1) / TILE_H);   // (<= 2^31 / 8 + ...: fits)
    hipLaunchKernelGGL(rt_upsample_kernel, dim3(tiles), dim3(UPSAMPLE_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace rtd
