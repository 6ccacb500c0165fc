// rt_rectify.hip -- the device kernel of history rectification (include/rt_abi.h: rt_temporal_rectify; DESIGN.md section
// 2.20).
//
// One lane per texel, a workgroup per tile of 32 x 8 of them (a wave: 32 x 2, the temporal kernel's map).  A lane's window
// is up to 7 x 7 taps of `color`, and neighbouring lanes share all but a column of them, so the workgroup first copies its
// tile and a halo of `radius` texels -- (32 + 2 r) x (8 + 2 r), at most 38 x 14 = 532 -- into LDS, one 16-byte record per
// texel: r, g, b and a key word.  The staging lane decides once whether the texel is inside the frame and its rgb finite:
//   with an object plane  a texel that counts holds (r, g, b, object word), one that does not holds (NaN, 0, 0, 0), and a tap
//                         counts when its key equals the lane's own object word and its r is not NaN;
//   without one           a texel that counts holds (r, g, b, 1), one that does not (0, 0, 0, 0): such a tap adds +0 to the
//                         sums, which leaves them as they are bit for bit (rt_rectify.h), and its key to the count, so a tap
//                         costs no compare at all.
// A tap is then one ds_read_b128 -- the sixteen lanes one LDS cycle serves lie in one tile row and read consecutive records,
// every bank once -- and the sums' nine operations (three products, six sums), in the definition's order: dy outer, dx
// inner, nothing separable.  The radius and the presence of the object plane are template parameters: six kernels, each with
// its window's rows unrolled and its LDS tile sized for its radius (5,440, 6,912 and 8,512 bytes).
// The lane's own reads -- color, history, history_length, the object word and the moments, each at its own texel only, which
// is what lets out be history, out_history history_length and out_moments history_moments -- are issued before the window
// loop and first used after it.  out, out_history, out_moments and out_clipped are written once and read by nobody in the
// launch: streaming stores.
// The per-texel arithmetic is csrc/rt_rectify.h, shared with the host restatement (host/rectify.cpp); this file is compiled
// with -ffp-contract=off, so the result is the host's bit for bit.
//
// Bounds: a lane outside the frame takes part in filling the LDS tile and leaves before any access of its own.  A staged
// texel's coordinates are formed in 64 bits and tested against the frame before its index q < width * height <= 2^31 - 1
// (the entry point checks) is; every address is formed in 64 bits.  The tile is written at r < LW * LH, its size, and read at
// (ly + R + dy) * LW + (lx + R + dx) with lx < 32, ly < 8 and |dx|, |dy| <= R: below LW * LH.
#include <hip/hip_runtime.h>

#include "rt_rectify.h"
#include "rt_rectify_api.h"

namespace rtd {
namespace {

constexpr uint32_t TILE_W = 32, TILE_H = 8, RECTIFY_THREADS = TILE_W * TILE_H;

typedef float v4f __attribute__((ext_vector_type(4)));
#define RT_GLOBAL(T, p) ((__attribute__((address_space(1))) T*)(void*)(p))

template <int R, bool OBJ>
__global__ void __launch_bounds__(RECTIFY_THREADS) rt_rectify_kernel(const RectifyArgs a) {
    constexpr uint32_t LW = TILE_W + 2 * R, LH = TILE_H + 2 * R, LN = LW * LH;
    __shared__ float4 tile[LN];
    const uint32_t W = a.call.width, H = a.call.height;
    const uint32_t tiles_x = (W + TILE_W - 1) / TILE_W;
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const uint32_t X0 = tx * TILE_W, Y0 = ty * TILE_H;
    const uint32_t lx = threadIdx.x & (TILE_W - 1), ly = threadIdx.x / TILE_W;
    const uint32_t x = X0 + lx, y = Y0 + ly;   // (< 2^31 + 32)
    const float nan = rttp::u2f(rttp::QUIET_NAN);

    for (uint32_t r = threadIdx.x; r < LN; r += RECTIFY_THREADS) {
        const uint32_t ry = r / LW, rx = r - ry * LW;
        const int64_t qx = (int64_t)X0 + (int64_t)rx - R, qy = (int64_t)Y0 + (int64_t)ry - R;
        float4 rec = OBJ ? make_float4(nan, 0.0f, 0.0f, 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (qx >= 0 && qx < (int64_t)W && qy >= 0 && qy < (int64_t)H) {
            const size_t q = (size_t)qy * W + (size_t)qx;
            const float4 c = reinterpret_cast<const float4*>(a.color)[q];
            const float rgb[3] = {c.x, c.y, c.z};
            uint32_t key = 1u;
            if constexpr (OBJ) key = a.object[q];
            if (rttp::finite3(rgb)) rec = make_float4(c.x, c.y, c.z, rttp::u2f(key));
        }
        tile[r] = rec;
    }
    __syncthreads();
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + (size_t)x;

    // the lane's own texel: issued here, used behind the window
    const float4 c4 = reinterpret_cast<const float4*>(a.color)[p];
    const float4 h4 = reinterpret_cast<const float4*>(a.history)[p];
    const float n = a.history_length[p];
    uint32_t obj = 0u;
    if constexpr (OBJ) obj = a.object[p];
    const bool have_moments = a.moments != nullptr;   // (and history_moments and out_moments: the entry point checks)
    float4 m4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hm4 = m4;
    if (have_moments) {
        m4 = reinterpret_cast<const float4*>(a.moments)[p];
        hm4 = reinterpret_cast<const float4*>(a.history_moments)[p];
    }

    // a row of the window at a time: the row's 2 R + 1 reads are issued together (28 registers at radius 3), the rows are a
    // loop -- unrolled whole, the compiler issues all 49 reads ahead of the sums and takes 219 registers for them
    rtrc::Sums s;
#pragma unroll 1
    for (int dy = -R; dy <= R; ++dy) {
#pragma unroll
        for (int dx = -R; dx <= R; ++dx) {
            const float4 t = tile[(ly + (uint32_t)(R + dy)) * LW + (lx + (uint32_t)(R + dx))];
            if constexpr (OBJ)
                s.add(rttp::f2u(t.w) == obj && t.x == t.x, t.x, t.y, t.z);
            else
                s.add_staged(t.x, t.y, t.z, rttp::f2u(t.w));
        }
    }

    const float color[4] = {c4.x, c4.y, c4.z, c4.w}, h[4] = {h4.x, h4.y, h4.z, h4.w};
    const float m[4] = {m4.x, m4.y, m4.z, m4.w}, hm[4] = {hm4.x, hm4.y, hm4.z, hm4.w};
    const rtrc::Result r = rtrc::resolve(a.call, s, color, h, n, have_moments, m, hm);
    __builtin_nontemporal_store(v4f{r.out[0], r.out[1], r.out[2], r.out[3]}, RT_GLOBAL(v4f, reinterpret_cast<float4*>(a.out) + p));
    __builtin_nontemporal_store(r.history, RT_GLOBAL(float, a.out_history + p));
    if (have_moments)
        __builtin_nontemporal_store(v4f{r.moments[0], r.moments[1], r.moments[2], r.moments[3]},
                                    RT_GLOBAL(v4f, reinterpret_cast<float4*>(a.out_moments) + p));
    if (a.out_clipped) __builtin_nontemporal_store(r.clipped, RT_GLOBAL(uint8_t, a.out_clipped + p));
}

template <int R>
void launch_radius(const RectifyArgs& a, uint32_t tiles, hipStream_t stream) {
    if (a.object)
        hipLaunchKernelGGL((rt_rectify_kernel<R, true>), dim3(tiles), dim3(RECTIFY_THREADS), 0, stream, a);
    else
        hipLaunchKernelGGL((rt_rectify_kernel<R, false>), dim3(tiles), dim3(RECTIFY_THREADS), 0, stream, a);
}

}  // namespace

hipError_t launch_rectify(const RectifyArgs& a, hipStream_t stream) {
    const uint32_t tiles = ((a.call.width + TILE_W - 1) / TILE_W) * ((a.call.height + TILE_H - 1) / TILE_H);   // (<= 2^31 / 8 + ...: fits)
    switch (a.call.radius) {   // (1, 2 or 3: the entry point checks)
        case 1: launch_radius<1>(a, tiles, stream); break;
        case 2: launch_radius<2>(a, tiles, stream); break;
        case 3: launch_radius<3>(a, tiles, stream); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace rtd
