// rt_temporal.hip -- the device kernels of temporal accumulation (include/rt_abi.h: rt_temporal_accumulate,
// rt_temporal_accumulate_moving, rt_temporal_accumulate_deforming).
//
// One texel body (temporal_texel) for the three calls, instantiated per kind in three kernels, so that the plain call does
// not pay for the table's tests nor the moving call for the triangle side's.
// One lane per current texel, a workgroup per tile of 32 x 8 texels (a wave: 32 x 2), so that the four taps of
// neighbouring lanes fall into neighbouring texels of the previous frame and a wave's gather touches a few rows of it.
// A lane reads its own texel's colour, point, normal and object word, leaves with the "no history" result when the texel
// is not reprojectable, cannot be carried (below) or falls off the previous screen, and otherwise issues the loads of all
// four taps -- from the previous frame's planes directly, a tap outside the frame from the nearest texel inside -- before
// any validity arithmetic; what a tap adds is selected afterwards (rttp::resolve), so no branch stands between the loads.
// out, out_history and motion are written once and read by nobody in the launch: streaming stores.
// With a motion table (MOVING, DEFORMING; `object` is required there) the lane's object word picks its record between the
// texel's own reads and its projection: outside the table there is no history; a still object's texel goes on as it is,
// without reading the record's matrices; a moved one's reads its 96 bytes (a wave's 64 adjacent texels hold a few objects
// at most: near-uniform addresses that stay in the cache; no LDS staging) and is carried into the previous frame's world
// (rttp::carry) before anything looks at its point and normal.
// With the triangle side (DEFORMING) a lane whose record says DEFORMED reads its primitive word and barycentrics, leaves
// with "no history" when the word is outside [tri_first, tri_first + n_prev_triangles) or a barycentric is not finite, and
// otherwise issues the six 16-byte loads of its previous triangle record (v1|uv .. n3|uv, 96 bytes, 16-byte aligned; the uv
// word of each row is not used and the compiler does not fetch it) before any arithmetic on them: a near-uniform gather
// like the table's, served by the cache (nothing is shared between lanes that the cache does not already share, and the
// kernel is bound by the planes it streams).  The carried point and normal (rttp::carry_deformed) then enter locate, the
// taps' loads and resolve unchanged.
// The per-texel arithmetic is csrc/rt_temporal.h, shared with the host restatement (host/temporal.cpp); this file is
// compiled with -ffp-contract=off, so the result is the host's bit for bit.
//
// Bounds: a lane outside the frame leaves before any access; a lane's own index p and every tap index q (both
// coordinates clamped into the frame) are < width * height <= 2^31 - 1 (the entry point checks), and every address is
// formed in 64 bits.  The snapped tap origin is in [-1, width] x [-1, height] (on screen: -1 < fx < width), so x0 + 1
// does not overflow an int32.  The parts a kind does not have are null and stand in branches its instantiation does not
// hold.  The motion table is read at record obj only after obj < n_objects.  The previous triangles are read at record
// t - tri_first only after tri_first <= t and t - tri_first < n_prev_triangles (the range test comes before the triangle
// load; tri_first + n_prev_triangles <= 2^32, the entry point checks), and the primitive, bary and flags planes at the
// lane's own p.
#include <hip/hip_runtime.h>

#include "rt_temporal.h"
#include "rt_temporal_api.h"

namespace rtd {
using rt2::TemporalKind;
namespace {

constexpr uint32_t TILE_W = 32, TILE_H = 8, TEMPORAL_THREADS = TILE_W * TILE_H;

typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));
#define RT_GLOBAL(T, p) ((__attribute__((address_space(1))) T*)(void*)(p))

__device__ __forceinline__ void store_texel(const TemporalArgs& a, size_t p, const float out[4], float history, float mx, float my) {
    __builtin_nontemporal_store(v4f{out[0], out[1], out[2], out[3]}, RT_GLOBAL(v4f, reinterpret_cast<float4*>(a.out) + p));
    __builtin_nontemporal_store(history, RT_GLOBAL(float, a.out_history + p));
    if (a.motion) __builtin_nontemporal_store(v2f{mx, my}, RT_GLOBAL(v2f, reinterpret_cast<float2*>(a.motion) + p));
}

// The carry step of a kind with a table: X, n of texel p, whose object word is obj, into the previous frame's world.
// False: the texel has no history.
template <TemporalKind KIND>
__device__ __forceinline__ bool carry_texel(const TemporalArgs& a, size_t p, uint32_t obj, float X[3], float n[3]) {
    // (obj < n_objects before the table is touched: nothing is read outside it)
    if (!rttp::in_table(obj, a.n_objects)) return false;
    const rttp::Motion* m = a.motions + obj;
    const uint32_t moved = m->moved;
    float cx[3], cn[3];
    bool deformed = false;   // (to the moving kind every non-zero `moved` is rigid)
    if constexpr (KIND == TemporalKind::DEFORMING) deformed = moved == rttp::DEFORMED;
    if (deformed) {
        const uint32_t t = a.primitive[p];
        const float u = a.bary[2 * p], v = a.bary[2 * p + 1];   // (4-byte aligned: two loads)
        const bool backface = (a.flags[p] & rttp::HIT_BACKFACE) != 0u;
        // (t in [tri_first, tri_first + n_prev_triangles) before the array is touched: nothing is read outside it)
        if (!rttp::has_prev_triangle(t, a.tri_first, a.n_prev_triangles, u, v)) return false;
        const float4* rows = reinterpret_cast<const float4*>(a.prev_triangles + (size_t)(t - a.tri_first));
        const float4 r0 = rows[0], r1 = rows[1], r2 = rows[2], r3 = rows[3], r4 = rows[4], r5 = rows[5];
        const rttp::Tri tri{{r0.x, r0.y, r0.z}, r0.w, {r1.x, r1.y, r1.z}, r1.w, {r2.x, r2.y, r2.z}, r2.w,
                            {r3.x, r3.y, r3.z}, r3.w, {r4.x, r4.y, r4.z}, r4.w, {r5.x, r5.y, r5.z}, r5.w};
        if (!rttp::carry_deformed(*m, tri, u, v, backface, cx, cn)) return false;
    } else if (moved != 0u) {
        if (!rttp::carry(*m, X, n, cx, cn)) return false;
    } else {
        return true;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) X[k] = cx[k], n[k] = cn[k];
    return true;
}

template <TemporalKind KIND>
__device__ __forceinline__ void temporal_texel(const TemporalArgs& a) {
    constexpr bool TABLE = KIND != TemporalKind::PLAIN;
    const uint32_t W = a.call.width, H = a.call.height;
    const uint32_t tiles_x = (W + TILE_W - 1) / TILE_W;
    const uint32_t ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const uint32_t x = tx * TILE_W + (threadIdx.x & (TILE_W - 1)), y = ty * TILE_H + threadIdx.x / TILE_W;   // (< 2^31 + 32)
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + (size_t)x;
    const float4 c4 = reinterpret_cast<const float4*>(a.color)[p];
    const float color[4] = {c4.x, c4.y, c4.z, c4.w};
    float X[3] = {a.point[3 * p], a.point[3 * p + 1], a.point[3 * p + 2]};
    float n[3] = {a.normal[3 * p], a.normal[3 * p + 1], a.normal[3 * p + 2]};
    // (with a table the object plane is there, the entry point checks)
    const bool have_object = TABLE || a.object != nullptr;
    const uint32_t obj = have_object ? a.object[p] : 0u;
    const float nan = rttp::u2f(rttp::QUIET_NAN);
    bool go = rttp::reprojectable(n, X, have_object, obj);
    if constexpr (TABLE) go = go && carry_texel<KIND>(a, p, obj, X, n);
    if (!go) {
        store_texel(a, p, color, 1.0f, nan, nan);
        return;
    }
    const rttp::Where w = rttp::locate(a.call, X, x, y);
    if (!w.on_screen) {
        store_texel(a, p, color, 1.0f, nan, nan);
        return;
    }
    const bool match_object = have_object && a.prev_object != nullptr;
    rttp::Tap taps[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        // (x0 is in [-1, W]: as unsigned, -1 wraps past W and fails the one comparison, like W and W + 1)
        const int32_t qx = w.ax.i0 + rttp::tap_dx(i), qy = w.ay.i0 + rttp::tap_dy(i);
        rttp::Tap& t = taps[i];
        t.inside = (uint32_t)qx < W && (uint32_t)qy < H;
        const uint32_t cx = qx < 0 ? 0u : (uint32_t)qx >= W ? W - 1u : (uint32_t)qx;
        const uint32_t cy = qy < 0 ? 0u : (uint32_t)qy >= H ? H - 1u : (uint32_t)qy;
        const size_t q = (size_t)cy * W + (size_t)cx;
        const float4 pc = reinterpret_cast<const float4*>(a.prev_color)[q];
        t.c[0] = pc.x; t.c[1] = pc.y; t.c[2] = pc.z; t.c[3] = pc.w;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            t.n[k] = a.prev_normal[3 * q + k];
            t.x[k] = a.prev_point[3 * q + k];
        }
        t.h = a.prev_history[q];
        t.obj = match_object ? a.prev_object[q] : 0u;
    }
    const rttp::Result r = rttp::resolve(a.call, w, X, n, match_object, obj, color, taps);
    store_texel(a, p, r.out, r.history, w.motion[0], w.motion[1]);
}

__global__ void __launch_bounds__(TEMPORAL_THREADS) rt_temporal_kernel(const TemporalArgs a) { temporal_texel<TemporalKind::PLAIN>(a); }
__global__ void __launch_bounds__(TEMPORAL_THREADS) rt_temporal_motion_kernel(const TemporalArgs a) { temporal_texel<TemporalKind::MOVING>(a); }
__global__ void __launch_bounds__(TEMPORAL_THREADS) rt_temporal_deform_kernel(const TemporalArgs a) { temporal_texel<TemporalKind::DEFORMING>(a); }

}  // namespace

hipError_t launch_temporal(const TemporalArgs& a, TemporalKind kind, hipStream_t stream) {
    const uint32_t tiles = ((a.call.width + TILE_W - 1) / TILE_W) * ((a.call.height + TILE_H - 1) / TILE_H);   // (<= 2^31 / 8 + ...: fits)
    const auto kernel = kind == TemporalKind::PLAIN ? rt_temporal_kernel : kind == TemporalKind::MOVING ? rt_temporal_motion_kernel : rt_temporal_deform_kernel;
    hipLaunchKernelGGL(kernel, dim3(tiles), dim3(TEMPORAL_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace rtd
