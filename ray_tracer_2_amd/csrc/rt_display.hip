// rt_display.hip -- the device kernels of the display pass and the exposure meter (include/rt_abi.h: rt_display,
// rt_auto_exposure, rt_snapshot_display).
//
// rt_display_kernel: bound by its bytes, 16 read and 4 written per texel.  A workgroup of 256 lanes takes ITEMS
// consecutive chunks of 256 texels; a lane takes texel `lane` of each chunk, so that every load instruction of a wave is
// 1 KiB of consecutive bytes (one float4 a lane) and every store 256 (one word a lane: `out` is only 4-byte aligned, and a
// row flip or a width that is no multiple of four leaves no wider unit that always holds).  The ITEMS loads are issued before
// the first texel is encoded.  The sRGB search reads LDS: the 259 thresholds and the 417 bytes of the coarse index, copied
// by the workgroup once (2 KiB; the copy is why a workgroup takes more than one chunk) -- per channel one byte read for the
// bucket's base and RT_SRGB_ENCODE_STEPS = 3 independent threshold reads, against the eight dependent reads of a binary
// search.  The exposure scale is one float read by every lane (a uniform load).
//
// rt_exposure_count_kernel: the luminance histogram.  The same map of lanes to texels; each of the workgroup's four
// waves keeps 256 counters of its own in LDS.  Before the LDS atomic a wave folds the lanes that share the bin of its first
// counted lane into one add of their number (ballot), so that a frame -- or a flat region -- in one bin costs one atomic a
// wave instead of 64 serialised ones; the other lanes add 1 each.  After a barrier lane b sums the four counters of bin b
// and adds a non-zero sum to the global bin with one integer atomic: the result does not depend on arrival order, and
// no workgroup waits on another.  rt_exposure_finish_kernel, one wave, behind it in stream order: lane l takes bins 4 l ..
// 4 l + 3, a wave scan gives each bin's first rank, the trimmed sums are reduced by xor shuffles, lane 0 writes the float.
// The global bins are the handle's scratch, zeroed in stream order before the count.
// The per-texel arithmetic is csrc/rt_display.h, shared with the host restatement (host/display.cpp); this file is
// compiled with -ffp-contract=off, so the results are the host's bit for bit.
//
// Bounds: w * h <= 2^31 - 1 (the entry points check), a chunk's first texel is formed in 64 bits, and a lane whose texel is
// >= w * h makes no access to a plane (in the count kernel it stays for the wave's ballots, with bin -1).  The output index
// is out_row(y) * w + x < w * h.  LDS: thresholds read at base + j <= 255 + 3 < 259, the index at a bucket < 417
// (rtdp::srgb_byte clamps its argument into [0, 1] first); the counters at a bin in [0, 255].
#include <hip/hip_runtime.h>

#include "rt_display.h"
#include "rt_display_api.h"

namespace rtd {
namespace {

// What tools/display_bench.py measured against each other, as built with
// build_product(extra_flags=...): texels a lane of the display kernel takes, and the fold before the LDS atomic.
#ifndef RT_DISPLAY_ITEMS
#define RT_DISPLAY_ITEMS 4
#endif
#ifndef RT_EXPOSURE_FOLD
#define RT_EXPOSURE_FOLD 1
#endif
constexpr uint32_t THREADS = 256, ITEMS = RT_DISPLAY_ITEMS, COUNT_ITEMS = 8, WAVES = THREADS / 64;

__device__ const float ENCODE_T[rtdp::T_COUNT] = {RT_SRGB_ENCODE_T_VALUES};
__device__ const uint8_t ENCODE_BASE[rtdp::BUCKETS] = {RT_SRGB_ENCODE_BASE_VALUES};

#define RT_GLOBAL(T, p) ((__attribute__((address_space(1))) T*)(void*)(p))

__global__ void __launch_bounds__(THREADS) rt_display_kernel(const DisplayArgs a) {
    __shared__ float lds_t[rtdp::T_COUNT];
    __shared__ uint8_t lds_base[rtdp::BUCKETS];
    const rtdp::Call& c = a.call;
    const bool srgb = c.transfer == rtdp::TRANSFER_SRGB;   // (uniform)
    if (srgb) {
        for (uint32_t i = threadIdx.x; i < rtdp::T_COUNT; i += THREADS) lds_t[i] = ENCODE_T[i];
        for (uint32_t i = threadIdx.x; i < rtdp::BUCKETS; i += THREADS) lds_base[i] = ENCODE_BASE[i];
        __syncthreads();
    }
    const uint64_t texels = (uint64_t)c.width * c.height;
    const uint64_t first = (uint64_t)blockIdx.x * (THREADS * ITEMS) + threadIdx.x;
    const float e = rtdp::exposure_of(c.exposure, a.exposure_scale != nullptr, a.exposure_scale ? *a.exposure_scale : 1.0f);
    float4 v[ITEMS];
#pragma unroll
    for (uint32_t i = 0; i < ITEMS; ++i) {
        const uint64_t p = first + (uint64_t)i * THREADS;
        if (p < texels) v[i] = reinterpret_cast<const float4*>(a.color)[p];
    }
#pragma unroll
    for (uint32_t i = 0; i < ITEMS; ++i) {
        const uint64_t p = first + (uint64_t)i * THREADS;
        if (p >= texels) continue;
        const float rgba[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
        const uint32_t word = rtdp::texel_word(c, rgba, e, lds_t, lds_base);
        uint64_t q = p;
        if (c.layout & rtdp::LAYOUT_TOP_FIRST) {
            const uint32_t y = (uint32_t)(p / c.width), x = (uint32_t)(p - (uint64_t)y * c.width);
            q = (uint64_t)rtdp::out_row(c, y) * c.width + x;
        }
        // written once and read by nobody in the launch: a streaming store
        __builtin_nontemporal_store(word, RT_GLOBAL(uint32_t, a.out + q));
    }
}

__global__ void __launch_bounds__(THREADS) rt_exposure_count_kernel(const AutoExposureArgs a) {
    __shared__ uint32_t counts[WAVES][rtdp::BINS];
    for (uint32_t i = threadIdx.x; i < WAVES * rtdp::BINS; i += THREADS) (&counts[0][0])[i] = 0u;
    __syncthreads();
    const uint64_t texels = (uint64_t)a.call.width * a.call.height;
    const uint64_t first = (uint64_t)blockIdx.x * (THREADS * COUNT_ITEMS) + threadIdx.x;
    uint32_t* mine = counts[threadIdx.x / 64u];
    const uint32_t lane = threadIdx.x & 63u;
    float4 v[COUNT_ITEMS];
#pragma unroll
    for (uint32_t i = 0; i < COUNT_ITEMS; ++i) {
        const uint64_t p = first + (uint64_t)i * THREADS;
        v[i] = p < texels ? reinterpret_cast<const float4*>(a.color)[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);   // (black: not counted)
    }
#pragma unroll
    for (uint32_t i = 0; i < COUNT_ITEMS; ++i) {
        const int32_t bin = rtdp::luminance_bin(v[i].x, v[i].y, v[i].z);
#if RT_EXPOSURE_FOLD
        const uint64_t counted = __ballot(bin >= 0);
        if (counted == 0ull) continue;   // (uniform in the wave)
        const uint32_t leader = (uint32_t)__ffsll((unsigned long long)counted) - 1u;
        const int32_t lead_bin = __shfl(bin, (int)leader);
        const uint64_t same = __ballot(bin == lead_bin);
        if (lane == leader)
            atomicAdd(&mine[lead_bin], (uint32_t)__popcll(same));
        else if (bin >= 0 && bin != lead_bin)
            atomicAdd(&mine[bin], 1u);
#else
        (void)lane;
        if (bin >= 0) atomicAdd(&mine[bin], 1u);
#endif
    }
    __syncthreads();
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t w = 0; w < WAVES; ++w) sum += counts[w][threadIdx.x];
    if (sum != 0u) atomicAdd(a.bins + threadIdx.x, sum);
}

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int mask) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, mask), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), mask);
    return ((uint64_t)hi << 32) | lo;
}

__global__ void __launch_bounds__(64) rt_exposure_finish_kernel(const AutoExposureArgs a) {
    const uint32_t lane = threadIdx.x;
    const uint4 n = reinterpret_cast<const uint4*>(a.bins)[lane];
    const uint32_t own[4] = {n.x, n.y, n.z, n.w};
    // the ranks before this lane's bins: an inclusive scan of the lanes' totals (all <= 2^31 - 1), minus its own
    const uint32_t total = (n.x + n.y) + (n.z + n.w);
    uint32_t scan = total;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)scan, d);
        if (lane >= (uint32_t)d) scan += up;
    }
    const uint64_t N = (uint32_t)__shfl((int)scan, 63);
    const uint32_t lo = (uint32_t)(N * a.call.low_permille / 1000u), hi = (uint32_t)(N * a.call.high_permille / 1000u);
    uint32_t start = scan - total, kept_n = 0;
    uint64_t kept_sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t k = rtdp::kept(start, own[j], lo, hi);
        kept_n += k;
        kept_sum += (uint64_t)k * (4u * lane + j);
        start += own[j];
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        kept_n += (uint32_t)__shfl_xor((int)kept_n, m);
        kept_sum += shfl_xor_u64(kept_sum, m);
    }
    if (a.histogram) {   // (4-byte aligned: a word at a time)
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) a.histogram[4u * lane + j] = own[j];
    }
    if (lane == 0u) {
        const float prev = a.prev_scale ? *a.prev_scale : 0.0f;
        *a.scale = rtdp::meter_scale(a.call, kept_n, kept_sum, a.prev_scale != nullptr, prev);
    }
}

}  // namespace

hipError_t launch_display(const DisplayArgs& a, hipStream_t stream) {
    const uint64_t texels = (uint64_t)a.call.width * a.call.height;
    const uint32_t blocks = (uint32_t)((texels + THREADS * ITEMS - 1) / (THREADS * ITEMS));   // (<= 2^21)
    hipLaunchKernelGGL(rt_display_kernel, dim3(blocks), dim3(THREADS), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_auto_exposure(const AutoExposureArgs& a, hipStream_t stream) {
    if (const hipError_t e = hipMemsetAsync(a.bins, 0, rtdp::BINS * sizeof(uint32_t), stream); e != hipSuccess) return e;
    const uint64_t texels = (uint64_t)a.call.width * a.call.height;
    const uint32_t blocks = (uint32_t)((texels + THREADS * COUNT_ITEMS - 1) / (THREADS * COUNT_ITEMS));
    hipLaunchKernelGGL(rt_exposure_count_kernel, dim3(blocks), dim3(THREADS), 0, stream, a);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(rt_exposure_finish_kernel, dim3(1), dim3(64), 0, stream, a);
    return hipGetLastError();
}

}  // namespace rtd
