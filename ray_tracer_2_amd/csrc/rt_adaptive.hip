// rt_adaptive.hip -- the device kernels of adaptive sampling (include/rt_abi.h: rt_adaptive_plan, rt_adaptive_merge;
// DESIGN.md section 2.16).
//
// The plan is two reduce-then-scan chains over blocks of ADAPTIVE_BLOCK = 1024 texels (256 lanes, four consecutive texels
// each), a u64 one for q and a u32 one for n.  No workgroup ever waits on another: the only ordering between workgroups is
// the boundary between two kernels of the stream.
//   max        -- the maximum of variance_key: a wave reduction, then one vector atomicMax per wave on a word the launch
//                 zeroes first.
//   q sums     -- a block's sum of q (below 2^30: u32 inside a block, u64 outside).
//   scan<u64>  -- ONE workgroup walks the block sums 1024 at a time with a running carry: exclusive scan and total (S).
//   counts     -- q again, its scan inside the block on top of the block's offset, F at each texel's two ends
//                 (rtad::mul_div_floor, shared with the host; a lane carries F from one of its texels to the next and skips
//                 texels with q = 0), n(p) -> counts; the block's sum of n and its two tallies.
//   scan<u32>  -- the same one-workgroup walk over the sums of n -> offsets of the blocks, totals.
//   downsweep  -- offsets(p); then the block's records, ONE RECORD PER LANE whatever texel it belongs to: a lane finds its
//                 record's texel by a binary search of the block's 1024 offsets in LDS, so a wave stores 64 consecutive
//                 records (2 KB) and a texel with many samples is spread over the block.  Then the tail, grid-strided.
// 1025 texels (one more than a block) reach the second block of every per-block kernel and the second entry of the block
// scans; 1025 x 1031 texels make 1033 block sums and reach the second round -- the carry -- of the one-workgroup scans,
// the only other level there is.
// The merge is one lane per texel over rtad::Merge, the host's code.  This file is compiled with -ffp-contract=off.
//
// Bounds.  Texel indices are < 2^31 (the entry point checks) and every address is formed in 64 bits.  A lane whose texel is
// outside the frame takes part in the scans with q = n = 0 and touches no plane.  A record index is checked against
// `budget` before its store although the sum of n cannot pass it, and the merge stops a texel's samples at `budget`.
#include <hip/hip_runtime.h>

#include "rt_adaptive.h"
#include "rt_adaptive_api.h"

namespace rtd {
namespace {

constexpr uint32_t THREADS = 256, ITEMS = 4, WAVES = THREADS / 64;
static_assert(THREADS * ITEMS == ADAPTIVE_BLOCK, "a block of the scans");
constexpr uint32_t SCAN_THREADS = 1024, SCAN_WAVES = SCAN_THREADS / 64;

// the handle's scratch (rt_adaptive_api.h)
struct Scratch {
    uint32_t* max_key;   // header word 0
    uint64_t* S;         // header bytes 8 .. 15
    uint64_t *qsum, *qoff;
    uint32_t *nsum, *noff, *tally;   // tally: texels above min_samples | clamped ones << 16, per block
};
__host__ __device__ inline Scratch scratch_of(void* base, size_t blocks) {
    uint8_t* b = static_cast<uint8_t*>(base);
    uint8_t* a = b + ADAPTIVE_HEADER_BYTES;
    Scratch s;
    s.max_key = reinterpret_cast<uint32_t*>(b);
    s.S = reinterpret_cast<uint64_t*>(b + 8);
    s.qsum = reinterpret_cast<uint64_t*>(a);
    s.qoff = reinterpret_cast<uint64_t*>(a + 8 * blocks);
    s.nsum = reinterpret_cast<uint32_t*>(a + 16 * blocks);
    s.noff = reinterpret_cast<uint32_t*>(a + 20 * blocks);
    s.tally = reinterpret_cast<uint32_t*>(a + 24 * blocks);   // (28 of the 32 bytes per block are used)
    return s;
}

__device__ __forceinline__ uint32_t shfl_up_(uint32_t v, uint32_t d) { return (uint32_t)__shfl_up((int)v, d, 64); }
__device__ __forceinline__ uint64_t shfl_up_(uint64_t v, uint32_t d) {
    const uint32_t lo = shfl_up_((uint32_t)v, d), hi = shfl_up_((uint32_t)(v >> 32), d);
    return ((uint64_t)hi << 32) | lo;
}

// inclusive scan over the 64 lanes of a wave
template <class T>
__device__ __forceinline__ T wave_inclusive(T v) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const T o = shfl_up_(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

// Exclusive scan of one value per lane over a workgroup of NW waves; total: the workgroup's sum.  part: NW words of LDS that
// nothing else uses until the next __syncthreads() after the call.
template <class T, uint32_t NW>
__device__ __forceinline__ T block_exclusive(T v, T* part, T& total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const T inc = wave_inclusive(v);
    if (lane == 63u) part[wave] = inc;
    __syncthreads();
    T base = 0, sum = 0;
#pragma unroll
    for (uint32_t w = 0; w < NW; ++w) {
        const T t = part[w];
        base += w < wave ? t : (T)0;
        sum += t;
    }
    total = sum;
    return base + inc - v;
}

// the four variances of a lane (0 outside the frame: variance_key and quantise give 0 for it)
__device__ __forceinline__ void load_variance(const float* variance, size_t texels, size_t first, float v[ITEMS]) {
#pragma unroll
    for (uint32_t i = 0; i < ITEMS; ++i) v[i] = first + i < texels ? variance[first + i] : 0.0f;
}

__global__ void __launch_bounds__(THREADS) rt_adaptive_max_kernel(const AdaptivePlanArgs a, const size_t texels, const size_t blocks) {
    const size_t first = (size_t)blockIdx.x * ADAPTIVE_BLOCK + (size_t)threadIdx.x * ITEMS;
    float v[ITEMS];
    load_variance(a.variance, texels, first, v);
    uint32_t m = 0u;
#pragma unroll
    for (uint32_t i = 0; i < ITEMS; ++i) {
        const uint32_t k = rtad::variance_key(v[i]);
        m = k > m ? k : m;
    }
#pragma unroll
    for (uint32_t d = 32; d >= 1; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)m, (int)d, 64);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63u) == 0u && m != 0u) atomicMax(scratch_of(a.scratch, blocks).max_key, m);
}

__global__ void __launch_bounds__(THREADS) rt_adaptive_qsum_kernel(const AdaptivePlanArgs a, const size_t texels, const size_t blocks) {
    __shared__ uint32_t part[WAVES];
    const Scratch s = scratch_of(a.scratch, blocks);
    const uint32_t max_key = *s.max_key;
    const size_t first = (size_t)blockIdx.x * ADAPTIVE_BLOCK + (size_t)threadIdx.x * ITEMS;
    float v[ITEMS];
    load_variance(a.variance, texels, first, v);
    uint32_t sum = 0u;
#pragma unroll
    for (uint32_t i = 0; i < ITEMS; ++i) sum += rtad::quantise(v[i], max_key);
    uint32_t total;
    (void)block_exclusive<uint32_t, WAVES>(sum, part, total);   // (<= 1024 * 2^20)
    if (threadIdx.x == 0u) s.qsum[blockIdx.x] = total;
}

// One workgroup: out = the exclusive scan of in[0 .. n), *total_out its sum.  TOTALS: the scan of the sums of n, which also
// adds up the blocks' tallies and writes the plan's totals.
template <class T, bool TOTALS>
__global__ void __launch_bounds__(SCAN_THREADS) rt_adaptive_scan_kernel(const T* __restrict__ in, T* __restrict__ out, const size_t n, T* total_out,
                                                                        const uint32_t* __restrict__ tally, uint32_t* totals) {
    __shared__ T part[SCAN_WAVES];
    __shared__ uint32_t tallies[2];
    T carry = 0;
    for (size_t i0 = 0; i0 < n; i0 += SCAN_THREADS) {
        const size_t i = i0 + threadIdx.x;
        const T v = i < n ? in[i] : (T)0;
        T total;
        const T ex = block_exclusive<T, SCAN_WAVES>(v, part, total);
        if (i < n) out[i] = carry + ex;
        carry += total;
        __syncthreads();   // (part is written again by the next round)
    }
    if (threadIdx.x == 0u && total_out) *total_out = carry;
    if constexpr (TOTALS) {
        if (threadIdx.x < 2u) tallies[threadIdx.x] = 0u;
        __syncthreads();
        uint32_t above = 0u, clamped = 0u;
        for (size_t i = threadIdx.x; i < n; i += SCAN_THREADS) {
            const uint32_t t = tally[i];
            above += t & 0xffffu;
            clamped += t >> 16;
        }
        if (above) atomicAdd(&tallies[0], above);       // (LDS atomics: at most 2^31 - 1 texels in all)
        if (clamped) atomicAdd(&tallies[1], clamped);
        __syncthreads();
        if (threadIdx.x == 0u) {
            totals[0] = (uint32_t)carry;
            totals[1] = tallies[0];
            totals[2] = tallies[1];
            totals[3] = 0u;
        }
    }
}

__global__ void __launch_bounds__(THREADS) rt_adaptive_counts_kernel(const AdaptivePlanArgs a, const size_t texels, const size_t blocks) {
    __shared__ uint32_t part_q[WAVES], part_n[WAVES], part_t[WAVES];
    const Scratch s = scratch_of(a.scratch, blocks);
    const uint32_t max_key = *s.max_key;
    const uint64_t S = *s.S, R = (uint64_t)a.budget - (uint64_t)a.min_samples * texels;
    const size_t first = (size_t)blockIdx.x * ADAPTIVE_BLOCK + (size_t)threadIdx.x * ITEMS;
    float v[ITEMS];
    load_variance(a.variance, texels, first, v);
    uint32_t q[ITEMS], sum = 0u;
#pragma unroll
    for (uint32_t i = 0; i < ITEMS; ++i) {
        q[i] = rtad::quantise(v[i], max_key);
        sum += q[i];
    }
    uint32_t unused;
    uint64_t C = s.qoff[blockIdx.x] + block_exclusive<uint32_t, WAVES>(sum, part_q, unused);
    // (S = 0 means every q is 0: sum is 0 everywhere and F is never evaluated)
    uint64_t f_begin = sum != 0u ? rtad::mul_div_floor(C, R, S) : 0u;
    uint32_t n_sum = 0u, tally = 0u;
#pragma unroll
    for (uint32_t i = 0; i < ITEMS; ++i) {
        C += q[i];
        const uint64_t f_end = q[i] != 0u ? rtad::mul_div_floor(C, R, S) : f_begin;
        bool over;
        const uint32_t n = rtad::samples_of(f_begin, f_end, a.min_samples, a.max_samples, over);
        f_begin = f_end;
        if (first + i < texels) {
            a.counts[first + i] = n;
            n_sum += n;
            tally += (n > a.min_samples ? 1u : 0u) + (over ? 0x10000u : 0u);
        }
    }
    uint32_t block_n, block_t;
    (void)block_exclusive<uint32_t, WAVES>(n_sum, part_n, block_n);   // (<= 1024 * 65535)
    (void)block_exclusive<uint32_t, WAVES>(tally, part_t, block_t);   // (two fields of at most 1024 each)
    if (threadIdx.x == 0u) {
        s.nsum[blockIdx.x] = block_n;
        s.tally[blockIdx.x] = block_t;
    }
}

typedef float v4f __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(THREADS) rt_adaptive_downsweep_kernel(const AdaptivePlanArgs a, const size_t texels, const size_t blocks) {
    __shared__ uint32_t part[WAVES];
    __shared__ uint32_t begin[ADAPTIVE_BLOCK];   // the exclusive scan of n inside the block
    const Scratch s = scratch_of(a.scratch, blocks);
    const size_t block_first = (size_t)blockIdx.x * ADAPTIVE_BLOCK;
    const size_t first = block_first + (size_t)threadIdx.x * ITEMS;
    uint32_t n[ITEMS], sum = 0u;
#pragma unroll
    for (uint32_t i = 0; i < ITEMS; ++i) {
        n[i] = first + i < texels ? a.counts[first + i] : 0u;
        sum += n[i];
    }
    uint32_t block_n;
    uint32_t ex = block_exclusive<uint32_t, WAVES>(sum, part, block_n);
    const uint32_t block_off = s.noff[blockIdx.x];
#pragma unroll
    for (uint32_t i = 0; i < ITEMS; ++i) {
        begin[threadIdx.x * ITEMS + i] = ex;
        if (first + i < texels) a.offsets[first + i] = block_off + ex;
        ex += n[i];
    }
    __syncthreads();
    v4f* rays = static_cast<v4f*>(a.rays);
    for (uint32_t r = threadIdx.x; r < block_n; r += THREADS) {
        // the last texel t of the block with begin[t] <= r: the one whose records hold r (texels without samples before it
        // share its begin and lose to it)
        uint32_t t = 0u;
#pragma unroll
        for (uint32_t step = ADAPTIVE_BLOCK / 2; step >= 1u; step >>= 1)
            if (begin[t + step] <= r) t += step;
        const size_t p = block_first + t;   // (inside the frame: a texel outside it has no samples)
        const size_t record = (size_t)block_off + r;
        if (record >= (size_t)a.budget) continue;
        const uint32_t seed = rtad::sample_seed((uint32_t)p, a.first_frame, r - begin[t]);
        rays[2 * record] = v4f{a.origin[0], a.origin[1], a.origin[2], __uint_as_float(seed)};
        rays[2 * record + 1] = v4f{a.dir[3 * p], a.dir[3 * p + 1], a.dir[3 * p + 2], 0.0f};
    }
    // the tail: records [totals[0], budget) are zeros
    const size_t stride = (size_t)gridDim.x * THREADS;
    for (size_t record = (size_t)a.totals[0] + (size_t)blockIdx.x * THREADS + threadIdx.x; record < (size_t)a.budget; record += stride) {
        rays[2 * record] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
        rays[2 * record + 1] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
    }
}

__global__ void __launch_bounds__(THREADS) rt_adaptive_merge_kernel(const AdaptiveMergeArgs a) {
    const size_t p = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (p >= (size_t)a.width * a.height) return;
    const float4 c4 = reinterpret_cast<const float4*>(a.color)[p];
    const float color[4] = {c4.x, c4.y, c4.z, c4.w};
    float moments[4] = {0.0f, 0.0f, 0.0f, 0.0f}, al[3] = {1.0f, 1.0f, 1.0f};
    if (a.moments) {
        const float4 m = reinterpret_cast<const float4*>(a.moments)[p];
        moments[0] = m.x; moments[1] = m.y; moments[2] = m.z; moments[3] = m.w;
    }
    if (a.albedo) {
        const float4 v = reinterpret_cast<const float4*>(a.albedo)[p];
        al[0] = rtdn::albedo_floor(v.x); al[1] = rtdn::albedo_floor(v.y); al[2] = rtdn::albedo_floor(v.z);
    }
    rtad::Merge t;
    t.start(color, a.history[p], moments);
    const uint32_t n = a.counts[p];
    const uint64_t first = a.offsets[p];
    const bool with_moments = a.moments != nullptr;
    for (uint32_t k = 0; k < n && first + k < (uint64_t)a.budget; ++k) {
        const float4 s = reinterpret_cast<const float4*>(a.radiance)[first + k];
        const float c[4] = {s.x, s.y, s.z, s.w};
        t.sample(c, al, a.max_history, with_moments);
    }
    reinterpret_cast<float4*>(a.out)[p] = make_float4(t.acc[0], t.acc[1], t.acc[2], t.acc[3]);
    a.out_history[p] = t.hl;
    if (a.out_moments) reinterpret_cast<float4*>(a.out_moments)[p] = make_float4(t.m[0], t.m[1], t.m[2], t.m[3]);
}

}  // namespace

hipError_t launch_adaptive_plan(const AdaptivePlanArgs& a, hipStream_t stream) {
    const size_t texels = (size_t)a.width * a.height, blocks = adaptive_blocks(texels);   // (blocks <= 2^21)
    const Scratch s = scratch_of(a.scratch, blocks);
    if (const hipError_t e = hipMemsetAsync(a.scratch, 0, ADAPTIVE_HEADER_BYTES, stream); e != hipSuccess) return e;
    const dim3 grid((uint32_t)blocks), block(THREADS);
    hipLaunchKernelGGL(rt_adaptive_max_kernel, grid, block, 0, stream, a, texels, blocks);
    hipLaunchKernelGGL(rt_adaptive_qsum_kernel, grid, block, 0, stream, a, texels, blocks);
    hipLaunchKernelGGL((rt_adaptive_scan_kernel<uint64_t, false>), dim3(1), dim3(SCAN_THREADS), 0, stream, s.qsum, s.qoff, blocks, s.S,
                       (const uint32_t*)nullptr, (uint32_t*)nullptr);
    hipLaunchKernelGGL(rt_adaptive_counts_kernel, grid, block, 0, stream, a, texels, blocks);
    hipLaunchKernelGGL((rt_adaptive_scan_kernel<uint32_t, true>), dim3(1), dim3(SCAN_THREADS), 0, stream, s.nsum, s.noff, blocks, (uint32_t*)nullptr,
                       s.tally, a.totals);
    hipLaunchKernelGGL(rt_adaptive_downsweep_kernel, grid, block, 0, stream, a, texels, blocks);
    return hipGetLastError();
}

hipError_t launch_adaptive_merge(const AdaptiveMergeArgs& a, hipStream_t stream) {
    const size_t texels = (size_t)a.width * a.height;
    hipLaunchKernelGGL(rt_adaptive_merge_kernel, dim3((uint32_t)((texels + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace rtd
