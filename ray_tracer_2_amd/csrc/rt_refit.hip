// rt_refit.hip -- the device refit of an uploaded BVH (include/rt_abi.h: rt_refit_triangles).
//
// Two phases, so that nothing is written before the host knows the refit can be committed:
//   fit   -- parent links of the selected meshes' wide records, then one launch that folds every leaf child's box from
//            the new triangles and carries the unions up the tree with arrival counters: a record is finished by the
//            last of its own thread and its internal children's threads to arrive.  Boxes go to scratch (one slot per
//            record), and per mesh the root box and the predicates pack_geometry evaluates (contains, the union test,
//            a proper bounding hierarchy) go to a small result table, the only thing the host reads back.
//   write -- the scratch boxes into the wide records, and the triangle intersection / shade records of the range.
// The box rule is csrc/rt_refit.h, shared with the host refit (host/bvh.cpp), and the triangle records are computed with
// the unfused binary32 operations of pack_geometry (this file is compiled with -ffp-contract=off), so the blob ends up
// with the bytes rt_upload_scene gives for the same arrays.
//
// Hand-off between workgroups (cdna_hip_programming Guideline 16, counter form with write-through payload): every box word
// a slot receives is an agent-scope atomic store (sc1, write-through past the XCD's L2), the storing lane waits for its
// stores (s_waitcnt vmcnt(0)) before its agent-scope fetch_add on the slot's counter, and the lane that arrives last reads
// the slot with agent-scope atomic loads.  No lane waits for another, so the launch has no residency requirement.
#include <hip/hip_runtime.h>

#include "rt_refit.h"

namespace rtd {
namespace {

constexpr uint32_t REFIT_THREADS = 256;
constexpr uint32_t NO_PARENT = 0xffffffffu;

__device__ __forceinline__ uint32_t bits_of(float f) { return __float_as_uint(f); }

__device__ __forceinline__ void store_word(unsigned long long* p, float lo, float hi) {
    const unsigned long long w = (unsigned long long)__float_as_uint(lo) | ((unsigned long long)__float_as_uint(hi) << 32);
    __hip_atomic_store(p, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void load_word(unsigned long long* p, float& lo, float& hi) {
    const unsigned long long w = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    lo = __uint_as_float((uint32_t)w);
    hi = __uint_as_float((uint32_t)(w >> 32));
}

__device__ __forceinline__ uint32_t mesh_of_slot(const RefitArgs& a, uint32_t k) {
    uint32_t lo = 0, hi = a.n_meshes;  // the last mesh whose slot0 <= k
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (a.meshes[mid].slot0 <= k) lo = mid;
        else hi = mid;
    }
    return lo;
}

// (idx, count) of a wide record's two children: float bits in q[1].zw and q[3].zw
__device__ __forceinline__ void record_refs(const RefitArgs& a, uint32_t r, uint32_t idx[2], uint32_t cnt[2]) {
    const float4* w = reinterpret_cast<const float4*>(static_cast<const char*>(a.blob) + a.wide_off) + (size_t)r * 4;
    const float4 q1 = w[1], q3 = w[3];
    idx[0] = bits_of(q1.z); cnt[0] = bits_of(q1.w);
    idx[1] = bits_of(q3.z); cnt[1] = bits_of(q3.w);
}

__device__ __forceinline__ bool finite_box(const float lo[3], const float hi[3]) {  // (pack_geometry's finite_box)
    for (int k = 0; k < 3; ++k)
        if (!(lo[k] <= hi[k] && lo[k] - lo[k] == 0.0f && hi[k] - hi[k] == 0.0f)) return false;
    return true;
}

__device__ __forceinline__ bool inside(const float clo[3], const float chi[3], const float lo[3], const float hi[3]) {
    for (int k = 0; k < 3; ++k)
        if (!(clo[k] >= lo[k] && chi[k] <= hi[k])) return false;
    return true;
}

// The box of triangles [idx, idx + cnt) (rt_refit.h); `proper` becomes false unless it is a finite box holding every vertex
// (the hierarchy test of a leaf).  The caller has checked the range against [first, first + n).
__device__ void leaf_box(const RefitArgs& a, uint32_t idx, uint32_t cnt, float lo[3], float hi[3], bool& proper) {
    const float4* t0 = static_cast<const float4*>(a.tris) + (size_t)(idx - a.first) * 6;
    rt_box_empty(lo, hi);
    for (uint32_t j = 0; j < cnt; ++j) {
        const float4 p = t0[6 * j], q = t0[6 * j + 1], r = t0[6 * j + 2];
        const float v1[3] = {p.x, p.y, p.z}, v2[3] = {q.x, q.y, q.z}, v3[3] = {r.x, r.y, r.z};
        rt_box_fold(lo, hi, v1, v2, v3);
    }
    if (!finite_box(lo, hi)) { proper = false; return; }
    for (uint32_t j = 0; j < cnt && proper; ++j)
        for (int v = 0; v < 3; ++v) {
            const float4 p = t0[6 * j + v];
            const float c[3] = {p.x, p.y, p.z};
            if (!inside(c, c, lo, hi)) { proper = false; break; }
        }
}

__global__ void __launch_bounds__(REFIT_THREADS) rt_refit_parent_kernel(RefitArgs a) {
    const uint32_t k = blockIdx.x * REFIT_THREADS + threadIdx.x;
    if (k >= a.slots) return;
    const uint32_t j = mesh_of_slot(a, k);
    const RefitMesh m = a.meshes[j];
    if (m.internal == 0) return;
    uint32_t idx[2], cnt[2];
    record_refs(a, m.wide_base + (k - m.slot0), idx, cnt);
    for (int s = 0; s < 2; ++s) {
        if (cnt[s] != 0) continue;
        // (a child record lies after its parent, inside the mesh's records)
        if (idx[s] <= m.wide_base + (k - m.slot0) || idx[s] >= m.wide_base + m.internal) {
            atomicOr(&a.results[j].flags, REFIT_BAD);
            continue;
        }
        a.parent[m.slot0 + (idx[s] - m.wide_base)] = (k << 1) | (uint32_t)s;
    }
}

__global__ void __launch_bounds__(REFIT_THREADS) rt_refit_fit_kernel(RefitArgs a) {
    uint32_t k = blockIdx.x * REFIT_THREADS + threadIdx.x;
    if (k >= a.slots) return;
    const uint32_t j = mesh_of_slot(a, k);
    const RefitMesh m = a.meshes[j];
    RefitResult& res = a.results[j];
    const uint64_t end = (uint64_t)a.first + a.n;
    bool proper = true;
    if (m.internal == 0) {  // a leaf root: the mesh's one slot
        float lo[3], hi[3];
        if (m.root_idx < a.first || (uint64_t)m.root_idx + m.root_count > end) {
            atomicOr(&res.flags, REFIT_BAD);
            return;
        }
        leaf_box(a, m.root_idx, m.root_count, lo, hi, proper);
        for (int c = 0; c < 3; ++c) { res.lo[c] = lo[c]; res.hi[c] = hi[c]; }
        atomicOr(&res.flags, REFIT_DONE | REFIT_UNIONS | (proper ? 0u : REFIT_IMPROPER));
        return;
    }
    // this slot's leaf children
    uint32_t idx[2], cnt[2];
    record_refs(a, m.wide_base + (k - m.slot0), idx, cnt);
    uint32_t internal_children = 0;
    for (int s = 0; s < 2; ++s) {
        if (cnt[s] == 0) { ++internal_children; continue; }
        if (idx[s] < a.first || (uint64_t)idx[s] + cnt[s] > end) {
            atomicOr(&res.flags, REFIT_BAD);
            return;  // (the root is never finished: the host sees REFIT_DONE missing)
        }
        float lo[3], hi[3];
        leaf_box(a, idx[s], cnt[s], lo, hi, proper);
        unsigned long long* w = a.boxes + (size_t)k * 8 + 4 * s;
        store_word(w + 0, lo[0], hi[0]);
        store_word(w + 1, lo[1], hi[1]);
        store_word(w + 2, lo[2], hi[2]);
    }
    if (internal_children > 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t before = __hip_atomic_fetch_add(a.arrivals + k, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (before != internal_children) {  // (1 + internal_children arrivals: the last one goes on)
            if (!proper) atomicOr(&res.flags, REFIT_IMPROPER);
            return;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // (no instruction: the loads below stay after the add)
    }
    // Slot k is complete: its union goes to its parent's slot, until a parent still waits for another child, or the root.
    for (;;) {
        float ch[2][6];
        unsigned long long* w = a.boxes + (size_t)k * 8;
        for (int s = 0; s < 2; ++s)
            for (int c = 0; c < 3; ++c) load_word(w + 4 * s + c, ch[s][2 * c], ch[s][2 * c + 1]);
        float lo[3], hi[3], alo[3], ahi[3], blo[3], bhi[3];
        for (int c = 0; c < 3; ++c) {
            alo[c] = ch[0][2 * c]; ahi[c] = ch[0][2 * c + 1];
            blo[c] = ch[1][2 * c]; bhi[c] = ch[1][2 * c + 1];
            lo[c] = rt_box_min(alo[c], blo[c]);
            hi[c] = rt_box_max(ahi[c], bhi[c]);
        }
        if (!finite_box(alo, ahi) || !finite_box(blo, bhi) || !inside(alo, ahi, lo, hi) || !inside(blo, bhi, lo, hi)) proper = false;
        if (k == m.slot0) {  // the root: pack_geometry's root predicates, with the same comparisons
            bool contains = true, unions = true;
            for (int c = 0; c < 3; ++c) {
                const float lo_c = alo[c] < blo[c] ? alo[c] : blo[c];
                const float hi_c = ahi[c] > bhi[c] ? ahi[c] : bhi[c];
                if (!(lo[c] <= lo_c && hi[c] >= hi_c)) contains = unions = false;
                if (!(alo[c] <= ahi[c] && blo[c] <= bhi[c])) contains = unions = false;
                if (!(lo[c] - lo[c] == 0.0f && hi[c] - hi[c] == 0.0f)) contains = false;
            }
            if (!finite_box(lo, hi)) proper = false;
            for (int c = 0; c < 3; ++c) { res.lo[c] = lo[c]; res.hi[c] = hi[c]; }
            atomicOr(&res.flags, REFIT_DONE | (contains ? REFIT_CONTAINS : 0u) | (unions ? REFIT_UNIONS : 0u) |
                                 (proper ? 0u : REFIT_IMPROPER));
            return;
        }
        const uint32_t p = a.parent[k];
        if (p == NO_PARENT || (p >> 1) < m.slot0 || (p >> 1) >= k) {
            atomicOr(&res.flags, REFIT_BAD);
            return;
        }
        const uint32_t pk = p >> 1, side = p & 1u;
        unsigned long long* pw = a.boxes + (size_t)pk * 8 + 4 * side;
        store_word(pw + 0, lo[0], hi[0]);
        store_word(pw + 1, lo[1], hi[1]);
        store_word(pw + 2, lo[2], hi[2]);
        uint32_t pidx[2], pcnt[2];
        record_refs(a, m.wide_base + (pk - m.slot0), pidx, pcnt);
        const uint32_t waits = (pcnt[0] == 0 ? 1u : 0u) + (pcnt[1] == 0 ? 1u : 0u);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t before = __hip_atomic_fetch_add(a.arrivals + pk, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (before != waits) break;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        k = pk;
    }
    if (!proper) atomicOr(&res.flags, REFIT_IMPROPER);
}

__global__ void __launch_bounds__(REFIT_THREADS) rt_refit_records_kernel(RefitArgs a) {
    const uint32_t k = blockIdx.x * REFIT_THREADS + threadIdx.x;
    if (k >= a.slots) return;
    const RefitMesh m = a.meshes[mesh_of_slot(a, k)];
    if (m.internal == 0) return;
    float* w = reinterpret_cast<float*>(static_cast<char*>(a.blob) + a.wide_off) + (size_t)(m.wide_base + (k - m.slot0)) * 16;
    const unsigned long long* b = a.boxes + (size_t)k * 8;
    for (int s = 0; s < 2; ++s) {  // (lo0, hi0, lo1, hi1) | (lo2, hi2, idx, count): the references stay
        reinterpret_cast<unsigned long long*>(w + 8 * s)[0] = b[4 * s + 0];
        reinterpret_cast<unsigned long long*>(w + 8 * s)[1] = b[4 * s + 1];
        reinterpret_cast<unsigned long long*>(w + 8 * s)[2] = b[4 * s + 2];
    }
}

// pack_geometry's triangle re-layout (rt_scene_format.h): intersection record (v1, n.x), (ab, n.y), (ac, n.z); shade record
// (n1, uv10), (n2, uv11), (n3, uv20), (uv21, uv30, uv31, 0).  The subtractions and the cross product are wgsl:261-263.
__global__ void __launch_bounds__(REFIT_THREADS) rt_refit_triangles_kernel(RefitArgs a) {
    const uint32_t t = blockIdx.x * REFIT_THREADS + threadIdx.x;
    if (t >= a.n) return;
    const float4* p = static_cast<const float4*>(a.tris) + (size_t)t * 6;
    const float4 q0 = p[0], q1 = p[1], q2 = p[2], q3 = p[3], q4 = p[4], q5 = p[5];
    const float abx = q1.x - q0.x, aby = q1.y - q0.y, abz = q1.z - q0.z;
    const float acx = q2.x - q0.x, acy = q2.y - q0.y, acz = q2.z - q0.z;
    const float nx = aby * acz - abz * acy;
    const float ny = abz * acx - abx * acz;
    const float nz = abx * acy - aby * acx;
    char* blob = static_cast<char*>(a.blob);
    float4* ti = reinterpret_cast<float4*>(blob + a.tri_off) + (size_t)(a.first + t) * 3;
    ti[0] = make_float4(q0.x, q0.y, q0.z, nx);
    ti[1] = make_float4(abx, aby, abz, ny);
    ti[2] = make_float4(acx, acy, acz, nz);
    float4* ts = reinterpret_cast<float4*>(blob + a.shade_off) + (size_t)(a.first + t) * 4;
    ts[0] = make_float4(q3.x, q3.y, q3.z, q0.w);
    ts[1] = make_float4(q4.x, q4.y, q4.z, q1.w);
    ts[2] = make_float4(q5.x, q5.y, q5.z, q2.w);
    ts[3] = make_float4(q3.w, q4.w, q5.w, 0.0f);
}

uint32_t blocks_for(uint32_t n) { return (n + REFIT_THREADS - 1) / REFIT_THREADS; }

}  // namespace

// Phase 1: reads the blob's wide-record references and the triangles, writes only the scratch of `a`.
hipError_t launch_refit_fit(const RefitArgs& a, hipStream_t stream) {
    if (a.slots == 0) return hipSuccess;
    hipLaunchKernelGGL(rt_refit_parent_kernel, dim3(blocks_for(a.slots)), dim3(REFIT_THREADS), 0, stream, a);
    hipLaunchKernelGGL(rt_refit_fit_kernel, dim3(blocks_for(a.slots)), dim3(REFIT_THREADS), 0, stream, a);
    return hipGetLastError();
}

// Phase 2: the boxes into a.blob's wide records, the triangles into its triangle records.
hipError_t launch_refit_write(const RefitArgs& a, hipStream_t stream) {
    if (a.slots) hipLaunchKernelGGL(rt_refit_records_kernel, dim3(blocks_for(a.slots)), dim3(REFIT_THREADS), 0, stream, a);
    if (a.n) hipLaunchKernelGGL(rt_refit_triangles_kernel, dim3(blocks_for(a.n)), dim3(REFIT_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace rtd
