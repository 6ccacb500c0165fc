// rt_refit.h -- the box rule of a BVH refit (include/rt_abi.h: rt_refit_bvh, rt_refit_triangles), shared by the host refit
// (host/bvh.cpp) and the device refit (rt_refit.hip) so that both produce the same bits.
//
// min / max are written out as comparisons and selects: neither libm fmin (whose sign of a zero result differs between
// compilers) nor v_min_f32 (whose NaN and signed-zero behaviour depends on the mode bits) is used.
//   - ordered operands: the smaller (larger) one;
//   - equal operands: for zeros of both signs, -0 for the min and +0 for the max; equal non-zero values have equal bits;
//   - a NaN operand: the other operand (a NaN only when both are NaN).
// A leaf's box is a fold over its triangles in array order, starting from (+FLT_MAX, -FLT_MAX) as the builder's
// fit_bounds does; each triangle contributes rt_box_min(v1, rt_box_min(v2, v3)) and the matching max, per axis.  An
// internal node's box is rt_box_min / rt_box_max of its two children's, element by element.  Since the fold starts from
// finite values and a NaN operand yields the other one, no box ever holds a NaN.
#ifndef RT_REFIT_H
#define RT_REFIT_H

#include <cfloat>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RT_REFIT_HD __host__ __device__
#else
#define RT_REFIT_HD
#endif

RT_REFIT_HD inline float rt_box_min(float a, float b) {
    if (a < b) return a;
    if (b < a) return b;
    if (a == b) return __builtin_signbit(a) ? a : b;  // (-0 over +0)
    return a != a ? b : a;
}

RT_REFIT_HD inline float rt_box_max(float a, float b) {
    if (a > b) return a;
    if (b > a) return b;
    if (a == b) return __builtin_signbit(a) ? b : a;  // (+0 over -0)
    return a != a ? b : a;
}

// One triangle's contribution to a leaf box fold (lo / hi hold the box so far).
RT_REFIT_HD inline void rt_box_fold(float lo[3], float hi[3], const float v1[3], const float v2[3], const float v3[3]) {
    for (int k = 0; k < 3; ++k) {
        lo[k] = rt_box_min(lo[k], rt_box_min(v1[k], rt_box_min(v2[k], v3[k])));
        hi[k] = rt_box_max(hi[k], rt_box_max(v1[k], rt_box_max(v2[k], v3[k])));
    }
}

RT_REFIT_HD inline void rt_box_empty(float lo[3], float hi[3]) {
    for (int k = 0; k < 3; ++k) {
        lo[k] = FLT_MAX;
        hi[k] = -FLT_MAX;
    }
}

// ---- the device refit's tables (rt_api.hip: rt_refit_triangles builds them, rt_refit.hip's kernels read them) ----
// Every selected mesh has slots: one per wide BVH record (a record holds the boxes of an internal node's two children), or
// one for a mesh whose root is a leaf.  Slot k of mesh j is record wide_base + (k - slot0); the root record is slot0.
namespace rtd {
struct RefitMesh {  // 32 B, in increasing slot0
    uint32_t slot0, wide_base, internal;  // internal == 0: the root is a leaf of root_count triangles from root_idx
    uint32_t root_idx, root_count, _p[3];
};
enum : uint32_t {
    REFIT_DONE = 1,       // the root box is in
    REFIT_CONTAINS = 2,   // MeshGeom::contains
    REFIT_UNIONS = 4,     // the mesh's part of SceneGeom::roots_are_unions
    REFIT_IMPROPER = 8,   // not a proper bounding hierarchy (MeshGeom::hierarchy_ok is false)
    REFIT_BAD = 16,       // a record's reference out of the mesh's ranges (the upload validated them: never expected)
};
struct RefitResult {  // 32 B per selected mesh: the one thing read back
    float lo[3], hi[3];
    uint32_t flags, _p;
};
struct RefitArgs {
    void* blob;                       // the blob to write (the fit kernels only read its wide records' references)
    uint32_t wide_off, tri_off, shade_off;
    const void* tris;                 // n rt_packed_triangle records (device memory), triangle first + t at tris[t]
    uint32_t first, n;
    const RefitMesh* meshes;
    uint32_t n_meshes, slots;
    uint32_t* parent;                 // per slot: (parent slot << 1) | side, ~0 for a root (memset 0xff)
    uint32_t* arrivals;               // per slot: arrivals so far (memset 0)
    unsigned long long* boxes;        // per slot 8 words: side s's box as (lo0, hi0), (lo1, hi1), (lo2, hi2) at 4 s + 0 .. 2
    RefitResult* results;             // per selected mesh (memset 0)
};
}  // namespace rtd

#endif
