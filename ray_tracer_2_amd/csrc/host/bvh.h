// bvh.h -- per-mesh SAH BVH builder restating src/core/bvh.rs operation for
// operation in f32 (the comparison `cost < best_cost` and the in-place
// partition decide triangle order, hence traversal order, hence the floats
// the shader produces).  Host-side; results-identical, not accelerated.
#ifndef RT_BVH_H
#define RT_BVH_H

#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../../../include/rt_abi.h"
#include "glam_math.h"

namespace rt2 {

struct Vertex {  // src/scene/components/geometry/vertex.rs:3-8
    Vec3 pos, normal;
    float uv[2] = {0, 0};
};

enum class Quality { Low = 0, High = 1, Disabled = 2 };  // bvh.rs:126-131

struct BvhResult {
    std::vector<rt_packed_triangle> triangles;
    std::vector<rt_node> nodes;
    std::vector<uint32_t> order;  // order[k]: the source triangle (BuildTri::i / 3) of packed triangle k
};

// ≙ BVH::build (bvh.rs:208-290)
BvhResult bvh_build(const std::vector<Vertex>& vertices, const std::vector<uint32_t>& indices,
                    Quality quality);

// Level-wise variant for large meshes: the same nodes, node numbering and triangle order as
// bvh_build, built breadth-first so that the SAH searches of a whole level (find_best_split,
// bvh.rs:299-351 -- the O(150 n)-per-level part) can be delegated in one batch, e.g. to the GPU
// (csrc/rt_bvh_search.hip).  The partitions and everything else run here, as in bvh_build.
struct SplitQuery {  // a node of the level: its range in the current triangle order and its bounds
    uint32_t start, count;
    float aabb_min[3], aabb_max[3];
};
struct SplitResult {  // find_best_split's (cost, axis, split_pos)
    int axis;
    float pos, cost;
};
// order[p] = original triangle index at position p of the current order (n entries)
using LevelSearch = std::function<void(const uint32_t* order, size_t n, const std::vector<SplitQuery>&, std::vector<SplitResult>&)>;
// per original triangle: centroid, min, max (9 floats) -- what a LevelSearch needs to price planes
std::vector<float> bvh_search_data(const std::vector<Vertex>& vertices, const std::vector<uint32_t>& indices);
BvhResult bvh_build_levels(const std::vector<Vertex>& vertices, const std::vector<uint32_t>& indices, Quality quality,
                           const LevelSearch& search);
// the searches on the GPU (throws std::runtime_error on HIP errors)
LevelSearch make_device_level_search(int device, const float* tri9, size_t n_tris);
// the searches on the host (reference implementation of a LevelSearch; tests)
LevelSearch make_host_level_search(const float* tri9, size_t n_tris);

// ---- refit (include/rt_abi.h: rt_refit_bvh; the box rule is csrc/rt_refit.h) ----
// What the selection of a refit needs of a mesh: its leaves' triangle range [tri_lo, tri_hi) (absolute; empty when
// tri_lo >= tri_hi), the interval [node_lo, node_hi] of the nodes its root reaches, and its triangle_offset.
struct RefitSpan {
    uint32_t tri_lo, tri_hi, node_lo, node_hi, triangle_offset;
};
// The span of mesh m over `nodes` (validated as rt_upload_scene validates a mesh: indices in range, no cycle).
// Returns RT_OK or RT_ERR_INDEX_RANGE with `why`.
int refit_span(const rt_mesh_uniform& m, const rt_node* nodes, uint32_t n_nodes, uint32_t n_triangles, RefitSpan& out,
               std::string& why);
// The meshes a refit of triangles [first, first + n) selects -- those whose leaf range meets it --, in mesh order;
// RT_ERR_INVALID_ARGUMENT (err names the mesh) when a selected mesh's leaf range is not inside [first, first + n) or its
// node interval overlaps that of a mesh with another triangle_offset.
int refit_select(const std::vector<RefitSpan>& spans, uint32_t first, uint32_t n, std::vector<uint32_t>& selected,
                 std::string& err);
// rt_refit_bvh
int refit_bvh(const rt_mesh_uniform* meshes, uint32_t n_meshes, const rt_packed_triangle* triangles, uint32_t n_triangles,
              rt_node* nodes, uint32_t n_nodes, uint32_t first, uint32_t n, std::string& err);

}  // namespace rt2

#endif
