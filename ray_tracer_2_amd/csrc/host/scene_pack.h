// scene_pack.h -- the host packer: scene arrays (include/rt_abi.h) -> the scene blob the kernels walk
// (csrc/rt_scene_format.h).  Plain C++ without HIP, so that a blob can be produced, compared and run under the host
// sanitizers on a machine without a GPU; rt_api.hip only puts the result on the device.
//
// One upload in two phases.  The blob is a head -- mesh records, materials, spheres, items,
// top-level trees, forest entries -- and a tail from wide_off on: wide BVH records, triangle intersection records, shade
// records.  The tail holds record and triangle indices, never byte offsets, so its bytes do not depend on where it
// starts.  The geometry phase builds the tail and the per-mesh facts that depend only on triangles / nodes / offsets
// (O(meshes): no triangle or node array is kept); the instance phase builds the head from those facts and the
// transforms, materials and spheres.  rt_upload_scene runs both, rt_update_instances and rt_refit_triangles only the second.
#ifndef RT_SCENE_PACK_H
#define RT_SCENE_PACK_H

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../rt_scene_format.h"

namespace rt2 {

// One 16-byte word of the blob (the staging vectors' element: a float4 without HIP, with float4's size and alignment).
struct alignas(16) Quad { float x, y, z, w; };
static_assert(sizeof(Quad) == 16, "the blob is made of 16-byte words");

// The one float / bits pun of the packer (integers travel in the blob's float words).
inline float as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
inline uint32_t as_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// The 64-byte two-child record (rt_scene_format.h: WIDE_REC_BYTES) of a BVH node or a node of a top-level tree:
// (box a, ref a, box b, ref b), a ref being (idx, count).
struct Child { float lo[3], hi[3]; uint32_t idx, count; };
struct Rec2 { Quad q[4]; };
static_assert(sizeof(Rec2) == rtd::WIDE_REC_BYTES, "a two-child record is one wide record");
inline Rec2 write_rec2(const Child& a, const Child& b) {
    return Rec2{{{a.lo[0], a.hi[0], a.lo[1], a.hi[1]}, {a.lo[2], a.hi[2], as_float(a.idx), as_float(a.count)},
                 {b.lo[0], b.hi[0], b.lo[1], b.hi[1]}, {b.lo[2], b.hi[2], as_float(b.idx), as_float(b.count)}}};
}
inline Child read_rec2(const Rec2& r, int c) {
    const Quad &p = r.q[2 * c], &q = r.q[2 * c + 1];
    return Child{{p.x, p.z, q.x}, {p.y, p.w, q.y}, as_bits(q.z), as_bits(q.w)};
}

// The options the packer reads (rt_set_option: they take effect at the next upload).
struct PackOptions {
    // 0 = every mesh is a single item / no forest items / meshes with a two-leaf BVH are not run as straight-line items
    int tlas = 1, forest = 1, flat2 = 1;
    int tlas_min = (int)rtd::TLAS_MIN_MESHES;  // smallest run of meshes that gets a top-level tree
    int defer_min_nodes = 1024;                // smallest BVH (internal nodes) that is worth deferring
};

// Per-mesh facts of a scene that depend only on its triangles, nodes and offsets.
struct MeshGeom {
    uint32_t node_offset = 0, triangle_offset = 0, triangles = 0;  // as uploaded: an update must keep them
    uint32_t wide_base = 0, internal = 0;                           // first wide record, internal nodes
    uint32_t root_idx = 0, root_count = 0;                          // the root: record index, or triangle index + count (leaf)
    uint32_t tri_lo = 0xffffffffu, tri_hi = 0u;                     // triangle range of the leaves
    uint32_t node_lo = 0, node_hi = 0;                              // interval of the nodes the root reaches (a refit's selection)
    uint32_t need = 0;                                              // stack entries of its walk
    float box_lo[3] = {0, 0, 0}, box_hi[3] = {0, 0, 0};             // the root node's box
    bool deep = false;          // height >= 32: the shader's literal stack (DMESH_DEEP)
    bool contains = false;      // internal root whose box provably contains its children's (finite, proper)
    bool unions = true;         // (internal root) the root box contains the union of two proper child boxes: roots_are_unions
    bool flat2_shape = false;   // internal, not deep, two leaf children (ITEM_FLAT2 when the scene allows it)
    bool hierarchy_ok = false;  // not deep, and a proper bounding hierarchy (cross-mesh pruning)
};
struct SceneGeom {
    std::vector<MeshGeom> mesh;
    uint32_t n_nodes = 0, n_triangles = 0, n_wide = 0;
    uint32_t max_height = 0, max_leaf_ref = 0;  // (largest triangle count of a leaf that can go on a stack)
    uint32_t top_mesh_records = 0, top_mesh_base = 0;
    bool roots_are_unions = true, any_deep = false;
    uint64_t tail_bytes() const {
        return (uint64_t)n_wide * rtd::WIDE_REC_BYTES + (uint64_t)n_triangles * (rtd::TRI_ISECT_BYTES + rtd::TRI_SHADE_BYTES);
    }
};

// What the instance phase decides, beside the head itself.
struct InstanceFacts {
    rtd::SceneLayout lay{};
    uint32_t n_items = 0, n_tlas_records = 0, n_forest_entries = 0, tlas_entries = 1;
    bool has_tlas = false, has_forest = false, plain_materials = false;  // (plain: no spheres, no glass, no textured material)
    // deferred walks (RenderArgs::park): the deferred mesh, the mesh whose matrices give its local ray, its internal nodes
    bool have_defer = false;
    uint32_t defer_mesh = 0, defer_xform = 0, defer_internal = 0;
};

// The geometry phase: validates every mesh's BVH, fills `g` and the tail [wide_off, bytes) of the blob.
// Returns RT_OK, RT_ERR_INDEX_RANGE or RT_ERR_CAPACITY with `why`.
int pack_geometry(const rt_mesh_uniform* meshes, uint32_t n_meshes, const rt_packed_triangle* triangles, uint32_t n_triangles,
                  const rt_node* nodes, uint32_t n_nodes, SceneGeom& g, std::vector<Quad>& tail, std::string& why);

// The instance phase: the facts and the head [0, lay.wide_off) of the blob.  Returns RT_OK or RT_ERR_CAPACITY with `why`.
int pack_instances(const PackOptions& opt, const SceneGeom& g, const rt_sphere* spheres, uint32_t n_spheres, const rt_mesh_uniform* meshes,
                   uint32_t n_meshes, InstanceFacts& facts, std::vector<Quad>& head, std::string& why);

}  // namespace rt2

#endif
