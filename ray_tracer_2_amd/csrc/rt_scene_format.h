// rt_scene_format.h -- the format of the scene blob: its layout, record sizes and flag words.  Shared by the host packer
// that writes the blob (host/scene_pack.cpp: plain C++, no HIP), by rt_api.hip, which puts it on the device, and by the
// kernels that read it (through rt_device.h).
#ifndef RT_SCENE_FORMAT_H
#define RT_SCENE_FORMAT_H

#include <stdint.h>

#include "../../include/rt_abi.h"

namespace rtd {

// The whole scene is one blob of 16-byte words, either read in place (global
// memory: uniform reads become scalar loads) or, when it fits the LDS budget,
// staged into LDS once per workgroup with coalesced 16-byte loads.  All
// offsets below are byte offsets into that blob.
struct SceneLayout {
    uint32_t mesh_off;    // MESH_REC_BYTES per mesh
    uint32_t wide_off;    // WIDE_REC_BYTES per internal BVH node
    uint32_t tri_off;     // TRI_ISECT_BYTES per triangle
    uint32_t shade_off;   // TRI_SHADE_BYTES per triangle
    uint32_t mat_off;     // 96 B rt_material per mesh, then per sphere
    uint32_t sphere_off;  // 16 B (centre, radius) per sphere
    uint32_t item_off;    // ITEM_BYTES per item of the mesh loop
    uint32_t tlas_off;    // WIDE_REC_BYTES per node of the top-level trees over mesh root boxes
    uint32_t forest_off;  // FOREST_ENTRY_BYTES per member of the forest items
    uint32_t bytes;       // total, multiple of 16
    uint32_t _pad[2];
};

// The mesh loop (wgsl:369) runs over items.  An item is one mesh, or a top-level tree
// (TLAS) over the root boxes of a run of meshes that share one world_to_model matrix and
// have internal roots; the order in which meshes are visited is free because ties between
// equal world distances are broken by mesh index, exactly as the shader's in-order loop with
// its strict `<` does.  Two 16-byte words per item:
//   q0 = (kind, a, b, c): kind = ITEM_* flags; b = mesh whose matrices give the local ray when
//        ITEM_NEW_XFORM is set; single mesh: a = mesh index, c = its wide_base;
//        TLAS: a = root node index, c = number of meshes below it
//   q1 = single mesh: a copy of the mesh record's q8 (flags, root_idx, root_count, tri_base), so
//        that a mesh visit needs no dependent load.
//   forest (ITEM_FOREST): a = first member entry, c = number of members (<= 32): meshes with an
//        internal, non-deep root that share both matrices; each lane walks the members whose root
//        box it hits one after the other, independently of the other lanes (traverse_forest).
constexpr uint32_t ITEM_BYTES = 32;
//   flat (ITEM_FLAT2, an attribute of a single-mesh item): the mesh's BVH is a root with two LEAF children
//        (a quad split into its two triangles, ...).  Its whole traversal is two box tests and the leaves' triangles,
//        near leaf first: the few-mesh kernels run it as straight-line code with every lane of the wave in step,
//        no stack and no loop (traverse_flat2), instead of as a forest member or a mesh walk.
enum : uint32_t { ITEM_TLAS = 1u, ITEM_NEW_XFORM = 2u, ITEM_FOREST = 4u, ITEM_FLAT2 = 8u,
                  ITEM_DEFER = 16u,       // the big mesh whose walk a launch with RenderArgs::park != 0 defers (last item)
                  ITEM_DEFER_CULL = 32u,  // ... and its root box provably contains its children's (missing it = missing the mesh)
                  ITEM_PRUNE = 64u        // cross-mesh pruning may cut this item's meshes (RenderArgs::cross_prune): every mesh of the
                                          // item has the model_to_world of the mesh that gives the local ray, bit for bit, and a BVH
                                          // that is a proper bounding hierarchy (checked at upload, rt_api.hip)
};
// A top-level tree's reference to a mesh (the child index of a tree record whose child count is non-zero; with bit
// 31 set, an entry of the tree stack): everything a lane needs to enter the mesh -- the mesh's index (the caps allow
// 400), the absolute index of its root's wide record (<= 1.3 M internal nodes) and whether it is glass (wgsl:376: no
// backface culling).  Meshes that do not fit these fields stay single items.
enum : uint32_t {
    TLAS_REF_ROOT_MASK = 0x001fffffu,  // bits 0-20
    TLAS_REF_MESH_SHIFT = 21u,
    TLAS_REF_MESH_MASK = 0x1ffu,       // bits 21-29
    TLAS_REF_GLASS = 0x40000000u,      // bit 30
};
// Forest member entry, 3 x 16 B: q0 = (root wide index, mesh index, flags, 0), q1/q2 = the root's
// packed box (as in a wide record).  flags: DMESH_GLASS, FOREST_CULLABLE = the root box provably
// contains the boxes of the root's children (so missing it means missing the mesh).
constexpr uint32_t FOREST_ENTRY_BYTES = 48;
constexpr uint32_t FOREST_MAX_MEMBERS = 32;
constexpr uint32_t FOREST_CULLABLE = 0x100u;
constexpr uint32_t TLAS_MIN_MESHES = 8;

// Mesh record, 12 x 16 B:
//   q0..q3  world_to_model columns   q4..q7  model_to_world columns
//   q8 = (flags, root_idx, root_count, tri_base)
//   q9 = (wide_base, S, C, 0): S >= the largest absolute row sum of model_to_world's 3 x 3 part, C >= the largest
//        absolute component of its translation (rounded up by the host; cross-mesh pruning's error terms)
//   q10 = root (min.x, max.x, min.y, max.y)   q11 = root (min.z, max.z, 0, 0)
// root_count > 0: the root is a leaf with triangles [root_idx, root_idx+count);
// root_count == 0: root_idx is the mesh-local index of its wide record.
constexpr uint32_t MESH_REC_BYTES = 192;
enum : uint32_t {
    DMESH_GLASS = 2u,       // material.flag == GLASS  => no backface culling (wgsl:375)
    DMESH_DEEP = 4u,        // BVH height >= 32: the shader's 32-entry stack can overflow; traverse it
                            // with the shader's literal push/pop and index clamping (naga Restrict)
};
// Wide BVH record of one internal node (both children's boxes inline, so a
// visit is one round trip instead of three dependent ones), 4 x 16 B:
//   q0 = (a.min.x, a.max.x, a.min.y, a.max.y) q1 = (a.min.z, a.max.z, a_idx, a_count)
//   q2, q3 = the same for child b   (min/max of an axis adjacent: one packed-f32 pair per axis)
// child leaf: idx = first triangle (mesh-local), count > 0;
// child internal: idx = mesh-local wide index, count = 0.
constexpr uint32_t WIDE_REC_BYTES = 64;
// Triangle intersection record, 3 x 16 B:
//   q0 = (v1.xyz, n.x) q1 = (edge_ab.xyz, n.y) q2 = (edge_ac.xyz, n.z)
//   with edge_ab = v2 - v1, edge_ac = v3 - v1, n = cross(edge_ab, edge_ac)
//   exactly as wgsl:261-263 computes them per test.
constexpr uint32_t TRI_ISECT_BYTES = 48;
// Triangle shading record, 4 x 16 B:
//   q0 = (n1.xyz, u10) q1 = (n2.xyz, u11) q2 = (n3.xyz, u20) q3 = (u21, u30, u31, 0)
constexpr uint32_t TRI_SHADE_BYTES = 64;
constexpr uint32_t MATERIAL_BYTES = 96;
constexpr uint32_t SPHERE_BYTES = 16;

}  // namespace rtd

#endif
