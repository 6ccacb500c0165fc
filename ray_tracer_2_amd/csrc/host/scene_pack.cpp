// scene_pack.cpp -- see scene_pack.h.  Every derived value that reaches the blob is computed with the same IEEE
// operations the shader would execute per ray (binary32 edges and normals; S, C and the SAH costs in double), so the
// re-layout is results-preserving.
#include "scene_pack.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <utility>

namespace rt2 {

using namespace rtd;

// Height (in edges) of the BVH under a mesh's root, with index validation and a visit budget that catches cycles.
// Returns RT_OK or RT_ERR_INDEX_RANGE with `why`.
static int mesh_bvh_height(const rt_node* nodes, uint32_t n_nodes, uint32_t node_offset, uint32_t tri_offset, uint32_t n_triangles, uint32_t& height, std::string& why) {
    auto bad = [&why](const char* what) { why = what; return (int)RT_ERR_INDEX_RANGE; };
    if (node_offset >= n_nodes) return bad("mesh node_offset out of range");
    // Iterative: explicit (node, depth) stack.
    std::vector<std::pair<uint32_t, uint32_t>> st;
    st.emplace_back(node_offset, 0u);
    uint64_t visits = 0;
    height = 0;
    while (!st.empty()) {
        auto [idx, depth] = st.back();
        st.pop_back();
        if (++visits > (uint64_t)n_nodes + 1) return bad("BVH has a cycle");
        const rt_node& nd = nodes[idx];
        if (depth > height) height = depth;
        if (nd.count > 0) {
            if ((uint64_t)tri_offset + nd.first + nd.count > n_triangles) return bad("leaf triangle range out of bounds");
        } else {
            uint64_t a = (uint64_t)node_offset + nd.left, b = (uint64_t)node_offset + nd.right;
            if (a >= n_nodes || b >= n_nodes) return bad("BVH child index out of range");
            st.emplace_back((uint32_t)a, depth + 1);
            st.emplace_back((uint32_t)b, depth + 1);
        }
    }
    return RT_OK;
}

namespace {

// ---- geometry phase ---------------------------------------------------------------------------------------------------

// Record order of a mesh with an internal root (`mn`: its nodes): the first TOP_BFS internal nodes breadth-first from
// the root (any prefix of them is a "top of the tree": what the render kernels stage into LDS for a big mesh), the
// rest in depth-first pre-order below them.  Returns the mesh-local indices of the internal nodes in record order and
// sets wide_index[node] (`wide_index` is per node of the mesh) to each one's place in it.
std::vector<uint32_t> record_order(const rt_node* mn, uint32_t* wide_index) {
    std::vector<uint32_t> order, frontier{0u}, st;
    constexpr size_t TOP_BFS = 2048;
    for (size_t q = 0; q < frontier.size(); ++q) {
        const uint32_t n = frontier[q];
        if (order.size() >= TOP_BFS) { st.push_back(n); continue; }
        wide_index[n] = (uint32_t)order.size();
        order.push_back(n);
        if (mn[mn[n].left].count == 0) frontier.push_back(mn[n].left);
        if (mn[mn[n].right].count == 0) frontier.push_back(mn[n].right);
    }
    std::reverse(st.begin(), st.end());  // (pop order = breadth-first order of the cut)
    while (!st.empty()) {
        uint32_t n = st.back();
        st.pop_back();
        wide_index[n] = (uint32_t)order.size();
        order.push_back(n);
        if (mn[mn[n].right].count == 0) st.push_back(mn[n].right);
        if (mn[mn[n].left].count == 0) st.push_back(mn[n].left);
    }
    return order;
}

// The root checks of a mesh with an internal root: does the root box provably contain its children's boxes
// (root_box_ok in the instance phase adds "walked with the ordinary stack"; the root-box shortcut, roots_are_unions,
// needs the same containment of proper child boxes), and is the root's BVH two leaves (ITEM_FLAT2)?
void check_root(const rt_node* mn, MeshGeom& mg) {
    const rt_node &ca = mn[mn[0].left], &cb = mn[mn[0].right];
    mg.contains = mg.unions = true;
    for (int k = 0; k < 3; ++k) {
        const float lo_k = ca.aabb_min[k] < cb.aabb_min[k] ? ca.aabb_min[k] : cb.aabb_min[k];
        const float hi_k = ca.aabb_max[k] > cb.aabb_max[k] ? ca.aabb_max[k] : cb.aabb_max[k];
        // the root box may also be larger than the union (still conservative)
        if (!(mn[0].aabb_min[k] <= lo_k && mn[0].aabb_max[k] >= hi_k)) mg.contains = mg.unions = false;
        // (and the children must be proper boxes, or the interval argument does not hold)
        if (!(ca.aabb_min[k] <= ca.aabb_max[k] && cb.aabb_min[k] <= cb.aabb_max[k])) mg.contains = mg.unions = false;
        if (!(mn[0].aabb_min[k] - mn[0].aabb_min[k] == 0.0f && mn[0].aabb_max[k] - mn[0].aabb_max[k] == 0.0f)) mg.contains = false;  // finite
    }
    // (root with two leaf children: a straight-line item in the few-mesh kernels, ITEM_FLAT2)
    mg.flat2_shape = !mg.deep && ca.count > 0 && cb.count > 0;
}

// A proper bounding hierarchy (cross-mesh pruning, pack_instances): finite boxes, every child box inside its
// parent's, every leaf triangle inside its leaf's box (true of the reference's builder; verified, since BVHs may
// be foreign).  `mn` / `tris`: the mesh's nodes and triangles.
bool hierarchy_ok(const rt_node* mn, const rt_packed_triangle* tris) {
    std::vector<uint32_t> st{0u};
    while (!st.empty()) {
        const rt_node& n = mn[st.back()];
        st.pop_back();
        for (int k = 0; k < 3; ++k)  // a proper, finite box
            if (!(n.aabb_min[k] <= n.aabb_max[k] && n.aabb_min[k] - n.aabb_min[k] == 0.0f && n.aabb_max[k] - n.aabb_max[k] == 0.0f)) return false;
        if (n.count > 0) {
            for (uint32_t t = 0; t < n.count; ++t) {
                const rt_packed_triangle& p = tris[n.first + t];
                for (const float* v : {p.v1, p.v2, p.v3})
                    for (int k = 0; k < 3; ++k)
                        if (!(v[k] >= n.aabb_min[k] && v[k] <= n.aabb_max[k])) return false;
            }
        } else {
            for (uint32_t c : {n.left, n.right}) {
                const rt_node& ch = mn[c];
                for (int k = 0; k < 3; ++k)
                    if (!(ch.aabb_min[k] >= n.aabb_min[k] && ch.aabb_max[k] <= n.aabb_max[k])) return false;
                st.push_back(c);
            }
        }
    }
    return true;
}

// The triangle re-layout (rt_scene_format.h): intersection records at `isect`, shade records at `shade`.  The
// subtractions and the cross product are wgsl:261-263, evaluated once here in binary32.
void relayout_triangles(const rt_packed_triangle* triangles, uint32_t n_triangles, Quad* isect, Quad* shade) {
    for (uint32_t t = 0; t < n_triangles; ++t) {
        const rt_packed_triangle& p = triangles[t];
        float abx = p.v2[0] - p.v1[0], aby = p.v2[1] - p.v1[1], abz = p.v2[2] - p.v1[2];
        float acx = p.v3[0] - p.v1[0], acy = p.v3[1] - p.v1[1], acz = p.v3[2] - p.v1[2];
        float nx = aby * acz - abz * acy, ny = abz * acx - abx * acz, nz = abx * acy - aby * acx;
        Quad* ti = isect + (size_t)t * (TRI_ISECT_BYTES / 16);
        ti[0] = Quad{p.v1[0], p.v1[1], p.v1[2], nx};
        ti[1] = Quad{abx, aby, abz, ny};
        ti[2] = Quad{acx, acy, acz, nz};
        Quad* ts = shade + (size_t)t * (TRI_SHADE_BYTES / 16);
        ts[0] = Quad{p.n1[0], p.n1[1], p.n1[2], p.uv10};
        ts[1] = Quad{p.n2[0], p.n2[1], p.n2[2], p.uv11};
        ts[2] = Quad{p.n3[0], p.n3[1], p.n3[2], p.uv20};
        ts[3] = Quad{p.uv21, p.uv30, p.uv31, 0.0f};
    }
}

}  // namespace

int pack_geometry(const rt_mesh_uniform* meshes, uint32_t n_meshes, const rt_packed_triangle* triangles, uint32_t n_triangles,
                  const rt_node* nodes, uint32_t n_nodes, SceneGeom& g, std::vector<Quad>& tail, std::string& why) {
    // ---- validation + wide BVH records ---------------------------------
    std::vector<Rec2> wide;
    g.mesh.assign(n_meshes, MeshGeom{});
    g.n_nodes = n_nodes;
    g.n_triangles = n_triangles;
    std::vector<uint32_t> wide_index(n_nodes, 0xffffffffu);  // per original node
    for (uint32_t i = 0; i < n_meshes; ++i) {
        const rt_mesh_uniform& m = meshes[i];
        MeshGeom& mg = g.mesh[i];
        mg.node_offset = m.node_offset;
        mg.triangle_offset = m.triangle_offset;
        mg.triangles = m.triangles;
        uint32_t height = 0;
        int rc = mesh_bvh_height(nodes, n_nodes, m.node_offset, m.triangle_offset, n_triangles, height, why);
        if (rc != RT_OK) { why = "mesh " + std::to_string(i) + ": " + why; return rc; }
        // The shader's stack holds 32 entries (wgsl:297); with the near child kept in
        // registers this kernel needs `height` entries and the shader height + 1.  A
        // tree of height >= 32 can overflow the shader's stack; such a mesh is traversed
        // with the shader's literal push/pop and clamped indices (DMESH_DEEP), which
        // needs the full 32 entries.
        mg.deep = height + 1 > RT_BVH_STACK;
        mg.need = mg.deep ? RT_BVH_STACK : height;
        if (mg.need > g.max_height) g.max_height = mg.need;
        // Wide records: internal nodes in record order, indexed per mesh.
        // (Meshes may alias node ranges; records are built per mesh.)
        mg.wide_base = (uint32_t)wide.size();
        mg.node_lo = mg.node_hi = m.node_offset;
        const rt_node* mn = nodes + m.node_offset;
        for (int k = 0; k < 3; ++k) { mg.box_lo[k] = mn[0].aabb_min[k]; mg.box_hi[k] = mn[0].aabb_max[k]; }
        // (child and root indices are absolute: triangle index into the scene's triangle
        // array, wide-record index into the scene's record array)
        if (mn[0].count > 0) {
            mg.root_idx = m.triangle_offset + mn[0].first;
            mg.root_count = mn[0].count;
            mg.tri_lo = mg.root_idx;
            mg.tri_hi = mg.root_idx + mg.root_count;
            continue;
        }
        mg.root_idx = mg.wide_base;
        const std::vector<uint32_t> order = record_order(mn, wide_index.data() + m.node_offset);
        if (order.size() > g.top_mesh_records) {  // the biggest BVH gets the LDS-staged top
            g.top_mesh_records = (uint32_t)order.size();
            g.top_mesh_base = mg.wide_base;
        }
        for (uint32_t n : order) {
            mg.node_hi = std::max({mg.node_hi, m.node_offset + mn[n].left, m.node_offset + mn[n].right});
            auto child = [&](uint32_t local) {
                const rt_node& c = mn[local];
                Child out{{c.aabb_min[0], c.aabb_min[1], c.aabb_min[2]}, {c.aabb_max[0], c.aabb_max[1], c.aabb_max[2]},
                          m.triangle_offset + c.first, c.count};
                if (c.count > 0) {
                    if (c.count > g.max_leaf_ref) g.max_leaf_ref = c.count;
                    mg.tri_lo = std::min(mg.tri_lo, out.idx);
                    mg.tri_hi = std::max(mg.tri_hi, out.idx + c.count);
                } else {
                    out.idx = mg.wide_base + wide_index[m.node_offset + local];
                }
                return out;
            };
            const Child a = child(mn[n].left), b = child(mn[n].right);
            wide.push_back(write_rec2(a, b));
        }
    }
    g.n_wide = (uint32_t)wide.size();
    for (uint32_t i = 0; i < n_meshes; ++i) {
        MeshGeom& mg = g.mesh[i];
        mg.internal = (i + 1 < n_meshes ? g.mesh[i + 1].wide_base : g.n_wide) - mg.wide_base;
        const rt_node* mn = nodes + meshes[i].node_offset;
        g.any_deep = g.any_deep || mg.deep;
        if (mn[0].count == 0) check_root(mn, mg);
        g.roots_are_unions = g.roots_are_unions && mg.unions;  // (a leaf root keeps unions = true)
        // (only asked of meshes walked with the ordinary stack)
        if (!mg.deep) mg.hierarchy_ok = hierarchy_ok(mn, triangles + meshes[i].triangle_offset);
    }
    // ---- the tail: wide records, then the triangle re-layout (see rt_scene_format.h) ----
    const uint64_t tail_bytes = g.tail_bytes();
    if (tail_bytes > 0xfffffff0ull) { why = "scene larger than 4 GiB"; return RT_ERR_CAPACITY; }
    tail.assign(tail_bytes / 16, Quad{0, 0, 0, 0});
    if (!wide.empty()) memcpy(tail.data(), wide.data(), wide.size() * sizeof(Rec2));
    Quad* isect = tail.data() + (size_t)g.n_wide * (WIDE_REC_BYTES / 16);
    relayout_triangles(triangles, n_triangles, isect, isect + (size_t)n_triangles * (TRI_ISECT_BYTES / 16));
    return RT_OK;
}

// ---- instance phase -----------------------------------------------------------------------------------------------------
namespace {

struct Item { uint32_t kind, a, b, n; };
struct ForestEntry { Quad q[3]; };
static_assert(sizeof(ForestEntry) == FOREST_ENTRY_BYTES, "a forest entry is three 16-byte words");
struct Run { uint32_t begin, end; };

// Runs of consecutive meshes with bit-identical world_to_model: they share a local space.
std::vector<Run> transform_runs(const rt_mesh_uniform* meshes, uint32_t n_meshes) {
    std::vector<Run> runs;
    for (uint32_t i0 = 0; i0 < n_meshes;) {
        uint32_t i1 = i0 + 1;
        while (i1 < n_meshes && memcmp(meshes[i1].world_to_model, meshes[i0].world_to_model, 64) == 0) ++i1;
        runs.push_back(Run{i0, i1});
        i0 = i1;
    }
    return runs;
}

bool is_glass(const rt_mesh_uniform& m) { return m.material.flag == RT_MATERIAL_GLASS; }
// (root_box_ok: the root box provably contains its children's boxes and the mesh is walked with the ordinary stack)
bool root_box_ok(const MeshGeom& r) { return !r.deep && r.contains; }
// (a tree's reference to a mesh has 9 bits for the mesh and 21 for its root record, rt_scene_format.h)
bool tree_ok(const std::vector<MeshGeom>& mg, uint32_t i) {
    return root_box_ok(mg[i]) && i <= TLAS_REF_MESH_MASK && mg[i].root_idx <= TLAS_REF_ROOT_MASK;
}
uint32_t ceil_log2(size_t n) { uint32_t d = 0; while (((size_t)1 << d) < n) ++d; return d; }

// What the instance phase works on: the scene and the parts of the head as they are decided -- items, the records of all
// trees so far, forest entries --, the depth limit of the tree being built (the balanced tree's depth + 6) and the deepest
// level any tree has reached.
struct Head {
    const std::vector<MeshGeom>& mg;
    const rt_mesh_uniform* meshes;
    std::vector<Item> items;
    std::vector<Rec2> tlas;
    std::vector<ForestEntry> forest;
    uint32_t max_depth = 0, depth = 0;
};

auto centroid_less(const std::vector<MeshGeom>& mg, int axis) {
    return [&mg, axis](uint32_t x, uint32_t y) {
        const MeshGeom &rx = mg[x], &ry = mg[y];
        const float cx = rx.box_lo[axis] + rx.box_hi[axis], cy = ry.box_lo[axis] + ry.box_hi[axis];
        return cx < cy || (cx == cy && x < y);
    };
}

// Split of ms[b0, e0): surface-area heuristic over the root boxes, swept along each axis in centroid order (the
// boxes are few -- one per mesh -- so the full sweep is affordable; a median split put the scene-wide
// floor and ceiling meshes of the many-mesh stand-in into the same subtrees as the columns next to
// their centroids).  Any split is a correct one: the tree only has to contain its root boxes.  Sorts the range;
// returns the axis and the size of the left part.
std::pair<int, size_t> sah_split(const std::vector<MeshGeom>& mg, std::vector<uint32_t>& ms, size_t b0, size_t e0) {
    auto half_area = [](const double* lo3, const double* hi3) {
        const double dx = hi3[0] - lo3[0], dy = hi3[1] - lo3[1], dz = hi3[2] - lo3[2];
        return dx * dy + dy * dz + dz * dx;
    };
    auto grow = [](const MeshGeom& r, double* lo3, double* hi3) {
        for (int k = 0; k < 3; ++k) {
            if (r.box_lo[k] < lo3[k]) lo3[k] = r.box_lo[k];
            if (r.box_hi[k] > hi3[k]) hi3[k] = r.box_hi[k];
        }
    };
    const size_t cnt_here = e0 - b0;
    int best_axis = 0;
    size_t best_left = cnt_here / 2;
    double best_cost = DBL_MAX;
    std::vector<double> right_area(cnt_here);
    for (int axis = 0; axis < 3; ++axis) {
        std::sort(ms.begin() + b0, ms.begin() + e0, centroid_less(mg, axis));
        double lo3[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, hi3[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
        for (size_t q = cnt_here; q-- > 1;) {  // right_area[q]: boxes q .. end
            grow(mg[ms[b0 + q]], lo3, hi3);
            right_area[q] = half_area(lo3, hi3);
        }
        for (int k = 0; k < 3; ++k) { lo3[k] = DBL_MAX; hi3[k] = -DBL_MAX; }
        for (size_t q = 1; q < cnt_here; ++q) {  // left = boxes 0 .. q-1
            grow(mg[ms[b0 + q - 1]], lo3, hi3);
            const double cost = half_area(lo3, hi3) * (double)q + right_area[q] * (double)(cnt_here - q);
            if (cost < best_cost) { best_cost = cost; best_axis = axis; best_left = q; }
        }
    }
    return {best_axis, best_left};
}

// Recursive split over the root boxes of ms[b0, e0); returns the child reference (idx, count) and its box.
Child build_tree(Head& cx, std::vector<uint32_t>& ms, size_t b0, size_t e0, uint32_t depth) {
    if (depth > cx.depth) cx.depth = depth;
    if (e0 - b0 == 1) {
        const MeshGeom& r = cx.mg[ms[b0]];
        const uint32_t ref = r.root_idx | (ms[b0] << TLAS_REF_MESH_SHIFT) | (is_glass(cx.meshes[ms[b0]]) ? TLAS_REF_GLASS : 0u);
        return Child{{r.box_lo[0], r.box_lo[1], r.box_lo[2]}, {r.box_hi[0], r.box_hi[1], r.box_hi[2]}, ref, 1};
    }
    const size_t cnt_here = e0 - b0;
    auto [best_axis, best_left] = sah_split(cx.mg, ms, b0, e0);
    // (every lane keeps a tree stack of depth + 2 entries in LDS: a subtree that would not fit below the
    // depth limit any other way is split in the middle)
    if (depth + ceil_log2(cnt_here) >= cx.max_depth) best_left = cnt_here / 2;
    std::sort(ms.begin() + b0, ms.begin() + e0, centroid_less(cx.mg, best_axis));
    const size_t mid = b0 + best_left;
    const uint32_t me = (uint32_t)cx.tlas.size();
    cx.tlas.emplace_back();
    const Child a = build_tree(cx, ms, b0, mid, depth + 1);
    const Child b = build_tree(cx, ms, mid, e0, depth + 1);
    cx.tlas[me] = write_rec2(a, b);
    Child out{{}, {}, me, 0};
    for (int k = 0; k < 3; ++k) {  // exact union (min/max are exact)
        out.lo[k] = a.lo[k] < b.lo[k] ? a.lo[k] : b.lo[k];
        out.hi[k] = a.hi[k] > b.hi[k] ? a.hi[k] : b.hi[k];
    }
    return out;
}

// Number the tree records breadth-first from the roots (all trees together): any prefix of the array is then
// "the top levels", which is what option "lds_tlas" stages into LDS when the whole tree does not fit.
void renumber_trees(Head& h) {
    std::vector<uint32_t> order, new_of(h.tlas.size(), 0xffffffffu);
    for (const Item& it : h.items)
        if (it.kind & ITEM_TLAS) order.push_back(it.a);
    for (size_t q = 0; q < order.size(); ++q)
        for (int c = 0; c < 2; ++c)
            if (const Child ch = read_rec2(h.tlas[order[q]], c); ch.count == 0u) order.push_back(ch.idx);  // the child is a tree node
    if (order.size() != h.tlas.size()) return;
    for (size_t q = 0; q < order.size(); ++q) new_of[order[q]] = (uint32_t)q;
    std::vector<Rec2> re(h.tlas.size());
    for (size_t q = 0; q < order.size(); ++q) {
        Child ch[2] = {read_rec2(h.tlas[order[q]], 0), read_rec2(h.tlas[order[q]], 1)};
        for (Child& c : ch)
            if (c.count == 0u) c.idx = new_of[c.idx];
        re[q] = write_rec2(ch[0], ch[1]);
    }
    h.tlas.swap(re);
    for (Item& it : h.items)
        if (it.kind & ITEM_TLAS) it.a = new_of[it.a];
}

// ---- cross-mesh pruning (RenderArgs::cross_prune): which items may be cut, and the order of the loop ----
// An item gets ITEM_PRUNE when every mesh of it (a) has the model_to_world of the mesh that gives the item's
// local ray, bit for bit -- the kernel's bound on the world distance is derived from that matrix --, (b) is
// not glass (no backface culling: a ray leaving a surface is not culled against the coplanar triangles next
// to it, the one place where the triangle test's parameter is noise), (c) is walked with
// the ordinary stack, and (d) has a BVH that is a proper bounding hierarchy (MeshGeom::hierarchy_ok).
// (Only the scenes the many-mesh kernels render: not few_mesh.)
void mark_prune_and_order(Head& h) {
    auto mesh_prune_ok = [&](uint32_t i, uint32_t xform_mesh) {
        return !h.mg[i].deep && !is_glass(h.meshes[i]) && h.mg[i].hierarchy_ok &&
               memcmp(h.meshes[i].model_to_world, h.meshes[xform_mesh].model_to_world, 64) == 0;
    };
    // members of a tree, per tree item (the trees are not renumbered again below)
    for (Item& it : h.items) {
        bool ok = true;
        if (it.kind & ITEM_TLAS) {
            std::vector<uint32_t> st{it.a};
            while (!st.empty() && ok) {
                const Rec2 w = h.tlas[st.back()];
                st.pop_back();
                for (int c = 0; c < 2 && ok; ++c) {
                    const Child ch = read_rec2(w, c);
                    if (ch.count == 0u) st.push_back(ch.idx);
                    else ok = mesh_prune_ok((ch.idx >> TLAS_REF_MESH_SHIFT) & TLAS_REF_MESH_MASK, it.b);
                }
            }
        } else if (it.kind & ITEM_FOREST) {
            ok = false;  // (few-mesh kernels only)
        } else {
            ok = h.mg[it.a].root_count == 0u && mesh_prune_ok(it.a, it.b);
        }
        if (ok) it.kind |= ITEM_PRUNE;
    }
    // The loop's order is free (ties between equal world distances go to the lower mesh index, rt_kernel.hip):
    // first the meshes whose root is a leaf (the whole wave tests their triangles in step), then the other
    // single meshes, then the trees, so that the long walks start with a closest hit to prune against.  Inside
    // a class the order stays; an item opens its local space when its class's previous item had another one.
    std::vector<Item> ordered;
    for (int cls = 0; cls < 3; ++cls) {
        bool first = true;
        uint32_t prev_b = 0;
        for (const Item& it0 : h.items) {
            const int c = (it0.kind & ITEM_TLAS) ? 2 : ((it0.kind & ITEM_FOREST) || h.mg[it0.a].root_count == 0u) ? 1 : 0;
            if (c != cls) continue;
            Item it = it0;
            it.kind &= ~(uint32_t)ITEM_NEW_XFORM;
            if (first || it.b != prev_b) it.kind |= ITEM_NEW_XFORM;
            first = false;
            prev_b = it.b;
            ordered.push_back(it);
        }
    }
    // (classes follow each other: the first item of a class whose local space is the previous class's last one
    // need not open it again)
    for (size_t k = 1; k < ordered.size(); ++k)
        if (ordered[k].b == ordered[k - 1].b) ordered[k].kind &= ~(uint32_t)ITEM_NEW_XFORM;
    h.items.swap(ordered);
}

// ---- the deferred mesh (RenderArgs::park) ----------------------------------------------
// The biggest single-mesh item of a few-mesh scene with a real BVH:
// its item goes to the end of the mesh loop (the loop's order is free), where a launch can stop in front
// of it.
void choose_deferred(Head& h, const PackOptions& opt, InstanceFacts& out) {
    size_t best_k = h.items.size();
    uint32_t best_big = 0;
    for (size_t k = 0; k < h.items.size(); ++k) {
        const Item& it = h.items[k];
        if ((it.kind & (ITEM_TLAS | ITEM_FOREST | ITEM_FLAT2)) || h.mg[it.a].root_count != 0) continue;
        const uint32_t internal = h.mg[it.a].internal;
        if (internal >= (uint32_t)opt.defer_min_nodes && internal > best_big) { best_big = internal; best_k = k; }
    }
    if (best_k == h.items.size()) return;
    Item d = h.items[best_k];
    h.items.erase(h.items.begin() + (std::ptrdiff_t)best_k);
    // (the item that followed it in the same local space now opens that space)
    if ((d.kind & ITEM_NEW_XFORM) && best_k < h.items.size() && !(h.items[best_k].kind & ITEM_NEW_XFORM)) h.items[best_k].kind |= ITEM_NEW_XFORM;
    d.kind |= ITEM_NEW_XFORM | ITEM_DEFER | (h.mg[d.a].contains ? ITEM_DEFER_CULL : 0u);
    h.items.push_back(d);
    out.have_defer = true;
    out.defer_mesh = d.a;
    out.defer_xform = d.b;
    out.defer_internal = best_big;
}

// ---- blob layout ------------------------------------------------------
// (the per-scene sections first, the per-node / per-triangle arrays last: the small blob of the hybrid launches has
// the same sections with shorter arrays, so every offset up to wide_off is the same in both -- the primary-ray memo
// keeps a material's byte offset across launches that read different blobs)
bool layout_head(const Head& h, const SceneGeom& g, uint32_t n_meshes, uint32_t n_spheres, SceneLayout& lay) {
    uint64_t off = 0;
    lay.mesh_off = (uint32_t)off;   off += (uint64_t)n_meshes * MESH_REC_BYTES;
    lay.mat_off = (uint32_t)off;    off += (uint64_t)(n_meshes + n_spheres) * MATERIAL_BYTES;
    lay.sphere_off = (uint32_t)off; off += (uint64_t)n_spheres * SPHERE_BYTES;
    lay.item_off = (uint32_t)off;   off += (uint64_t)h.items.size() * ITEM_BYTES;
    lay.tlas_off = (uint32_t)off;   off += (uint64_t)h.tlas.size() * WIDE_REC_BYTES;
    lay.forest_off = (uint32_t)off; off += (uint64_t)h.forest.size() * FOREST_ENTRY_BYTES;
    lay.wide_off = (uint32_t)off;   off += (uint64_t)g.n_wide * WIDE_REC_BYTES;
    lay.tri_off = (uint32_t)off;    off += (uint64_t)g.n_triangles * TRI_ISECT_BYTES;
    lay.shade_off = (uint32_t)off;  off += (uint64_t)g.n_triangles * TRI_SHADE_BYTES;
    lay.bytes = (uint32_t)(off ? off : 16);
    return off <= 0xfffffff0ull;
}

void write_head(const Head& h, const SceneLayout& lay, const rt_sphere* spheres, uint32_t n_spheres, uint32_t n_meshes, std::vector<Quad>& head) {
    head.assign(lay.wide_off / 16, Quad{0, 0, 0, 0});
    for (uint32_t i = 0; i < n_meshes; ++i) {
        const rt_mesh_uniform& m = h.meshes[i];
        Quad* r = head.data() + (lay.mesh_off + (size_t)i * MESH_REC_BYTES) / 16;
        memcpy(r, m.world_to_model, 64);
        memcpy(r + 4, m.model_to_world, 64);
        const uint32_t flags = (is_glass(m) ? DMESH_GLASS : 0u) | (h.mg[i].deep ? DMESH_DEEP : 0u);
        r[8] = Quad{as_float(flags), as_float(h.mg[i].root_idx), as_float(h.mg[i].root_count), as_float(m.triangle_offset)};
        // S >= the largest absolute row sum of model_to_world's 3 x 3 part ([col][row]), C >= the largest
        // absolute translation component: in double, then rounded up (cross-mesh pruning's error terms)
        double S = 0.0, C = 0.0;
        for (int row = 0; row < 3; ++row) {
            const double rs = std::fabs((double)m.model_to_world[0][row]) + std::fabs((double)m.model_to_world[1][row]) + std::fabs((double)m.model_to_world[2][row]);
            if (!(rs <= S)) S = rs;  // (NaN sticks)
            const double tc = std::fabs((double)m.model_to_world[3][row]);
            if (!(tc <= C)) C = tc;
        }
        auto up = [](double d) { float f = (float)d; if ((double)f < d) f = std::nextafter(f, INFINITY); return f; };
        r[9] = Quad{as_float(h.mg[i].wide_base), up(S), up(C), 0.0f};
        r[10] = Quad{h.mg[i].box_lo[0], h.mg[i].box_hi[0], h.mg[i].box_lo[1], h.mg[i].box_hi[1]};
        r[11] = Quad{h.mg[i].box_lo[2], h.mg[i].box_hi[2], 0.0f, 0.0f};
        memcpy(head.data() + (lay.mat_off + (size_t)i * MATERIAL_BYTES) / 16, &m.material, MATERIAL_BYTES);
    }
    if (!h.tlas.empty()) memcpy(head.data() + lay.tlas_off / 16, h.tlas.data(), h.tlas.size() * sizeof(Rec2));
    if (!h.forest.empty()) memcpy(head.data() + lay.forest_off / 16, h.forest.data(), h.forest.size() * sizeof(ForestEntry));
    for (size_t k = 0; k < h.items.size(); ++k) {
        const Item& it = h.items[k];
        const bool single = (it.kind & (ITEM_TLAS | ITEM_FOREST)) == 0;
        head[lay.item_off / 16 + 2 * k] = Quad{as_float(it.kind), as_float(it.a), as_float(it.b), as_float(single ? h.mg[it.a].wide_base : it.n)};
        if (single) head[lay.item_off / 16 + 2 * k + 1] = head[(lay.mesh_off + (size_t)it.a * MESH_REC_BYTES) / 16 + 8];
    }
    for (uint32_t i = 0; i < n_spheres; ++i) {
        head[(lay.sphere_off + (size_t)i * SPHERE_BYTES) / 16] = Quad{spheres[i].pos[0], spheres[i].pos[1], spheres[i].pos[2], spheres[i].radius};
        memcpy(head.data() + (lay.mat_off + (size_t)(n_meshes + i) * MATERIAL_BYTES) / 16, &spheres[i].material, MATERIAL_BYTES);
    }
}

}  // namespace

int pack_instances(const PackOptions& opt, const SceneGeom& g, const rt_sphere* spheres, uint32_t n_spheres, const rt_mesh_uniform* meshes,
                   uint32_t n_meshes, InstanceFacts& out, std::vector<Quad>& head, std::string& why) {
    const std::vector<MeshGeom>& mg = g.mesh;
    out = InstanceFacts{};
    // ---- mesh-loop h.items and top-level trees -------------------------------------
    // Within a run, meshes with an internal, non-deep root whose box provably contains its
    // children's go under a TLAS when there are enough of them; every other mesh is a
    // single item.  (Visit order is free: rt_kernel.hip breaks distance ties by mesh index.)
    const std::vector<Run> runs = transform_runs(meshes, n_meshes);
    Head h{mg, meshes, {}, {}, {}};
    // per run: the meshes that go under its top-level tree (none when there are fewer than tlas_min of them)
    std::vector<std::vector<uint32_t>> grouped_of(runs.size());
    bool any_tlas = false;
    for (size_t r = 0; r < runs.size() && opt.tlas; ++r) {
        for (uint32_t i = runs[r].begin; i < runs[r].end; ++i)
            if (tree_ok(mg, i)) grouped_of[r].push_back(i);
        if (grouped_of[r].size() < (size_t)opt.tlas_min) grouped_of[r].clear();
        any_tlas = any_tlas || !grouped_of[r].empty();
    }
    // The few-mesh kernels walk forest h.items, run two-leaf meshes as straight-line code and defer a big mesh: none of
    // that when the scene gets a top-level tree anywhere or has enough meshes for automatic root-box culling (the
    // many-mesh kernels, which prune and order the loop instead).
    const bool few_mesh = !any_tlas && n_meshes < 16;
    // meshes whose root has two leaf children run as straight-line code in the few-mesh kernels (ITEM_FLAT2)
    auto is_flat2 = [&](uint32_t i) { return opt.flat2 && few_mesh && mg[i].flat2_shape; };
    auto in = [](const std::vector<uint32_t>& sorted, uint32_t i) { return std::binary_search(sorted.begin(), sorted.end(), i); };
    for (size_t r = 0; r < runs.size(); ++r) {
        const uint32_t i0 = runs[r].begin, i1 = runs[r].end;
        const std::vector<uint32_t>& grouped = grouped_of[r];
        // the other meshes of the run with an internal, non-deep root (and the run's
        // model_to_world as well) form a forest when there are at least two of them
        std::vector<uint32_t> forest;
        for (uint32_t i = i0; i < i1 && opt.forest && few_mesh; ++i)
            if (!in(grouped, i) && mg[i].root_count == 0 && !mg[i].deep && !is_flat2(i) &&
                memcmp(meshes[i].model_to_world, meshes[i0].model_to_world, 64) == 0)
                forest.push_back(i);
        if (forest.size() < 2) forest.clear();
        bool first = true;
        auto flag = [&]() { uint32_t f = first ? ITEM_NEW_XFORM : 0u; first = false; return f; };
        for (uint32_t i = i0; i < i1; ++i)
            if (!in(grouped, i) && !in(forest, i)) h.items.push_back(Item{flag() | (is_flat2(i) ? ITEM_FLAT2 : 0u), i, i0, 1});
        for (size_t f0 = 0; f0 < forest.size(); f0 += FOREST_MAX_MEMBERS) {
            const size_t f1 = std::min(forest.size(), f0 + (size_t)FOREST_MAX_MEMBERS);
            h.items.push_back(Item{ITEM_FOREST | flag(), (uint32_t)h.forest.size(), i0, (uint32_t)(f1 - f0)});
            for (size_t f = f0; f < f1; ++f) {
                const uint32_t i = forest[f];
                const MeshGeom& r = mg[i];
                const uint32_t fl = (is_glass(meshes[i]) ? DMESH_GLASS : 0u) | (root_box_ok(r) ? FOREST_CULLABLE : 0u);
                h.forest.push_back(ForestEntry{{{as_float(r.root_idx), as_float(i), as_float(fl), 0.0f},
                                                {r.box_lo[0], r.box_hi[0], r.box_lo[1], r.box_hi[1]}, {r.box_lo[2], r.box_hi[2], 0.0f, 0.0f}}});
            }
        }
        if (!grouped.empty()) {
            std::vector<uint32_t> ms = grouped;
            h.max_depth = 1 + ceil_log2(ms.size()) + 6;
            const Child root = build_tree(h, ms, 0, ms.size(), 1);
            h.items.push_back(Item{ITEM_TLAS | flag(), root.idx, i0, (uint32_t)grouped.size()});
        }
    }
    if (!h.tlas.empty()) renumber_trees(h);
    if (!few_mesh) mark_prune_and_order(h);
    // (one entry is always there: the many-mesh kernels, which the debug views use too,
    // run single meshes through the same stack)
    out.tlas_entries = h.tlas.empty() ? 1u : h.depth + 2u;
    out.has_tlas = !h.tlas.empty();
    if (few_mesh) choose_deferred(h, opt, out);
    if (!layout_head(h, g, n_meshes, n_spheres, out.lay)) { why = "scene larger than 4 GiB"; return RT_ERR_CAPACITY; }
    write_head(h, out.lay, spheres, n_spheres, n_meshes, head);
    out.n_items = (uint32_t)h.items.size();
    out.n_tlas_records = (uint32_t)h.tlas.size();
    out.n_forest_entries = (uint32_t)h.forest.size();
    out.has_forest = !h.forest.empty();
    out.plain_materials = n_spheres == 0;
    for (uint32_t i = 0; i < n_meshes && out.plain_materials; ++i)
        out.plain_materials = !is_glass(meshes[i]) && !(meshes[i].material.flag == RT_MATERIAL_TEXTURE && meshes[i].material.diffuse_index != -1);
    return RT_OK;
}

}  // namespace rt2
