"""BVH refit on the host (include/rt_abi.h: rt_refit_bvh, rt_scene_set_mesh_vertices, rt_scene_triangle_order).  No GPU:
a refit of unchanged vertices gives back the builder's nodes value for value; after deformations every node box is the
header's fold over the triangles under it, bit for bit; topology and unselected meshes stay; refusals change nothing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ASSETS, ROOT

DATA = os.path.join(ROOT, "tests", "data")
F32 = np.float32
FMAX = np.finfo(F32).max
BOX = ("aabb_min", "aabb_max")
TOPO = ("left", "right", "first", "count")


def _scene(rt, name, quality):
    from ray_tracer_2_amd import scenes
    if name == "sponza_standin":
        sc = scenes.sponza_standin(24)
        sc.build(quality)
        return sc
    sc = rt.Scene.from_name(name, ASSETS if name in ("cornell_box", "texture_test") else DATA)
    sc.build(quality)
    return sc


# ---- the header's box rule, in numpy ----------------------------------------------------------------------------------
def bmin(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    eq = np.where(np.signbit(a), a, b)
    nan = np.where(np.isnan(a), b, a)
    return np.where(a < b, a, np.where(b < a, b, np.where(a == b, eq, nan))).astype(F32)


def bmax(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    eq = np.where(np.signbit(a), b, a)
    nan = np.where(np.isnan(a), b, a)
    return np.where(a > b, a, np.where(b > a, b, np.where(a == b, eq, nan))).astype(F32)


def fold(tris):
    """(lo, hi) of triangles in array order from (+FLT_MAX, -FLT_MAX)."""
    lo, hi = np.full(3, FMAX, F32), np.full(3, -FMAX, F32)
    for t in tris:
        lo = bmin(lo, bmin(t["v1"], bmin(t["v2"], t["v3"])))
        hi = bmax(hi, bmax(t["v1"], bmax(t["v2"], t["v3"])))
    return lo, hi


def under(nodes, base, n):
    """Triangle indices (local) of the leaves under node base + n, in leaf pre-order."""
    nd = nodes[base + n]
    if nd["count"] > 0:
        return list(range(nd["first"], nd["first"] + nd["count"]))
    return under(nodes, base, nd["left"]) + under(nodes, base, nd["right"])


def mesh_nodes(meshes, nodes, i):
    """Absolute indices of the nodes mesh i's root reaches."""
    base, out, st = int(meshes[i]["node_offset"]), [], [0]
    while st:
        n = st.pop()
        out.append(base + n)
        if nodes[base + n]["count"] == 0:
            st += [int(nodes[base + n]["left"]), int(nodes[base + n]["right"])]
    return out


def check_boxes(arrays, i):
    """Every node box of mesh i == the numpy fold over the triangles under it, bit for bit."""
    m = arrays.meshes[i]
    tris = arrays.triangles[int(m["triangle_offset"]):int(m["triangle_offset"]) + int(m["triangles"])]
    base = int(m["node_offset"])
    for a in mesh_nodes(arrays.meshes, arrays.nodes, i):
        lo, hi = fold(tris[under(arrays.nodes, base, a - base)])
        got = arrays.nodes[a]
        assert got["aabb_min"].tobytes() == lo.tobytes() and got["aabb_max"].tobytes() == hi.tobytes(), (i, a)


SCENES = ("cornell_box", "texture_test", "room", "metal", "balls", "sponza_standin")


@pytest.mark.parametrize("quality", [0, 1])
@pytest.mark.parametrize("name", SCENES)
def test_refit_of_unchanged_vertices_gives_the_builders_nodes(rt, name, quality):
    sc = _scene(rt, name, quality)
    a = rt.SceneArrays.from_scene(sc)
    before = a.nodes.copy()
    a.refit_bvh(0, len(a.triangles))
    for f in TOPO:
        assert np.array_equal(a.nodes[f], before[f])
    for f in BOX:   # value for value (the builder's zeros may have either sign)
        assert np.array_equal(a.nodes[f], before[f]), (name, quality, np.flatnonzero((a.nodes[f] != before[f]).any(1))[:8])
    for i in range(len(a.meshes)):
        check_boxes(a, i)


def deformed(v, rng, specials=True):
    v = v.copy()
    v[:, :3] += rng.normal(0, 0.05, (len(v), 3)).astype(F32)
    v[:, 3:6] = rng.normal(0, 1, (len(v), 3)).astype(F32)
    if specials and len(v) >= 8:
        k = rng.choice(len(v), 8, replace=False)
        v[k[0], 0], v[k[1], 1], v[k[2], 2] = F32(0.0), F32(-0.0), F32(-0.0)
        v[k[3], 0], v[k[4], 1] = np.inf, -np.inf
        v[k[5], 2] = np.nan
        v[k[6], :3] = np.nan
        v[k[7], :3] = (F32(-0.0), F32(0.0), F32(-0.0))
    return v


def packed_from(vertices, indices, order):
    """The packed triangles of a mesh in BVH order: vertices[indices[3 * order + k]]."""
    p = np.zeros(len(order), _abi().TRI_DTYPE)
    for k, key in enumerate(("1", "2", "3")):
        vv = vertices[indices[3 * order.astype(np.int64) + k]]
        p["v" + key], p["n" + key] = vv[:, :3], vv[:, 3:6]
    p["uv10"], p["uv11"] = vertices[indices[3 * order], 6], vertices[indices[3 * order], 7]
    p["uv20"], p["uv21"] = vertices[indices[3 * order + 1], 6], vertices[indices[3 * order + 1], 7]
    p["uv30"], p["uv31"] = vertices[indices[3 * order + 2], 6], vertices[indices[3 * order + 2], 7]
    return p


def _abi():
    from ray_tracer_2_amd import _abi
    return _abi


@pytest.mark.parametrize("quality", [0, 1])
@pytest.mark.parametrize("name", ["cornell_box", "room", "sponza_standin"])
def test_set_mesh_vertices_repacks_and_refits_one_mesh(rt, name, quality):
    sc = _scene(rt, name, quality)
    a0 = rt.SceneArrays.from_scene(sc)
    raw = sc.raw_meshes()
    rng = np.random.RandomState(3)
    i = len(raw) // 2
    v = deformed(raw[i][1], rng)
    sc.set_mesh_vertices(i, v)
    b = rt.SceneArrays.from_scene(sc)
    assert np.array_equal(b.meshes.view(np.uint8), a0.meshes.view(np.uint8))
    for f in TOPO:
        assert np.array_equal(b.nodes[f], a0.nodes[f])
    m = b.meshes[i]
    t0, t1 = int(m["triangle_offset"]), int(m["triangle_offset"]) + int(m["triangles"])
    want = packed_from(v, raw[i][2], sc.triangle_order(i))
    assert b.triangles[t0:t1].tobytes() == want.tobytes()
    # only mesh i's triangles and nodes changed
    assert b.triangles[:t0].tobytes() == a0.triangles[:t0].tobytes() and b.triangles[t1:].tobytes() == a0.triangles[t1:].tobytes()
    mine = set(mesh_nodes(b.meshes, b.nodes, i))
    others = np.array(sorted(set(range(len(b.nodes))) - mine), np.int64)
    assert b.nodes[others].tobytes() == a0.nodes[others].tobytes()
    check_boxes(b, i)
    assert sc.raw_meshes()[i][1].tobytes() == v.tobytes()
    # the arrays route gives the same nodes
    c = rt.SceneArrays(a0.uniform, a0.spheres, a0.meshes, a0.triangles.copy(), a0.nodes.copy())
    c.refit_bvh(t0, t1 - t0, want)
    assert c.nodes.tobytes() == b.nodes.tobytes() and c.triangles.tobytes() == b.triangles.tobytes()


def test_triangle_order_is_a_permutation_that_packs_the_triangles(rt):
    sc = _scene(rt, "sponza_standin", 1)
    a = rt.SceneArrays.from_scene(sc)
    for i, (_l, v, idx, _t, _m) in enumerate(sc.raw_meshes()):
        order = sc.triangle_order(i)
        assert sorted(order.tolist()) == list(range(len(idx) // 3))
        m = a.meshes[i]
        got = a.triangles[int(m["triangle_offset"]):int(m["triangle_offset"]) + int(m["triangles"])]
        assert got.tobytes() == packed_from(v, idx, order).tobytes()


@pytest.mark.parametrize("name", ["cornell_box", "sponza_standin"])
def test_random_deformations_of_every_mesh(rt, name):
    sc = _scene(rt, name, 1)
    rng = np.random.RandomState(11)
    for rep in range(2):
        for i, (_l, v, _idx, _t, _m) in enumerate(sc.raw_meshes()):
            sc.set_mesh_vertices(i, deformed(v, rng, specials=(i % 3 == rep)))
    b = rt.SceneArrays.from_scene(sc)
    for i in range(len(b.meshes)):
        check_boxes(b, i)
    # a mesh with a NaN vertex keeps NaN-free boxes
    assert not np.isnan(b.nodes["aabb_min"]).any() and not np.isnan(b.nodes["aabb_max"]).any()


def test_all_nan_leaf_keeps_the_empty_box(rt):
    sc = rt.Scene()
    v = np.zeros((3, 8), F32)
    v[:, :3] = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
    sc.add_mesh_from_data(v, [0, 1, 2])
    sc.build(1)
    v[:, :3] = np.nan
    sc.set_mesh_vertices(0, v)
    n = rt.SceneArrays.from_scene(sc).nodes[0]
    assert np.all(n["aabb_min"] == FMAX) and np.all(n["aabb_max"] == -FMAX)


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_wrong_vertex_count_is_refused(rt):
    sc = _scene(rt, "cornell_box", 1)
    a0 = rt.SceneArrays.from_scene(sc)
    v = sc.raw_meshes()[2][1]
    with pytest.raises(rt.RtError) as e:
        sc.set_mesh_vertices(2, v[:-1])
    assert e.value.code == -1 and "vertices" in str(e.value)
    with pytest.raises(rt.RtError):
        sc.set_mesh_vertices(99, v)
    a1 = rt.SceneArrays.from_scene(sc)
    assert a1.triangles.tobytes() == a0.triangles.tobytes() and a1.nodes.tobytes() == a0.nodes.tobytes()


def test_a_partial_mesh_range_is_refused(rt):
    a = rt.SceneArrays.from_scene(_scene(rt, "cornell_box", 1))
    nodes0 = a.nodes.copy()
    m = a.meshes[1]
    with pytest.raises(rt.RtError) as e:
        a.refit_bvh(int(m["triangle_offset"]) + 1, int(m["triangles"]) - 1)
    assert e.value.code == -1 and "mesh 1" in str(e.value)
    with pytest.raises(rt.RtError) as e:
        a.refit_bvh(0, len(a.triangles) + 1)
    assert e.value.code == -1
    assert a.nodes.tobytes() == nodes0.tobytes()


def test_aliased_node_ranges_are_refused(rt):
    a = rt.SceneArrays.from_scene(_scene(rt, "cornell_box", 1))
    meshes = a.meshes.copy()
    j = len(meshes) - 1
    meshes[0]["node_offset"] = meshes[j]["node_offset"]   # mesh 0 walks mesh j's nodes over other triangles
    assert meshes[0]["triangle_offset"] != meshes[j]["triangle_offset"]
    b = rt.SceneArrays(a.uniform, a.spheres, meshes, a.triangles, a.nodes.copy())
    nodes0 = b.nodes.copy()
    with pytest.raises(rt.RtError) as e:
        b.refit_bvh(int(meshes[j]["triangle_offset"]), int(meshes[j]["triangles"]))
    assert e.value.code == -1 and f"mesh {j}" in str(e.value) and "mesh 0" in str(e.value)
    assert b.nodes.tobytes() == nodes0.tobytes()
    # the same node range with the same triangle_offset (an instance) is fine
    meshes[0]["triangle_offset"] = meshes[j]["triangle_offset"]
    b = rt.SceneArrays(a.uniform, a.spheres, meshes, a.triangles, a.nodes.copy())
    b.refit_bvh(int(meshes[j]["triangle_offset"]), int(meshes[j]["triangles"]))
    assert all(np.array_equal(b.nodes[f], nodes0[f]) for f in BOX + TOPO)


def test_unbuilt_and_disabled_scenes_are_refused(rt):
    from ray_tracer_2_amd import scenes
    sc = scenes.cornell_from_raw(rt.Scene.from_name("cornell_box", ASSETS).raw_meshes())   # (not built)
    with pytest.raises(rt.RtError) as e:
        sc.triangle_order(0)
    assert e.value.code == -1
    v = sc.raw_meshes()[1][1]
    sc.set_mesh_vertices(1, v + F32(0.5))   # (unbuilt: only the mesh data changes)
    assert np.array_equal(sc.raw_meshes()[1][1], v + F32(0.5)) and sc.meshes().size == 0
    sc.build(2)   # Disabled: nodes, no packed triangles
    a0 = rt.SceneArrays.from_scene(sc)
    with pytest.raises(rt.RtError) as e:
        sc.set_mesh_vertices(1, v)
    assert e.value.code == -1 and "Disabled" in str(e.value)
    assert np.array_equal(sc.raw_meshes()[1][1], v + F32(0.5))
    assert rt.SceneArrays.from_scene(sc).nodes.tobytes() == a0.nodes.tobytes()


COW_DRIVER = r'''
#include <cstdio>
#include "ray_tracer_2_amd/csrc/host/scene.h"
using namespace rt2;
int main() {
    Scene s;
    MeshInstance mi;
    mi.data = std::make_shared<MeshData>();
    for (int k = 0; k < 6; ++k) {
        Vertex v;
        v.pos = {float(k % 3), float(k / 3), float(k % 2)};
        mi.data->vertices.push_back(v);
    }
    mi.data->indices = {0, 1, 2, 3, 4, 5, 0, 2, 4};
    mi.material = material_uniform_default();
    s.meshes.push_back(mi);
    s.meshes.push_back(mi);  // a second instance sharing the mesh data
    s.build_per_mesh(Quality::High);
    std::vector<rt_packed_triangle> tri0(s.triangles.begin(), s.triangles.begin() + 3);
    std::vector<rt_node> nodes0(s.nodes.begin(), s.nodes.begin() + s.mesh_uniforms[1].node_offset);
    std::vector<Vertex> moved = mi.data->vertices;
    for (Vertex& v : moved) v.pos.y += 2.0f;
    std::string err;
    if (s.set_mesh_vertices(1, moved, err) != RT_OK) { printf("refused: %s\n", err.c_str()); return 1; }
    bool ok = s.meshes[0].data != s.meshes[1].data && s.meshes[0].data->vertices[0].pos.y == 0.0f &&
              s.meshes[1].data->vertices[0].pos.y == 2.0f && mi.data.use_count() == 2 &&
              memcmp(tri0.data(), s.triangles.data(), 3 * sizeof(rt_packed_triangle)) == 0 &&
              memcmp(nodes0.data(), s.nodes.data(), nodes0.size() * sizeof(rt_node)) == 0 &&
              s.triangles[3].v1[1] >= 2.0f && s.nodes[s.mesh_uniforms[1].node_offset].aabb_min[1] == 2.0f;
    printf(ok ? "cow ok\n" : "cow FAILED\n");
    return ok ? 0 : 1;
}
'''


def test_copy_on_write_of_shared_mesh_data(rt, tmp_path):
    """Two instances share one MeshData (the C++ Scene allows it): moving one instance's vertices leaves the other's
    mesh data, packed triangles and nodes as they were."""
    from ray_tracer_2_amd import lib
    src = tmp_path / "cow.cpp"
    src.write_text(COW_DRIVER.replace("#include <cstdio>", "#include <cstdio>\n#include <cstring>"))
    exe = tmp_path / "cow"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", ROOT, "-I", os.path.join(ROOT, "include"), str(src),
                    "-L", os.path.dirname(lib.LIB_PATH), "-lrt2_mi355x", "-Wl,-rpath," + os.path.dirname(lib.LIB_PATH),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "cow ok" in out.stdout, out.stdout + out.stderr


def test_the_refit_symbols_are_exported_with_the_header_signatures(rt):
    import re
    from ray_tracer_2_amd import lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rt_abi.h")).read(), flags=re.S)
    protos = {n: len([x for x in args.split(",") if x.strip()])
              for n, args in re.findall(r"\b(rt_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S)}
    L = rt.load()
    syms = subprocess.run(["nm", "-D", "--defined-only", lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in syms.splitlines()}
    for name in ("rt_refit_bvh", "rt_refit_triangles", "rt_refit_built_scene", "rt_scene_set_mesh_vertices",
                 "rt_scene_triangle_order"):
        assert name in protos and name in lib.EXPORTS and name in exported, name
        assert len(getattr(L, name).argtypes) == protos[name] and getattr(L, name).restype is C.c_int, name
    from ray_tracer_2_amd import _abi as A
    assert A.REFIT_HOST_MEMORY == 1
