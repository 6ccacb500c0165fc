"""BVH refit on the device (include/rt_abi.h: rt_refit_triangles, rt_refit_built_scene).  Every check starts from
update_buffers(A) followed by a refit to A', and compares the handle with a fresh one given update_buffers(A'), where A''s
nodes come from rt_refit_bvh (SceneArrays.refit_bvh): the blob's bytes and SceneLayout (test library: rt_test_scene_blob),
the launch shape, the image against the oracle of A' bit for bit, and ray queries.  Host and torch device input (the
latter in a process of its own), one mesh of many and all meshes, a resized head, refits between instance updates, refits
with frames in flight, and refusals."""
import os

import numpy as np
import pytest

import _ray_families as RF
import test_gpu_scene_edits as E
from conftest import ASSETS
from ray_tracer_2_amd import _abi as A

pytestmark = pytest.mark.gpu
F32 = np.float32
W, H = E.W, E.H
LIBRARY = ("cornell", "room", "sponza200", "dragon")
FAMILIES = ("tlas7", "tlas8", "tlas9", "leaf127", "leaf128", "height30", "height31", "height32", "height33")
SCENES = LIBRARY + FAMILIES
_cache = {}


def scene(rt, name):
    if name not in _cache:
        _cache[name] = E.scene(rt, name) if name in LIBRARY else RF.scene(rt, name)
    return _cache[name]


def arrays_with(a, meshes=None, triangles=None, nodes=None):
    """A copy of `a` that owns its mesh, triangle and node arrays."""
    u = A.SceneUniform.from_buffer_copy(bytes(a.uniform))
    m = (a.meshes if meshes is None else meshes).copy()
    return type(a)(u, a.spheres.copy(), m, (a.triangles if triangles is None else triangles).copy(),
                   (a.nodes if nodes is None else nodes).copy(), a.textures)


def mesh_range(a, i0, i1):
    """[first, first + n): the triangles of meshes i0 .. i1 - 1 (consecutive in the array)."""
    m = a.meshes[i0:i1]
    first = int(m["triangle_offset"].min())
    return first, int((m["triangle_offset"] + m["triangles"]).max()) - first


def moved(a, first, n, seed, scale=0.03):
    """Triangles [first, first + n) of `a` with every vertex moved by noise of `scale` times the range's extent, plus a
    shift of the whole range (new normals too): what a skinned or simulated mesh would send."""
    rng = np.random.RandomState(seed)
    t = a.triangles[first:first + n].copy()
    if n == 0:
        return t
    pts = np.concatenate([t["v1"], t["v2"], t["v3"]])
    ext = F32(np.max(pts.max(0) - pts.min(0)))
    shift = rng.normal(0, 0.5 * scale, 3).astype(F32) * ext
    for k in ("v1", "v2", "v3"):
        t[k] = (t[k] + rng.normal(0, scale, t[k].shape).astype(F32) * ext + shift).astype(F32)
    for k in ("n1", "n2", "n3"):
        t[k] = (t[k] + rng.normal(0, 0.1, t[k].shape)).astype(F32)
    return t


def refitted(a, first, new):
    return arrays_with(a).refit_bvh(first, len(new), new)


def check_equal(rt, oracle, T, F, b, name, what):
    blob, lay, _ = T.scene_blob()
    blob_f, lay_f, words_f = E.fresh(rt, F, b)
    assert np.array_equal(lay, lay_f), (what, lay.tolist(), lay_f.tolist())
    assert np.array_equal(blob, blob_f), (what, np.flatnonzero(blob != blob_f)[:8])
    T.render(E.params(rt, 0))
    assert E.launch_words(T) == words_f, what
    T.render(E.params(rt, 1))
    assert E.same_image(T.read_image(W, H), E.oracle_frames(rt, oracle, b, name), name), what
    ro, rd = E.rays(b, n=2000)
    got = T.trace_rays(ro, rd)
    want = F.trace_rays(ro, rd)
    assert got.tobytes() == want.tobytes(), what
    occ_t, occ_f = T.occluded(ro, rd, 2.5), F.occluded(ro, rd, 2.5)
    assert np.array_equal(occ_t, occ_f), what


@pytest.fixture(scope="module")
def T(rt):
    t = rt.RayTracer(device=0, max_width=W, max_height=H, lib=rt.load_test())
    yield t
    t.close()


@pytest.fixture(scope="module")
def F(rt):
    t = rt.RayTracer(device=0, max_width=W, max_height=H, lib=rt.load_test())
    yield t
    t.close()


def which_meshes(a, which):
    if which == "all" or len(a.meshes) == 1:
        return 0, len(a.meshes)
    big = int(np.argmax(a.meshes["triangles"]))   # (the dragon in the dragon stand-in: the deferred walks)
    return big, big + 1


@pytest.mark.parametrize("which", ["one", "all"])
@pytest.mark.parametrize("name", SCENES)
def test_refit_equals_a_fresh_upload(rt, oracle, T, F, name, which):
    a = scene(rt, name)
    first, n = mesh_range(a, *which_meshes(a, which))
    new = moved(a, first, n, seed=len(name) * 7 + n)
    b = refitted(a, first, new)
    T.load_scene(a)
    _, lay_a, ptr_a = T.scene_blob()
    T.refit_triangles(new, first)
    _, lay, ptr = T.scene_blob()
    if lay[1] == lay_a[1]:
        assert ptr == ptr_a, "a refit that keeps the head's size reallocated the blob"
    check_equal(rt, oracle, T, F, b, name, (name, which))


def test_device_input():
    """Triangles in a torch tensor on the device (tests/_refit_device_path.py, a process of its own that imports torch
    first): the same handle as a fresh upload, and device refits between pipelined frames give the host refits' image."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "_refit_device_path.py")],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "device input ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_a_refit_that_resizes_the_head(rt, oracle, T, F):
    """tlas8: mesh 0's uploaded root box does not contain its children (a foreign BVH), so only 7 meshes of the run can go
    under a tree -- fewer than tlas_min: no tree.  Its refit makes the box the union: 8 meshes, a tree, a longer head."""
    a0 = scene(rt, "tlas8")
    nodes = a0.nodes.copy()
    r = int(a0.meshes[0]["node_offset"])
    nodes[r]["aabb_max"] = nodes[r]["aabb_max"] - F32(0.05)
    a = arrays_with(a0, nodes=nodes)
    first, n = mesh_range(a, 0, 1)
    new = moved(a, first, n, seed=5)
    b = refitted(a, first, new)
    T.load_scene(a)
    _, lay_a, ptr_a = T.scene_blob()
    T.refit_triangles(new, first)
    _, lay, ptr = T.scene_blob()
    assert lay[1] != lay_a[1] and ptr != ptr_a
    check_equal(rt, oracle, T, F, b, "tlas8", "resize")


@pytest.mark.parametrize("name", ["cornell", "sponza200", "dragon"])
def test_refits_interleaved_with_instance_updates(rt, oracle, T, F, name):
    a = scene(rt, name)
    T.load_scene(a)
    lo, hi = which_meshes(a, "one")
    f1, n1 = mesh_range(a, lo, hi)
    new1 = moved(a, f1, n1, seed=1)
    b = refitted(a, f1, new1)
    T.refit_triangles(new1, f1)
    _, c = E.edit_pair(rt, b, "split")     # (an instance edit over the refitted geometry)
    c = arrays_with(c)
    c.meshes[0]["material"]["color"] = (0.25, 0.5, 0.75, 1.0)
    T.update_instances(c)
    f2, n2 = mesh_range(c, 0, len(c.meshes))
    new2 = moved(c, f2, n2, seed=2)
    d = refitted(c, f2, new2)
    T.refit_triangles(new2, f2)
    check_equal(rt, oracle, T, F, d, name, "interleaved")


@pytest.mark.parametrize("name", ["cornell", "dragon"])
def test_refits_with_frames_in_flight_render_the_geometry_of_their_call(rt, oracle, T, name):
    """Eight refits, each followed by a render call that is not waited for (the automatic pipeline): the accumulated image
    is the oracle's with frame f of geometry f, so every frame sampled the geometry it was asked under."""
    a = scene(rt, name)
    lo, hi = which_meshes(a, "one")
    first, n = mesh_range(a, lo, hi)
    T.load_scene(a)
    T.reset_timing()
    geoms = []
    cur = a
    for f in range(8):
        new = moved(a, first, n, seed=100 + f, scale=0.01 * (1 + f % 3))
        cur = refitted(cur, first, new)
        geoms.append(cur)
        T.refit_triangles(new, first)
        T.render(E.params(rt, f))
    img = T.read_image(W, H)
    acc = None
    for f, g in enumerate(geoms):
        acc = E.oracle_frames(rt, oracle, g, name, n=1, image=acc, first=f)
    assert E.same_image(img, acc, name)


def test_refusals_leave_the_blob_unchanged(rt, oracle, T, F):
    a = scene(rt, "cornell")
    T.load_scene(a)
    blob0, lay0, ptr0 = T.scene_blob()
    m = a.meshes[1]
    first, n = int(m["triangle_offset"]), int(m["triangles"])
    new = moved(a, first, n, seed=9)
    with pytest.raises(rt.RtError) as e:   # part of a mesh
        T.refit_triangles(new[1:], first + 1)
    assert e.value.code == -1 and "mesh 1" in str(e.value)
    with pytest.raises(rt.RtError) as e:   # past the end
        T.refit_triangles(new, len(a.triangles) - n + 1)
    assert e.value.code == -1
    assert T._L.rt_refit_triangles(T._h, new.ctypes.data, first, n, 4 | A.REFIT_HOST_MEMORY) == -1   # unknown flag
    T.set_option("max_device_mb", 1)
    try:
        big = scene(rt, "dragon")
        T.load_scene(big)
        bblob, blay, bptr = T.scene_blob()
        bf, bn = mesh_range(big, 0, len(big.meshes))
        with pytest.raises(rt.RtError) as e:   # the scratch does not fit the cap
            T.refit_triangles(moved(big, bf, bn, seed=3), bf)
        assert e.value.code == -8   # RT_ERR_OUT_OF_MEMORY
        blob, lay, ptr = T.scene_blob()
        assert np.array_equal(blob, bblob) and np.array_equal(lay, blay) and ptr == bptr
    finally:
        T.set_option("max_device_mb", 0)
    # aliased node ranges: mesh 0 walks the last mesh's nodes over other triangles
    meshes = a.meshes.copy()
    j = len(meshes) - 1
    meshes[0]["node_offset"] = meshes[j]["node_offset"]
    al = arrays_with(a, meshes=meshes)
    T.load_scene(al)
    blob0, lay0, ptr0 = T.scene_blob()
    jf, jn = int(meshes[j]["triangle_offset"]), int(meshes[j]["triangles"])
    with pytest.raises(rt.RtError) as e:
        T.refit_triangles(moved(al, jf, jn, seed=4), jf)
    assert e.value.code == -1 and f"mesh {j}" in str(e.value) and "mesh 0" in str(e.value)
    blob, lay, ptr = T.scene_blob()
    assert np.array_equal(blob, blob0) and np.array_equal(lay, lay0) and ptr == ptr0
    T.render(E.params(rt, 0))
    T.render(E.params(rt, 1))
    assert E.same_image(T.read_image(W, H), E.oracle_frames(rt, oracle, al, "cornell"), "cornell")
    t = rt.RayTracer(device=0, max_width=16, max_height=16)
    try:
        with pytest.raises(rt.RtError) as e:
            t.refit_triangles(new, first)
        assert e.value.code == -4
    finally:
        t.close()


def test_refit_built_scene_after_set_mesh_vertices(rt, oracle, T, F):
    """The scene route: Scene.set_mesh_vertices (repack + host refit), then refit_built_scene sends that mesh's triangles;
    the handle equals a fresh upload of the scene's arrays."""
    sc = rt.Scene.from_name("cornell_box", ASSETS)
    T.load_built_scene(sc)
    raw = sc.raw_meshes()
    rng = np.random.RandomState(4)
    for i in (2, 3):
        v = raw[i][1].copy()
        v[:, :3] += rng.normal(0, 0.02, (len(v), 3)).astype(F32)
        sc.set_mesh_vertices(i, v)
    T.refit_built_scene(sc, 2, 2)
    b = rt.SceneArrays.from_scene(sc)
    check_equal(rt, oracle, T, F, b, "cornell", "built scene")
