"""Instance edits on an uploaded scene (include/rt_abi.h: rt_update_instances, rt_update_built_scene).  Every check starts
from update_buffers(A) followed by update_instances(B), and compares the handle with a fresh one given update_buffers(B):
the blob's bytes and SceneLayout (test library: rt_test_scene_blob), the launch shape, the image against the oracle of B
bit for bit, and ray queries against oracle.intersect(B).  Also: sequences of updates, frames in flight across an
update, and errors that leave the scene as it was."""
import os

import numpy as np
import pytest

import _query_helpers as QH
from conftest import GOLDEN, ROOT, bits
from ray_tracer_2_amd import _abi as A
from ray_tracer_2_amd.ray_tracer import normalize3_f32

pytestmark = pytest.mark.gpu
DATA = os.path.join(ROOT, "tests", "data")
F32 = np.float32
W, H = 64, 40
BIG = ("sponza200", "dragon")
SCENES = ("cornell", "room", "metal", "texture_test") + BIG
EDITS = ("color", "glass", "unglass", "textured", "split", "run", "merge", "spheres", "sphere_removed")
MESHLESS, SPHERELESS = ("metal", "texture_test"), ("cornell", "dragon")   # (material edits go to sphere 0 of a meshless scene)
CASES = [(n, e) for n in SCENES for e in EDITS
         if not (n in MESHLESS and e in ("split", "run", "merge")) and not (n in SPHERELESS and e == "sphere_removed")]
LAUNCH_KEYS = ("lds_bytes_per_workgroup", "workgroups", "scene_in_lds", "many_mesh", "specialised", "one_wave_per_tile",
               "deferred_walks", "wavefront")   # (rt_last_launch words 0 - 3)
_cache = {}


def scene(rt, name):
    if name not in _cache:
        from ray_tracer_2_amd import scenes
        if name in ("cornell", "texture_test"):
            a = rt.SceneArrays.load(os.path.join(GOLDEN, f"{name}_scene.npz"))
        elif name in ("room", "metal"):
            a = rt.SceneArrays.from_scene(rt.Scene.from_name(name, DATA))
        elif name == "sponza200":
            a = rt.SceneArrays.from_scene(scenes.sponza_standin(200))
        else:   # BASELINE config 3 stand-in: the scene is read from global memory, the dragon's walks are deferred
            a = rt.SceneArrays.from_scene(scenes.cornell_dragon(scenes.load_raw_meshes(os.path.join(GOLDEN, "cornell_raw.npz")),
                                                                scenes.load_raw_meshes(os.path.join(GOLDEN, "dragon_raw.npz")),
                                                                subdivide=3))
        _cache[name] = a
    return _cache[name]


# ---- edits of scene arrays ------------------------------------------------------------------------------------------
def clone(a, meshes=None, spheres=None):
    u = A.SceneUniform.from_buffer_copy(bytes(a.uniform))
    m = a.meshes.copy() if meshes is None else meshes
    s = a.spheres.copy() if spheres is None else spheres
    u.spheres, u.meshes = len(s), len(m)
    return type(a)(u, s, m, a.triangles, a.nodes, a.textures)


def translated(m, d):
    """The mesh record `m` moved by d in world space: model_to_world's translation + d, world_to_model's - w2m(d)."""
    m = m.copy()
    d = np.asarray(d, np.float64)
    m2w = np.asarray(m["model_to_world"], np.float64)
    w2m = np.asarray(m["world_to_model"], np.float64)
    m2w[3, :3] += d
    w2m[3, :3] -= d[0] * w2m[0, :3] + d[1] * w2m[1, :3] + d[2] * w2m[2, :3]
    m["model_to_world"], m["world_to_model"] = m2w.astype(F32), w2m.astype(F32)
    return m


def runs(meshes):
    """Runs of consecutive meshes with bit-identical world_to_model (the blob's local spaces)."""
    out, i0 = [], 0
    for i in range(1, len(meshes) + 1):
        if i == len(meshes) or meshes[i]["world_to_model"].tobytes() != meshes[i0]["world_to_model"].tobytes():
            out.append((i0, i))
            i0 = i
    return out


GLASS = dict(color=(0.9, 0.95, 1, 1), flag=1, ior=1.45, smoothness=0.9, specular=0.8, absorption=(0.2, 0.1, 0.05, 0),
             absorption_strength=1.5)


def _mat(rt, **kw):
    return np.frombuffer(bytes(rt.material(**kw)), A.MATERIAL_DTYPE)[0]


def edit_pair(rt, a, edit):
    """(A, B): the scene before and after `edit` (A is `a` itself unless the edit needs another starting point)."""
    n = len(a.meshes)
    k = n // 2
    m = a.meshes.copy()
    if n == 0 and edit in ("color", "glass", "unglass", "textured"):   # the same edit of sphere 0's material
        s = a.spheres.copy()
        sb = s.copy()
        if edit == "color":
            sb[0]["material"]["color"] = (0.125, 0.75, 0.375, 1.0)
        elif edit == "textured":
            sb[0]["material"] = _mat(rt, flag=2, diffuse_index=0, smoothness=0.2, color=(0.5, 0.25, 0.125, 1))
        else:
            sb[0]["material"] = _mat(rt, **GLASS)
        return (clone(a, spheres=sb), a) if edit == "unglass" else (a, clone(a, spheres=sb))
    if edit == "color":
        m[k]["material"]["color"] = (0.125, 0.75, 0.375, 1.0)
        return a, clone(a, meshes=m)
    if edit in ("glass", "unglass"):   # the kernel kind flips (glass is not a plain material)
        m[k]["material"] = _mat(rt, **GLASS)
        return (a, clone(a, meshes=m)) if edit == "glass" else (clone(a, meshes=m), a)
    if edit == "textured":
        m[k]["material"] = _mat(rt, flag=2, diffuse_index=0, smoothness=0.2, color=(0.5, 0.25, 0.125, 1))
        return a, clone(a, meshes=m)
    if edit == "split":   # one mesh out of its run (a longer head: a new blob)
        r = max(runs(m), key=lambda r: r[1] - r[0])
        j = (r[0] + r[1]) // 2
        m[j] = translated(m[j], (0.0625, 0.03125, -0.125))
        return a, clone(a, meshes=m)
    if edit == "run":     # a whole run moved by one matrix (the head keeps its size: in place)
        r = max(runs(m), key=lambda r: r[1] - r[0])
        moved = translated(m[r[0]], (-0.09375, 0.0625, 0.046875))
        for j in range(r[0], r[1]):
            m[j]["model_to_world"], m[j]["world_to_model"] = moved["model_to_world"], moved["world_to_model"]
        return a, clone(a, meshes=m)
    if edit == "merge":   # two runs made identical
        far = translated(m[0], (0.25, 0.0, 0.125))
        for j in range(n):
            src = m[0] if j < k else far
            m[j]["model_to_world"], m[j]["world_to_model"] = src["model_to_world"], src["world_to_model"]
        b = m.copy()
        for j in range(k, n):
            b[j]["model_to_world"], b[j]["world_to_model"] = m[0]["model_to_world"], m[0]["world_to_model"]
        return clone(a, meshes=m), clone(a, meshes=b)
    if edit == "spheres":  # moved, resized, and one added
        s = a.spheres.copy()
        if len(s):
            s[0]["pos"] = np.asarray(s[0]["pos"]) + F32(0.125)
            s[0]["radius"] = s[0]["radius"] * F32(0.75)
        extra = np.zeros(1, A.SPHERE_DTYPE)
        extra[0]["pos"], extra[0]["radius"] = (0.25, 0.75, -0.5), 0.3125
        extra[0]["material"] = _mat(rt, color=(1, 0.5, 0.25, 1), emission_color=(1, 1, 1, 1), emission_strength=2.0)
        return a, clone(a, spheres=np.concatenate([s, extra]))
    if edit == "sphere_removed":
        return a, clone(a, spheres=a.spheres[:-1].copy())
    raise KeyError(edit)


# ---- handles and checks ---------------------------------------------------------------------------------------------
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


def params(rt, frames):
    return rt.make_params(W, H, 3, 2, skybox=1, frames=frames)


def rows_of(name):
    return np.arange(0, H, 5, dtype=np.uint32) if name in BIG else None


def oracle_frames(rt, oracle, arrays, name, n=2, image=None, first=0):
    acc = np.zeros((H, W, 4), F32) if image is None else image
    for f in range(first, first + n):
        acc, _ = oracle.render(params(rt, f), arrays, image=acc, rows=rows_of(name))
    return acc


def same_image(gpu, ref, name):
    r = rows_of(name)
    if r is not None:
        gpu, ref = gpu[r], ref[r]
    return np.array_equal(bits(gpu), bits(ref))


def launch_words(t):
    d = t.last_launch()
    return tuple(d[k] for k in LAUNCH_KEYS)


def rays(arrays, n=3000, seed=7):
    rng = np.random.RandomState(seed)
    c2w = arrays.uniform.camera.cam_to_world
    cam = np.array([c2w[3][r] for r in range(3)], F32)
    ro = (cam + rng.normal(0, 0.25, (n, 3))).astype(F32)
    rd = normalize3_f32(rng.normal(0, 1, (n, 3)).astype(F32))
    return ro, rd


def check_queries(oracle, t, arrays, what):
    ro, nd = rays(arrays)
    want, _ = QH.filtered_probe_words(oracle.intersect(arrays, ro, normalize3_f32(nd)), np.inf)
    got = QH.hits_as_probe_words(t.trace_rays(ro, nd))
    isf = np.zeros(12, bool)
    isf[1:10] = True
    nan = ((got & 0x7fffffff) > 0x7f800000) & ((want & 0x7fffffff) > 0x7f800000) & isf[None, :]
    bad = np.flatnonzero(((got != want) & ~nan).any(1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(got)} rays differ from oracle.intersect"


def fresh(rt, F, arrays):
    F.load_scene(arrays)
    blob, lay, _ = F.scene_blob()
    F.render(params(rt, 0))
    return blob, lay, launch_words(F)


@pytest.mark.parametrize("name,edit", CASES)
def test_update_equals_a_fresh_upload(rt, oracle, T, F, name, edit):
    a, b = edit_pair(rt, scene(rt, name), edit)
    T.load_scene(a)
    _, lay_a, ptr_a = T.scene_blob()
    T.update_instances(b)
    blob, lay, ptr = T.scene_blob()
    blob_f, lay_f, words_f = fresh(rt, F, b)
    assert np.array_equal(lay, lay_f), (name, edit, lay.tolist(), lay_f.tolist())
    assert np.array_equal(blob, blob_f), (name, edit, np.flatnonzero(blob != blob_f)[:8])
    # the tail keeps its sections (wide BVH records, triangle records), wherever it starts
    assert lay[2] - lay[1] == lay_a[2] - lay_a[1] and lay[3] - lay[2] == lay_a[3] - lay_a[2]
    if lay[1] == lay_a[1]:
        assert ptr == ptr_a, "an update that keeps the head's size reallocated the blob"
    if edit == "run":
        assert lay[1] == lay_a[1] and ptr == ptr_a
    if edit == "split" and name == "sponza200":
        assert lay[1] != lay_a[1]   # (the run's tree splits in two, and a single item joins: a new blob)
    T.render(params(rt, 0))
    assert launch_words(T) == words_f, (name, edit)
    T.render(params(rt, 1))
    img = T.read_image(W, H)
    assert same_image(img, oracle_frames(rt, oracle, b, name), name), (name, edit)
    check_queries(oracle, T, b, f"{name} {edit}")


@pytest.mark.parametrize("name", ["cornell", "sponza200", "dragon"])
def test_a_sequence_of_updates_equals_a_direct_upload(rt, oracle, T, F, name):
    a = scene(rt, name)
    _, b = edit_pair(rt, a, "split")
    _, c = edit_pair(rt, b, "spheres")
    c.meshes[0]["material"]["color"] = (0.25, 0.5, 0.75, 1.0)
    T.load_scene(a)
    T.update_instances(b)
    T.update_instances(c)
    blob, lay, _ = T.scene_blob()
    blob_f, lay_f, words_f = fresh(rt, F, c)
    assert np.array_equal(lay, lay_f) and np.array_equal(blob, blob_f)
    T.render(params(rt, 0))
    assert launch_words(T) == words_f
    T.render(params(rt, 1))
    assert same_image(T.read_image(W, H), oracle_frames(rt, oracle, c, name), name)


@pytest.mark.parametrize("frame_ahead", [-1, 8])
@pytest.mark.parametrize("name,edit", [("cornell", "color"), ("cornell", "split"), ("dragon", "glass")])
def test_frames_in_flight_render_the_scene_of_their_call(rt, oracle, T, name, edit, frame_ahead):
    """Pipelined calls (the automatic pipeline; frame_ahead = 8 renders frames ahead in batches), the update, more calls:
    the accumulated image is the oracle's with frames 0 - 4 of A and 5 - 9 of B, so every call sampled the scene it was
    made under, and no frame rendered ahead under A was blended after the update."""
    a, b = edit_pair(rt, scene(rt, name), edit)
    T.set_option("frame_ahead", frame_ahead)
    try:
        T.load_scene(a)
        T.reset_timing()
        for f in range(5):
            T.render(params(rt, f))
        T.update_instances(b)
        for f in range(5, 10):
            T.render(params(rt, f))
        img = T.read_image(W, H)
        print(name, edit, "frame_ahead", frame_ahead, "frames rendered ahead and never asked for:", T.stats().frames_speculative)
    finally:
        T.set_option("frame_ahead", -1)
    acc = oracle_frames(rt, oracle, a, name, n=5)
    acc = oracle_frames(rt, oracle, b, name, n=5, image=acc, first=5)
    assert same_image(img, acc, name)


def test_errors_change_nothing(rt, oracle, T):
    a = scene(rt, "cornell")
    T.load_scene(a)
    blob0, lay0, ptr0 = T.scene_blob()
    m = a.meshes.copy()
    m[1]["triangle_offset"] += 1
    with pytest.raises(rt.RtError) as e:
        T.update_instances(clone(a, meshes=m))
    assert e.value.code == -1 and "mesh 1" in str(e.value)
    with pytest.raises(rt.RtError) as e:
        T.update_instances(clone(a, meshes=a.meshes[:-1].copy()))
    assert e.value.code == -1 and "mesh count" in str(e.value)
    s = np.zeros(501, A.SPHERE_DTYPE)
    s["radius"] = 0.1
    with pytest.raises(rt.RtError) as e:
        T.update_instances(clone(a, spheres=s))
    assert e.value.code == -2
    u = A.SceneUniform.from_buffer_copy(bytes(a.uniform))
    u.spheres = 3
    assert T._L.rt_update_instances(T._h, u, None, 3, a.meshes.ctypes.data, len(a.meshes)) == -1
    blob, lay, ptr = T.scene_blob()
    assert np.array_equal(blob, blob0) and np.array_equal(lay, lay0) and ptr == ptr0
    T.render(params(rt, 0))
    T.render(params(rt, 1))
    assert same_image(T.read_image(W, H), oracle_frames(rt, oracle, a, "cornell"), "cornell")
    # a handle without a scene
    t = rt.RayTracer(device=0, max_width=16, max_height=16)
    try:
        with pytest.raises(rt.RtError) as e:
            t.update_instances(a)
        assert e.value.code == -4
    finally:
        t.close()


def test_update_built_scene_after_the_setters(rt, oracle, T, F):
    """The inspector path: Scene setters, then update_built_scene -- the handle equals one given the edited arrays."""
    from conftest import ASSETS
    sc = rt.Scene.from_name("cornell_box", ASSETS)
    T.load_built_scene(sc)
    _, lay_a, ptr_a = T.scene_blob()
    sc.set_mesh_material(2, rt.material(**GLASS))
    sc.set_mesh_transform(3, rt.transform(pos=(0.1, 0.0, -0.05), rot=(0, 0.19509032, 0, 0.98078528)))
    sc.add_sphere((0.2, 0.5, 0.3), 0.2, rt.material(color=(1, 1, 1, 1)))
    sc.set_sphere(0, (-0.3, 0.4, 0.2), 0.25, rt.material(color=(0.9, 0.2, 0.1, 1), smoothness=0.5))
    T.update_built_scene(sc)
    b = rt.SceneArrays.from_scene(sc)
    blob, lay, _ = T.scene_blob()
    blob_f, lay_f, _ = fresh(rt, F, b)
    assert np.array_equal(lay, lay_f) and np.array_equal(blob, blob_f)
    assert lay[1] != lay_a[1]   # (a sphere more)
    T.render(params(rt, 0))
    T.render(params(rt, 1))
    assert same_image(T.read_image(W, H), oracle_frames(rt, oracle, b, "cornell"), "cornell")
