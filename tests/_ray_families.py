"""Seeded rays and hand-built scenes for the per-ray intersection tests (tests/test_intersect_oracle_f64.py on the CPU,
tests/test_gpu_intersect.py on the device).

A render only ever hands the walk the rays a camera and the bounce sampling produce.  The families below aim at the places
where a walk goes wrong and images almost never look: axis-parallel rays with signed zeros from exactly the planes of the
scene's own boxes, shared edges and vertices, the determinant at the 1e-8 cull threshold, origins around EPSILON off a
surface, sphere tangents and insides, equal distances between meshes / triangles / a sphere, mirrored and sheared
transforms, and every item kind and size boundary the upload builds.  Everything is deterministic (seeded).

The probe traces normalize3(rd) (ray_tracer.normalize3_f32: the kernels' normalize, whose outputs are the only directions
a render traces); the oracle and the float64 reference are handed normalized(rd), the same bits.  Every origin and
direction is finite.
"""
import os

import numpy as np

from ray_tracer_2_amd import _abi as A
from ray_tracer_2_amd.ray_tracer import normalize3_f32
from ray_tracer_2_amd.scene import SceneArrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
F32 = np.float32


# ---- hand-built scenes ------------------------------------------------------------------------------------------------
def material(flag=A.MATERIAL_DEFAULT, color=(0.7, 0.7, 0.7, 1.0), ior=1.5, diffuse_index=-1):
    m = np.zeros((), A.MATERIAL_DTYPE)
    m["color"] = color
    m["smoothness"] = 0.5
    m["ior"] = ior
    m["flag"] = flag
    m["diffuse_index"] = diffuse_index
    m["normal_index"] = -1
    return m


def quad(c, du, dv):
    """Two triangles of the parallelogram c +- du +- dv, front face (wgsl:268's culling) facing cross(du, dv)."""
    c, du, dv = (np.asarray(x, np.float64) for x in (c, du, dv))
    p = [c - du - dv, c + du - dv, c + du + dv, c - du + dv]
    return np.array([[p[0], p[1], p[2]], [p[0], p[2], p[3]]], F32)


def box(lo, hi):
    """12 triangles, front faces outwards."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c, h = (lo + hi) / 2, (hi - lo) / 2
    e = np.eye(3) * h
    out = []
    for a in range(3):
        b, d = (a + 1) % 3, (a + 2) % 3
        out.append(quad(c + e[a], e[b], e[d]))
        out.append(quad(c - e[a], e[d], e[b]))
    return np.concatenate(out)


def layers(n, size=0.5, step=0.02, z0=0.0, seed=0):
    """n single triangles stacked along z (a ray along z crosses them all): deep chains of boxes."""
    rng = np.random.default_rng(seed)
    t = []
    for k in range(n):
        j = rng.uniform(-0.05, 0.05, 2)
        z = z0 + k * step
        t.append([[-size + j[0], -size, z], [size, -size + j[1], z], [0.0, size, z]])
    return np.array(t, F32)


def grid(n, size=1.0, z=0.0, seed=0, bump=0.0):
    """An n x n sheet of 2 n^2 triangles sharing edges and vertices (optionally bumped: non-coplanar neighbours)."""
    rng = np.random.default_rng(seed)
    xs = np.linspace(-size, size, n + 1)
    zz = z + bump * rng.uniform(-1, 1, (n + 1, n + 1))
    v = np.stack(np.meshgrid(xs, xs, indexing="ij"), -1)
    p = np.concatenate([v, zz[..., None]], -1).astype(F32)
    t = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = p[i, j], p[i + 1, j], p[i + 1, j + 1], p[i, j + 1]
            t += [[a, b, c], [a, c, d]]
    return np.array(t, F32)


def _bvh(tris, shape):
    """Nodes (mesh-relative indices, exact union boxes of the f32 vertices) and the leaf order of the triangles.
    shape: ("median", max_leaf) | ("chain", height) | ("rootleaf",) | ("flat2",)."""
    nodes, order = [], []

    def new():
        nodes.append(dict(left=0, right=0, first=0, count=0, lo=None, hi=None))
        return len(nodes) - 1

    def leaf(k, idx):
        nodes[k].update(first=len(order), count=len(idx))
        order.extend(idx)
        pts = tris[idx].reshape(-1, 3)
        nodes[k].update(lo=pts.min(0), hi=pts.max(0))

    def join(k, a, b):
        nodes[k].update(left=a, right=b, lo=np.minimum(nodes[a]["lo"], nodes[b]["lo"]), hi=np.maximum(nodes[a]["hi"], nodes[b]["hi"]))

    idx_all = list(range(len(tris)))
    kind = shape[0]
    if kind == "rootleaf":
        leaf(new(), idx_all)
    elif kind == "flat2":
        r, a, b = new(), new(), new()
        h = len(idx_all) // 2
        leaf(a, idx_all[:h])
        leaf(b, idx_all[h:])
        join(r, a, b)
    elif kind == "chain":   # internal node i (depth i) holds the leaf of triangle i and internal node i + 1
        height = shape[1]
        assert len(tris) == height + 1
        ks = [new() for _ in range(height)]
        for i in range(height - 1, -1, -1):
            la = new()
            leaf(la, [i])
            if i == height - 1:
                lb = new()
                leaf(lb, [height])
                join(ks[i], la, lb)
            else:
                join(ks[i], la, ks[i + 1])
    else:
        max_leaf = shape[1]
        cen = tris.astype(np.float64).mean(1)

        def rec(k, idx):
            if len(idx) <= max_leaf:
                leaf(k, idx)
                return
            c = cen[idx]
            ax = int(np.argmax(c.max(0) - c.min(0)))
            s = [idx[j] for j in np.argsort(c[:, ax], kind="stable")]
            a, b = new(), new()
            rec(a, s[:len(s) // 2])
            rec(b, s[len(s) // 2:])
            join(k, a, b)
        rec(new(), idx_all)
    return nodes, order


def _matrices(m2w):
    """(world_to_model, model_to_world) as stored ([column][row]) from a 4 x 4 row-major model-to-world matrix."""
    m = np.asarray(m2w, np.float64)
    return np.linalg.inv(m).T.astype(F32), m.T.astype(F32)


def trs(pos=(0, 0, 0), axis=(0, 0, 1), angle=0.0, scale=(1, 1, 1), shear=0.0):
    """Row-major model-to-world: translate * rotate (axis, angle) * shear (x += shear * y) * scale."""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * k @ k
    sh = np.eye(3)
    sh[0, 1] = shear
    m = np.eye(4)
    m[:3, :3] = r @ sh @ np.diag(scale)
    m[:3, 3] = pos
    return m


def make_arrays(meshes, spheres=()):
    """SceneArrays from [dict(tris=(T, 3, 3), bvh=shape, m2w=4x4 or None, mat=material)] and [(centre, radius, mat)]."""
    rng = np.random.default_rng(len(meshes) * 7 + len(spheres))
    tri_rows, node_rows, mesh_rows = [], [], []
    for m in meshes:
        tris = np.asarray(m["tris"], F32)
        nodes, order = _bvh(tris, m.get("bvh", ("median", 4)))
        t = tris[order]
        rec = np.zeros(len(t), A.TRI_DTYPE)
        rec["v1"], rec["v2"], rec["v3"] = t[:, 0], t[:, 1], t[:, 2]
        fn = np.cross(t[:, 1].astype(np.float64) - t[:, 0], t[:, 2].astype(np.float64) - t[:, 0])
        fn /= np.maximum(np.linalg.norm(fn, axis=1, keepdims=True), 1e-30)
        for k in ("n1", "n2", "n3"):   # smooth-ish normals: interpolation is exercised
            rec[k] = (fn + 0.2 * rng.uniform(-1, 1, fn.shape)).astype(F32)
        for k in ("uv10", "uv11", "uv20", "uv21", "uv30", "uv31"):
            rec[k] = rng.uniform(0, 1, len(t)).astype(F32)
        mr = np.zeros((), A.MESH_DTYPE)
        mr["world_to_model"], mr["model_to_world"] = _matrices(m.get("m2w") if m.get("m2w") is not None else np.eye(4))
        mr["node_offset"] = sum(len(x) for x in node_rows)
        mr["triangle_offset"] = sum(len(x) for x in tri_rows)
        mr["triangles"] = len(t)
        mr["material"] = m.get("mat", material())
        nr = np.zeros(len(nodes), A.NODE_DTYPE)
        for i, n in enumerate(nodes):
            nr[i]["left"], nr[i]["right"], nr[i]["first"], nr[i]["count"] = n["left"], n["right"], n["first"], n["count"]
            nr[i]["aabb_min"], nr[i]["aabb_max"] = n["lo"], n["hi"]
        tri_rows.append(rec)
        node_rows.append(nr)
        mesh_rows.append(mr)
    sp = np.zeros(len(spheres), A.SPHERE_DTYPE)
    for i, (c, r, mt) in enumerate(spheres):
        sp[i]["pos"], sp[i]["radius"], sp[i]["material"] = c, r, mt
    u = A.SceneUniform()
    u.spheres, u.meshes = len(spheres), len(meshes)
    u.nodes = sum(len(x) for x in node_rows)
    for k in range(4):
        u.camera.cam_to_world[k][k] = 1.0
    u.camera.view_params[:] = [1.0, 1.0, 1.0]
    return SceneArrays(u, sp, np.array(mesh_rows, A.MESH_DTYPE), np.concatenate(tri_rows) if tri_rows else np.zeros(0, A.TRI_DTYPE),
                       np.concatenate(node_rows) if node_rows else np.zeros(0, A.NODE_DTYPE))


def _plain_meshes(n, seed, same_xform=True, shape=("median", 4), spread=3.0):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        c = rng.uniform(-spread, spread, 3)
        h = rng.uniform(0.2, 0.6, 3)
        m2w = None if same_xform else trs(pos=rng.uniform(-0.5, 0.5, 3), axis=rng.normal(size=3), angle=float(rng.uniform(0, 3)))
        out.append(dict(tris=box(c - h, c + h), bvh=shape, m2w=m2w, mat=material(color=(0.5, 0.5, 0.5 + i / (4 * n), 1))))
    return out


def built_scene(name):
    """The hand-built scenes by name (see SCENES)."""
    if name == "items":   # one of every item kind of the few-mesh kernels: forest, flat2, root leaf, single
        ms = [dict(tris=grid(4, 1.0, z=-1.0, seed=1, bump=0.05), bvh=("median", 4)),       # \ forest (same transform,
              dict(tris=box((-0.5, -0.5, 0.2), (0.1, 0.3, 0.6)), bvh=("median", 2)),      # / internal roots)
              dict(tris=box((0.3, -0.2, 0.0), (0.8, 0.4, 0.5)), bvh=("flat2",)),          # two-leaf root
              dict(tris=quad((0, 0, 1.5), (0.6, 0, 0), (0, 0.6, 0)), bvh=("rootleaf",)),  # root leaf
              dict(tris=box((-0.3, -0.3, -0.3), (0.3, 0.3, 0.3)), bvh=("median", 2),      # single (own transform)
                   m2w=trs(pos=(0.2, 0.9, 0.3), axis=(1, 1, 0), angle=0.7))]
        return make_arrays(ms)
    if name == "xforms":  # rotated + non-uniformly scaled, sheared, mirrored (negative determinant), glass mirrored
        b = box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
        ms = [dict(tris=b, bvh=("median", 2), m2w=trs(pos=(-1.5, 0, 0), axis=(1, 2, 3), angle=0.9, scale=(1.7, 0.4, 1.1))),
              dict(tris=b, bvh=("median", 2), m2w=trs(pos=(0, 1.2, 0), axis=(0, 1, 0), angle=0.3, shear=0.6)),
              dict(tris=b, bvh=("median", 2), m2w=trs(pos=(1.5, 0, 0), scale=(-1.0, 1.0, 1.0))),
              dict(tris=grid(3, 0.8, seed=2, bump=0.1), bvh=("median", 2), m2w=trs(pos=(0, -1.2, 0), axis=(1, 0, 0), angle=0.4, scale=(1, -1.5, 1)),
                   mat=material(A.MATERIAL_GLASS)),
              dict(tris=box((-2.5, -2.5, -2.5), (2.5, 2.5, 2.5)), bvh=("median", 4))]
        return make_arrays(ms)
    if name == "glass":   # culled back faces of opaque meshes against glass meshes, hit from both sides
        ms = [dict(tris=box((-1, -1, -1), (0, 1, 1)), bvh=("median", 2)),
              dict(tris=box((0, -1, -1), (1, 1, 1)), bvh=("median", 2), mat=material(A.MATERIAL_GLASS)),
              dict(tris=grid(3, 1.5, z=1.5, seed=3), bvh=("flat2",), mat=material(A.MATERIAL_GLASS)),
              dict(tris=grid(3, 1.5, z=-1.5, seed=4), bvh=("rootleaf",))]
        return make_arrays(ms, [((0.0, 0.0, 2.5), 0.4, material(A.MATERIAL_GLASS))])
    if name == "ties":    # equal distances: a duplicated mesh, coincident triangles, a sphere and a triangle
        g = grid(3, 1.0, z=0.0, seed=5)
        ms = [dict(tris=g, bvh=("median", 2), mat=material(color=(1, 0, 0, 1))),
              dict(tris=g, bvh=("median", 2), mat=material(color=(0, 1, 0, 1))),
              dict(tris=np.concatenate([g, g[::-1]]), bvh=("median", 3)),
              dict(tris=g, bvh=("flat2",), mat=material(color=(0, 0, 1, 1))),
              dict(tris=g, bvh=("rootleaf",), mat=material(color=(1, 1, 0, 1)))]
        return make_arrays(ms, [((0.0, 0.0, -1.0), 1.0, material())])
    if name == "ties_tlas":   # the duplicated meshes inside top-level tree runs (and a run without a tree)
        g = grid(3, 1.0, z=0.0, seed=6)
        ms = [dict(tris=g, bvh=("median", 2), mat=material(color=(i / 12.0, 0.5, 0.5, 1))) for i in range(12)]
        ms += [dict(tris=g, bvh=("median", 2), m2w=trs(pos=(0, 0, 0.5)), mat=material(color=(0.1, 0.1, i / 4.0, 1))) for i in range(3)]
        return make_arrays(ms)
    if name.startswith("tlas"):   # a run of tlas_min - 1 / tlas_min / tlas_min + 1 meshes under one transform
        return make_arrays(_plain_meshes(int(name[4:]), seed=int(name[4:])))
    if name.startswith("cull"):   # 15 / 16 / 17 meshes under their own transforms (root-box culling from 16 on)
        return make_arrays(_plain_meshes(int(name[4:]), seed=int(name[4:]), same_xform=False))
    if name.startswith("leaf"):   # a leaf of 127 / 128 triangles beside another (the one-dword stack entry limit)
        k = int(name[4:])
        g = grid(8, 1.0, seed=k, bump=0.3)[:k]
        sh = [np.array(v, F32) for v in ((0, 0, 0.6), (0, 0, 0.2), (0, 0, -0.2), (0, 0, -0.6))]
        return make_arrays([dict(tris=np.concatenate([g + sh[0], g + sh[0] + F32(0.01)]), bvh=("flat2",)),   # root leaves
                            dict(tris=np.concatenate([g + d for d in sh[1:]] + [g + sh[1] + F32(0.03)]), bvh=("median", k))])
    if name.startswith("height"):   # BVH height 30, 31 (not deep), 32, 33 (deep: the shader's clamped stack)
        hgt = int(name[6:])
        return make_arrays([dict(tris=layers(hgt + 1, seed=hgt), bvh=("chain", hgt)),
                            dict(tris=box((-1, -1, -0.5), (1, 1, -0.2)), bvh=("median", 2))])
    raise KeyError(name)


BUILT = ["items", "xforms", "glass", "ties", "ties_tlas", "tlas7", "tlas8", "tlas9", "cull15", "cull16", "cull17",
         "leaf127", "leaf128", "height30", "height31", "height32", "height33"]
LIBRARY = ["cornell", "dragon", "sponza", "room"]


def library_scene(rt, name):
    from ray_tracer_2_amd import scenes
    if name == "cornell":
        return rt.SceneArrays.load(os.path.join(GOLDEN, "cornell_scene.npz"))
    if name == "dragon":   # BASELINE config 3 stand-in (tests/test_gpu_scenes.py dragon_arrays)
        sc = scenes.cornell_dragon(scenes.load_raw_meshes(os.path.join(GOLDEN, "cornell_raw.npz")),
                                   scenes.load_raw_meshes(os.path.join(GOLDEN, "dragon_raw.npz")), subdivide=3)
        return rt.SceneArrays.from_scene(sc)
    if name == "sponza":
        return rt.SceneArrays.from_scene(scenes.sponza_standin())
    if name == "room":
        return rt.SceneArrays.from_scene(rt.Scene.from_name("room", os.path.join(ROOT, "tests", "data")))
    raise KeyError(name)


def scene(rt, name):
    return library_scene(rt, name) if name in LIBRARY else built_scene(name)


# ---- ray families -----------------------------------------------------------------------------------------------------
def _world(m, p, w=1.0):
    """(model_to_world * (p, w)).xyz in binary32, the stored [column][row] matrix."""
    c = np.asarray(m["model_to_world"], F32)
    p = np.asarray(p, F32).reshape(-1, 3)
    return ((p[:, 0:1] * c[0, :3] + p[:, 1:2] * c[1, :3]) + p[:, 2:3] * c[2, :3] + F32(w) * c[3, :3]).astype(F32)


def _identity(m):
    return np.array_equal(np.asarray(m["model_to_world"], F32), np.eye(4, dtype=F32))


def _mesh_tris(arrays, mi):
    m = arrays.meshes[mi]
    t = arrays.triangles[int(m["triangle_offset"]):int(m["triangle_offset"]) + int(m["triangles"])]
    return np.stack([t["v1"], t["v2"], t["v3"]], 1).astype(F32)


def _pick_meshes(arrays, rng, k):
    n = len(arrays.meshes)
    return rng.choice(n, size=min(n, k), replace=False) if n else []


def _bounds(arrays):
    pts = []
    for mi in range(len(arrays.meshes)):
        t = _mesh_tris(arrays, mi).reshape(-1, 3)
        pts.append(_world(arrays.meshes[mi], t[:: max(1, len(t) // 4096)]))
    for s in arrays.spheres:
        pts.append(np.array([np.asarray(s["pos"]) - s["radius"], np.asarray(s["pos"]) + s["radius"]], F32))
    p = np.concatenate(pts)
    return p.min(0).astype(np.float64), p.max(0).astype(np.float64)


def _finish(ro, rd):
    """(origins, directions) in binary32, without the rays normalize3 cannot make a direction of.  The directions are
    NOT normalized: the probe normalizes what it is given (RayTracer.intersect), and the oracle and the float64
    reference take normalized(rd) -- the same bits."""
    ro = np.ascontiguousarray(ro, F32).reshape(-1, 3)
    rd = np.ascontiguousarray(rd, F32).reshape(-1, 3)
    n = normalize3_f32(rd)
    ok = np.isfinite(ro).all(1) & np.isfinite(rd).all(1) & np.isfinite(n).all(1) & (np.abs(n).max(1) > 0)
    return ro[ok], rd[ok]


def normalized(rd):
    """The directions the probe traces for `rd`: the kernels' normalize3 in binary32."""
    return normalize3_f32(rd)


def _random_dirs(rng, n):
    return rng.normal(size=(n, 3))


def fam_axis(arrays, rng, n_boxes=160):
    """The 6 signed axis directions, the other components +0 or -0, from origins exactly on a face plane of one of the
    scene's own node boxes (aabb_min / aabb_max), and one nextafter either side."""
    ro, rd = [], []
    nodes = arrays.nodes
    for mi in _pick_meshes(arrays, rng, 24):
        m = arrays.meshes[mi]
        off = int(m["node_offset"])
        cnt = len(nodes) - off
        for ni in rng.integers(off, off + min(cnt, 4096), size=max(1, n_boxes // 24)):
            lo, hi = nodes[ni]["aabb_min"].astype(F32), nodes[ni]["aabb_max"].astype(F32)
            for ax in range(3):
                for face in (lo[ax], hi[ax]):
                    for val in (np.nextafter(face, F32(-np.inf)), face, np.nextafter(face, F32(np.inf))):
                        p = (lo + (hi - lo) * rng.uniform(0, 1, 3).astype(F32)).astype(F32)
                        if rng.uniform() < 0.3:   # exactly on an edge or a corner of the box too
                            other = (ax + 1 + rng.integers(0, 2)) % 3
                            p[other] = lo[other] if rng.uniform() < 0.5 else hi[other]
                        p[ax] = val
                        pw = _world(m, p)[0] if not _identity(m) else p
                        for d_ax in range(3):
                            for sgn in (1.0, -1.0):
                                d = np.array([0.0, 0.0, 0.0], F32) * np.where(rng.uniform(size=3) < 0.5, F32(-1), F32(1))
                                d[d_ax] = sgn
                                ro.append(pw)
                                rd.append(d)
    return _finish(ro, rd)


def _shared(tris):
    """(edge midpoints, vertices) shared by two triangles of a mesh (exact f32 vertex matches)."""
    key = {}
    for ti, t in enumerate(tris[:20000]):
        for a, b in ((0, 1), (1, 2), (2, 0)):
            e = tuple(sorted((t[a].tobytes(), t[b].tobytes())))
            key.setdefault(e, []).append(ti)
    mids, verts = [], []
    for (a, b), ts in key.items():
        if len(ts) >= 2:
            va, vb = np.frombuffer(a, F32), np.frombuffer(b, F32)
            mids.append(((va + vb) * F32(0.5)).astype(F32))
            verts.append(va)
    return np.array(mids, F32).reshape(-1, 3), np.array(verts, F32).reshape(-1, 3)


def fam_edges(arrays, rng, per_mesh=60):
    """Rays aimed at f32-rounded shared edge midpoints and shared vertices of adjacent triangles, and at their
    nextafter neighbours, from both sides."""
    ro, rd = [], []
    for mi in _pick_meshes(arrays, rng, 12):
        m = arrays.meshes[mi]
        mids, verts = _shared(_mesh_tris(arrays, mi))
        pts = np.concatenate([mids, verts])
        if len(pts) == 0:
            continue
        pts = pts[rng.choice(len(pts), size=min(len(pts), per_mesh), replace=False)]
        for p in pts:
            for step in (None, -1, 1):
                q = p.copy()
                if step is not None:
                    k = rng.integers(0, 3)
                    q[k] = np.nextafter(q[k], F32(np.inf) * step)
                tw = _world(m, q)[0]
                d = _random_dirs(rng, 1)[0]
                dist = rng.uniform(0.05, 2.0)
                o = (tw - d * dist).astype(F32)
                ro.append(o)
                rd.append(tw.astype(np.float64) - o)
    return _finish(ro, rd)


def _tri_frames(arrays, rng, k):
    """Random triangles (world space): centroid, unit normal, in-plane unit vector, |cross(e_ab, e_ac)| in world units."""
    out = []
    for mi in _pick_meshes(arrays, rng, 12):
        m = arrays.meshes[mi]
        t = _mesh_tris(arrays, mi)
        for ti in rng.choice(len(t), size=min(len(t), max(1, k // 12)), replace=False):
            w = _world(m, t[ti]).astype(np.float64)
            n = np.cross(w[1] - w[0], w[2] - w[0])
            nn = np.linalg.norm(n)
            if nn < 1e-12:
                continue
            e = (w[1] - w[0]) / np.linalg.norm(w[1] - w[0])
            out.append((mi, ti, w, n / nn, e, nn))
    return out


def fam_thresholds(arrays, rng, k=240):
    """Grazing rays whose determinant brackets 1e-8; origins 0, 0.5e-5 .. 2e-5 off a surface on both sides (around
    EPSILON), towards it and away; origins on the surface with random directions (what bounce rays do)."""
    ro, rd = [], []
    for _mi, _ti, w, n, e, nn in _tri_frames(arrays, rng, k):
        c = w.mean(0)
        for f in (0.5, 0.9, 1.0, 1.1, 2.0):   # det = -dot(ld, n) ~ f * 1e-8 (local = world for the untransformed)
            s = f * 1e-8 / nn
            for sign in (1.0, -1.0):
                d = e * np.sqrt(max(0.0, 1.0 - s * s)) - sign * n * s
                ro.append(c - d * rng.uniform(0.05, 1.0))
                rd.append(d)
        for h in (0.0, 0.5e-5, 0.9e-5, 1e-5, 1.1e-5, 2e-5):
            for side in (1.0, -1.0):
                o = c + side * h * n
                ro.append(o)
                rd.append(-side * n + 0.3 * rng.normal(size=3))
                ro.append(o)
                rd.append(side * n + 0.3 * rng.normal(size=3))
        b = rng.dirichlet((1, 1, 1))
        p = (w[0] * b[0] + w[1] * b[1] + w[2] * b[2]).astype(F32)
        for _ in range(4):
            ro.append(p)
            rd.append(_random_dirs(rng, 1)[0])
    return _finish(ro, rd)


def fam_spheres(arrays, rng, per_sphere=120):
    """Origins inside and on the surface, tangent rays, exits with `far` bracketing 0.001."""
    ro, rd = [], []
    for s in arrays.spheres:
        c, r = np.asarray(s["pos"], np.float64), float(s["radius"])
        for _ in range(per_sphere // 6):
            u = rng.normal(size=3)
            u /= np.linalg.norm(u)
            ro.append(c + u * r * rng.uniform(0, 0.99))
            rd.append(_random_dirs(rng, 1)[0])                      # inside
            ro.append(c + u * r)
            rd.append(_random_dirs(rng, 1)[0])                      # on the surface
            t = np.cross(u, rng.normal(size=3))
            t /= np.linalg.norm(t)
            ro.append(c + u * r - t * r * rng.uniform(0.5, 3))
            rd.append(t)                                            # tangent
            for f in (0.5, 1.0, 2.0):
                ro.append(c + u * (r - 0.001 * f))
                rd.append(u)                                        # far ~ 0.001 f
    return _finish(ro, rd)


def fam_random(arrays, rng, n):
    """n random rays from inside and outside the scene bounds (1.5 x the box), random directions."""
    lo, hi = _bounds(arrays)
    c, h = (lo + hi) / 2, (hi - lo) / 2 * 1.5
    return _finish(c + h * rng.uniform(-1, 1, (n, 3)), _random_dirs(rng, n))


def fam_ties(arrays, rng, n=2000):
    """Axis rays and near-axis rays onto z = 0 from above and below (the tie scenes put equal-distance primitives there)."""
    xy = rng.uniform(-1.1, 1.1, (n, 2))
    z = rng.choice([-2.0, 2.0, 0.5, -0.5], n)
    ro = np.concatenate([xy, z[:, None]], 1)
    rd = np.zeros((n, 3))
    rd[:, 2] = -np.sign(z)
    rd[n // 2:] += 0.2 * rng.normal(size=(n - n // 2, 3))
    ro[:8] = [[0, 0, 2], [0, 0, -2], [0.5, 0.5, 2], [-0.5, 0.25, 2], [0, 0, 0.5], [1.0 / 3, 1.0 / 3, 2], [0, 0, 1], [0.2, -0.3, 3]]
    rd[:8] = [[0, 0, -1], [0, 0, 1], [0, 0, -1], [0, 0, -1], [0, 0, -1], [0, 0, -1], [0, 0, -1], [0, 0, -1]]
    return _finish(ro, rd)


def families(arrays, name, n_random=100000, seed=0):
    """name -> (ro, rd) for every family that applies to the scene (rd not normalized: see _finish)."""
    rng = np.random.default_rng([seed, sum(map(ord, name))])
    out = {"axis": fam_axis(arrays, rng), "edges": fam_edges(arrays, rng), "thresholds": fam_thresholds(arrays, rng),
           "random": fam_random(arrays, rng, n_random)}
    if len(arrays.spheres):
        out["spheres"] = fam_spheres(arrays, rng)
    if name.startswith("ties") or name.startswith("height") or name.startswith("leaf"):
        out["ties"] = fam_ties(arrays, rng)
    return {k: v for k, v in out.items() if len(v[0])}
