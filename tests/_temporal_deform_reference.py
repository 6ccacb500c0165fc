"""An independent numpy restatement of temporal accumulation across deforming meshes (include/rt_abi.h:
rt_temporal_accumulate_deforming) and of rt_object_motions_deforming, and the frames their tests run on.

`carry_deformed` carries the texels of the deformed records into the previous frame's world by their previous triangle, in
numpy float32 -- one rounded binary32 ufunc per line, np.float32 throughout, the square root np.sqrt on float32 (correctly
rounded), in the order the definition gives.  `reference` hands the carried planes, with the deformed records struck from the
table, to the restatements of the rest (tests/_temporal_motion_reference.py for the rigid records, tests/
_temporal_reference.py for everything after the carry).  Nothing here shares code with csrc/.  `stats` reports which of the
new rules fired where, which the tests use to show that their inputs meet every one.

`synthetic_case(W, H)` is a seeded pair of frames with 5 previous triangles behind tri_first = 3 and a table of 4 objects --
still, rigid, deformed, deformed under a sheared previous transform -- salted with every rule; `sheet_scene` is the scene of
the GPU tests: a rippling sheet of 8 x 8 quads over a floor, with one sphere."""
import functools

import numpy as np

import _temporal_motion_reference as M
import _temporal_reference as R

F32 = R.F32
NO_OBJECT = R.NO_OBJECT
DEFORMED = 2
BACKFACE = 2
TRI_FIRST, N_TRI = 3, 5
GUIDES = ("primitive", "bary", "flags")


def tri_dtype():
    from ray_tracer_2_amd import _abi as A
    return A.TRI_DTYPE


def carry_deformed(planes, motions, prev_triangles, tri_first, stats=None):
    """The point and normal planes with the deformed records' texels carried (X', n' of the definition) and those of them
    that take the "no history" result made unreprojectable (zeros); every other texel as it is."""
    X, n = np.ascontiguousarray(planes["point"], F32), np.ascontiguousarray(planes["normal"], F32)
    obj = np.ascontiguousarray(planes["object"], np.uint32)
    prim = np.ascontiguousarray(planes["primitive"], np.uint32).astype(np.int64)
    bary = np.ascontiguousarray(planes["bary"], F32)
    back = (np.ascontiguousarray(planes["flags"], np.uint8) & BACKFACE) != 0
    tris = np.ascontiguousarray(prev_triangles)
    n_tri, n_objects = len(tris), len(motions)
    u = bary[..., 0]
    v = bary[..., 1]
    with np.errstate(all="ignore"):
        rep = (n != 0).any(-1) & np.isfinite(n).all(-1) & np.isfinite(X).all(-1) & (obj != NO_OBJECT)
        inside = obj < n_objects
        k = np.where(inside, obj, 0)
        deformed = rep & inside & (motions["moved"][k] == DEFORMED)
        in_range = (prim >= tri_first) & (prim - tri_first < n_tri)
        bary_ok = np.isfinite(u) & np.isfinite(v)
        T = tris[np.where(in_range, prim - tri_first, 0)]
        d = motions["d"][k].astype(F32)      # (H, W, 4, 3): [col][row]
        nt = motions["nt"][k].astype(F32)    # (H, W, 3, 3)
        one = F32(1)
        w = one - u
        w = w - v
        Xm, g = [], []
        for r in range(3):
            a = T["v1"][..., r] * w
            b = T["v2"][..., r] * u
            a = a + b
            b = T["v3"][..., r] * v
            Xm.append(a + b)
            a = T["n1"][..., r] * w
            b = T["n2"][..., r] * u
            a = a + b
            b = T["n3"][..., r] * v
            g.append(a + b)
        Xp, m = [], []
        for r in range(3):
            a = d[..., 0, r] * Xm[0]
            b = d[..., 1, r] * Xm[1]
            a = a + b
            b = d[..., 2, r] * Xm[2]
            a = a + b
            Xp.append(a + d[..., 3, r])
            a = nt[..., 0, r] * g[0]
            b = nt[..., 1, r] * g[1]
            a = a + b
            b = nt[..., 2, r] * g[2]
            m.append(a + b)
        a = m[0] * m[0]
        b = m[1] * m[1]
        a = a + b
        b = m[2] * m[2]
        a = a + b
        length = np.sqrt(a)
        s = np.where(back, F32(-1), F32(1)).astype(F32)
        np_ = []
        for r in range(3):
            a = m[r] / length
            np_.append(a * s)
        Xp, np_ = np.stack(Xp, -1), np.stack(np_, -1)
        assert Xp.dtype == F32 and np_.dtype == F32 and length.dtype == F32 and w.dtype == F32
        bad_x, bad_n = ~np.isfinite(Xp).all(-1), ~np.isfinite(np_).all(-1)
        readable = in_range & bary_ok
        lost = deformed & (~readable | bad_x | bad_n)
        kept = deformed & ~lost
        X2 = np.where(kept[..., None], Xp, np.where(lost[..., None], F32(0), X)).astype(F32)
        n2 = np.where(kept[..., None], np_, np.where(lost[..., None], F32(0), n)).astype(F32)
    if stats is not None:
        stats.update(deformed=deformed, carried=kept, deform_lost=lost, below_range=deformed & (prim < tri_first),
                     past_range=deformed & (prim - tri_first >= n_tri), bary_bad=deformed & in_range & ~bary_ok,
                     zero_normal_length=deformed & readable & (length == 0), deform_point_bad=deformed & readable & bad_x,
                     deform_normal_bad=deformed & readable & bad_n, backface=deformed & back, frontface=deformed & ~back)
    return X2, n2


def reference(planes, prev_camera, motions, prev_triangles, tri_first, max_history=np.inf, point_tolerance=0.01, normal_cos=0.9,
              stats=None):
    """planes: R.INPUTS and GUIDES.  Returns out, out_history, motion; stats receives every restatement's masks."""
    own = {}
    X2, n2 = carry_deformed(planes, motions, prev_triangles, tri_first, own)
    rest = motions.copy()
    rest["moved"][motions["moved"] == DEFORMED] = 0      # (a carried texel is then worked as a still one's: on X', n')
    st = {} if stats is None else stats
    res = M.reference(dict({k: planes[k] for k in R.INPUTS if planes.get(k) is not None}, point=X2, normal=n2), prev_camera, rest,
                      max_history, point_tolerance, normal_cos, stats=st)
    st.update(own)
    return res


def object_motions(prev_meshes, meshes, prev_spheres, spheres, deformed):
    """rt_object_motions_deforming in numpy: deformed is a boolean per mesh."""
    t = M.object_motions(prev_meshes, meshes, prev_spheres, spheres)
    for k in np.flatnonzero(np.asarray(deformed, bool)):
        t[k] = np.zeros((), t.dtype)
        t["moved"][k] = DEFORMED
        t["d"][k] = prev_meshes["model_to_world"][k][:, :3]
        t["nt"][k] = prev_meshes["model_to_world"][k][:3, :3]
    return t


def _barycentric(P, a, b, c):
    """(u, v) of the points P (..., 3) in the triangle a, b, c (weights of b and c), float64, by least squares."""
    e1, e2, q = b - a, c - a, P - a
    d11, d12, d22 = e1 @ e1, e1 @ e2, e2 @ e2
    q1, q2 = q @ e1, q @ e2
    det = d11 * d22 - d12 * d12
    return (d22 * q1 - d12 * q2) / det, (d11 * q2 - d12 * q1) / det


@functools.lru_cache(maxsize=None)
def synthetic_case(W=37, H=19, seed=2025):
    """A wall at view depth 4 of the previous camera, in four bands of columns, one per object of the table: 0 stands still;
    1 moved rigidly (rotation, non-uniform scale, translation); 2 is deformed, its previous transform a rotation and a
    translation; 3 is deformed under a sheared previous transform.  The upper half of the wall faces away (the previous
    normals are flipped there) and is seen from behind: the deformed texels there carry RT_HIT_BACKFACE.  Every current
    texel falls at a seeded offset of up to 1.5 texels from itself in the previous frame (taps off every edge at the frame's
    border, and four placed texels); a deformed texel's primitive and barycentrics name that point on one of the previous
    triangles 3 .. 6 -- large triangles of the wall in the object's model space, with vertex normals that differ --; triangle
    7 is degenerate: its normals interpolate to zero length.  Salted, on deformed texels: primitive words below, past and far
    past the range, NaN and infinite barycentrics, zero and NaN normals, object words past the table and 0xffffffff; NaNs
    and misses in the previous planes.  Returns (planes, prev_camera, motions, prev_triangles, notes), read-only."""
    from ray_tracer_2_amd import _abi as A
    rng = np.random.default_rng(seed)
    a = 0.02
    c2w = np.array([[np.cos(a), 0, -np.sin(a), 0], [0, 1, 0, 0], [np.sin(a), 0, np.cos(a), 0], [0.3, -0.2, 0.1, 1]], np.float64)
    cam = R.make_camera(A, c2w, (1.2, 0.8, 1.5))
    facing = -c2w[2, :3]
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    band = lambda x: np.minimum((np.floor(x) * 4 // W).astype(np.int64), 3)   # noqa: E731
    up = lambda y: np.where(y >= H // 2, -1.0, 1.0)                            # noqa: E731
    prev_point = R.unproject(cam, xx, yy, 4.0, W, H)
    prev_normal = facing * up(yy)[..., None]
    prev_object = band(xx).astype(np.uint32)
    prev_color = np.concatenate([rng.uniform(0, 3, (H, W, 3)), rng.uniform(0, 1, (H, W, 1))], -1)
    prev_history = rng.integers(1, 11, (H, W)).astype(np.float64)
    # the current frame: where each texel falls in the previous one
    tx, ty = xx + rng.uniform(-1.5, 1.5, (H, W)), yy + rng.uniform(-1.5, 1.5, (H, W))
    obj = band(xx).astype(np.uint32)
    notes = {}
    x2 = int(np.flatnonzero(band(np.arange(W)) == 2)[0])      # the first column of object 2

    def place(name, y, x, fx, fy):
        tx[y, x], ty[y, x] = fx, fy
        notes[name] = (y, x)

    place("left_edge", 3, x2, -0.5, 3.25)
    place("right_edge", 3, x2 + 1, W - 0.5, 3.25)
    place("bottom_edge", 3, x2 + 2, 4.25, -0.75)
    place("top_edge", 3, x2 + 3, 4.25, H - 0.25)
    place("off_left", 4, x2, -3.0, 5.0)
    place("one_tap", 4, x2 + 1, float(x2), 5.004)
    P = R.unproject(cam, tx, ty, 4.0, W, H)                   # float64 targets on the wall
    sign = up(yy)
    point, normal = P.copy(), facing * sign[..., None]
    t = M.table(4)
    # 1: rigid.  X' = L X + T: the current points are L^-1 (P - T), the current normals L^T n' normalised
    ra, rb = 0.3, -0.2
    rot = np.array([[np.cos(ra), -np.sin(ra), 0], [np.sin(ra), np.cos(ra), 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, np.cos(rb), -np.sin(rb)], [0, np.sin(rb), np.cos(rb)]])
    L, T = rot @ np.diag([1.5, 0.75, 1.25]), np.array([0.4, -0.3, 0.2])
    M.record(t, 1, L, T)
    rigid = obj == 1
    point[rigid] = (P[rigid] - T) @ np.linalg.inv(L).T
    nb = normal[rigid] @ L
    normal[rigid] = nb / np.linalg.norm(nb, axis=-1, keepdims=True)
    # 2, 3: deformed.  d = the previous model_to_world, nt its 3 x 3; the current point and normal planes are NOT what the
    # call uses for these texels: they hold a displaced surface (what a deformation leaves)
    shear = np.array([[1.0, 0.35, 0.0], [0.0, 1.0, -0.25], [0.15, 0.0, 1.0]])
    m2w = {2: (rot.T, np.array([-0.2, 0.1, 0.3])), 3: (shear @ np.diag([0.8, 1.2, 1.1]), np.array([0.25, -0.15, -0.1]))}
    for k, (lin, tr) in m2w.items():
        t["d"][k, :3] = lin.T
        t["d"][k, 3] = tr
        t["nt"][k] = lin.T
        t["moved"][k] = DEFORMED
    corners = R.unproject(cam, np.array([-40.0, 90.0, 10.0, -30.0, 70.0]), np.array([-30.0, -20.0, 80.0, 60.0, -45.0]), 4.0, W, H)
    world = [(0, 1, 2), (1, 2, 3), (3, 4, 0), (4, 1, 2)]      # four large triangles of the wall that hold the frame and its rim
    owner = [2, 2, 2, 3]                                        # triangles 3, 4, 5 in object 2's model space, 6 in object 3's
    tris = np.zeros(N_TRI, tri_dtype())
    for j, (ids, k) in enumerate(zip(world, owner)):
        lin, tr = m2w[k]
        inv = np.linalg.inv(lin)
        for name, nname, c in zip(("v1", "v2", "v3"), ("n1", "n2", "n3"), ids):
            tris[name][j] = inv @ (corners[c] - tr)
            tris[nname][j] = inv @ (facing + 0.08 * rng.uniform(-1, 1, 3))
    tris["v1"][4], tris["v2"][4], tris["v3"][4] = tris["v1"][3], tris["v2"][3], tris["v3"][3]   # 7: its normals are zero
    for name in ("uv10", "uv11", "uv20", "uv21", "uv30", "uv31"):
        tris[name] = rng.uniform(0, 1, N_TRI)
    prim = np.full((H, W), 0xFFFFFFFF, np.uint32)
    bary = rng.uniform(0, 1, (H, W, 2))
    flags = np.where(obj < 4, 1, 0).astype(np.uint8) | np.where(sign < 0, BACKFACE, 0).astype(np.uint8)
    pick = rng.integers(0, 3, (H, W))
    for k in (2, 3):
        on = obj == k
        j = np.where(on, pick if k == 2 else 3, 0)
        for jj in range(4):
            sel = on & (j == jj)
            ca, cb, cc = (corners[c] for c in world[jj])
            u, v = _barycentric(P[sel], ca, cb, cc)
            bary[sel, 0], bary[sel, 1] = u, v
            prim[sel] = TRI_FIRST + jj
        # what the G-buffer holds of a deformed mesh: the point off the previous surface, the normal turned
        point[on] = P[on] + 0.3 * facing + rng.uniform(-0.2, 0.2, (int(on.sum()), 3))
        nn = sign[on][..., None] * facing + rng.uniform(-0.5, 0.5, (int(on.sum()), 3))
        normal[on] = nn / np.linalg.norm(nn, axis=-1, keepdims=True)
    # salt, on texels of object 2 (rows 6 ..) and object 3
    x3 = int(np.flatnonzero(band(np.arange(W)) == 3)[0])
    prim[6, x2], prim[6, x2 + 1], prim[6, x2 + 2], prim[6, x2 + 3] = 2, TRI_FIRST + N_TRI, 0xFFFFFFFF, 0
    prim[7, x2:x2 + 2] = TRI_FIRST + 4                          # the degenerate triangle
    bary[8, x2, 0], bary[8, x2 + 1, 1], bary[8, x2 + 2, 0], bary[8, x2 + 3, 1] = np.nan, np.inf, -np.inf, np.nan
    normal[9, x2], normal[9, x2 + 1, 1] = 0, np.nan
    point[9, x2 + 2, 2] = np.inf                               # (the point plane of a deformed texel still decides "reprojectable")
    obj[10, x2], obj[10, x2 + 1], obj[10, x2 + 2] = 4, 9, NO_OBJECT
    normal[H - 2, x3:x3 + 3], obj[H - 2, x3:x3 + 3] = 0, NO_OBJECT      # misses
    for name, (y, x) in (("below_range", (6, x2)), ("past_range", (6, x2 + 1)), ("degenerate", (7, x2)), ("nan_bary", (8, x2)),
                         ("inf_bary", (8, x2 + 1)), ("zero_normal", (9, x2)), ("nan_normal", (9, x2 + 1)), ("past_table", (10, x2)),
                         ("no_object", (10, x2 + 2))):
        notes[name] = (y, x)
    prev_normal[12, x2 + 1:x2 + 3] = 0
    prev_normal[13, x2 + 1, 0] = np.nan
    prev_point[13, x2 + 3, 1] = np.nan
    prev_color[14, x2 + 2, 2] = np.nan
    prev_history[14, x2 + 4] = 0.5
    prev_object[12:15, x3 + 1] = 1
    prev_point[15:17, x3 + 3:x3 + 6] = R.unproject(cam, xx, yy, 5.0, W, H)[15:17, x3 + 3:x3 + 6]    # a recess: another plane
    prev_normal[16, x2:x2 + 3] = -(0.8 * facing + 0.6 * c2w[0, :3])                                # tilted by 37 degrees
    color = np.concatenate([rng.uniform(0, 3, (H, W, 3)), rng.uniform(0, 1, (H, W, 1))], -1)
    color[5, x2 + 4, 1] = np.nan                                 # (valid history: the sample is dropped)
    planes = dict(color=color.astype(F32), point=point.astype(F32), normal=normal.astype(F32), object=obj,
                  prev_color=prev_color.astype(F32), prev_history=prev_history.astype(F32), prev_point=prev_point.astype(F32),
                  prev_normal=prev_normal.astype(F32), prev_object=prev_object, primitive=prim, bary=bary.astype(F32), flags=flags)
    for v in (*planes.values(), t, tris):
        v.setflags(write=False)
    return planes, cam, t, tris, notes


def split(planes):
    """(guides, prev_guides) of the wrappers from a dict of planes."""
    g = {k: planes[k] for k in ("point", "normal", "object", *GUIDES) if planes.get(k) is not None}
    pg = {k[5:]: planes[k] for k in ("prev_point", "prev_normal", "prev_object") if planes.get(k) is not None}
    return g, pg


# ---- the scene of the GPU tests: a sheet of 8 x 8 quads with smooth normals over a floor, one sphere ----
SHEET_N = 8            # quads per side
SHEET_SIZE = 2.4       # world units per side
SHEET_Y = 0.6          # its rest height over the floor
RIPPLE = 0.2           # the ripple's amplitude, world units: see tests/test_gpu_temporal_deform.py for how it was chosen


def sheet_vertices(phase=None, amplitude=RIPPLE):
    """(81, 8) float32 vertices (pos, normal, uv) of the sheet: flat for phase None, otherwise y = SHEET_Y + amplitude *
    sin(3 x + phase) * cos(2.5 z) with the analytic normals of that surface."""
    s = np.linspace(-SHEET_SIZE / 2, SHEET_SIZE / 2, SHEET_N + 1)
    z, x = np.meshgrid(s, s, indexing="ij")
    v = np.zeros((SHEET_N + 1, SHEET_N + 1, 8), np.float64)
    v[..., 0], v[..., 2] = x, z
    v[..., 1] = SHEET_Y
    v[..., 4] = 1.0
    if phase is not None:
        v[..., 1] += amplitude * np.sin(3 * x + phase) * np.cos(2.5 * z)
        dydx = amplitude * 3 * np.cos(3 * x + phase) * np.cos(2.5 * z)
        dydz = -amplitude * 2.5 * np.sin(3 * x + phase) * np.sin(2.5 * z)
        nrm = np.stack([-dydx, np.ones_like(dydx), -dydz], -1)
        v[..., 3:6] = nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)
    v[..., 6], v[..., 7] = (x / SHEET_SIZE + 0.5), (z / SHEET_SIZE + 0.5)
    return v.reshape(-1, 8).astype(F32)


def sheet_indices():
    n = SHEET_N + 1
    idx = []
    for j in range(SHEET_N):
        for i in range(SHEET_N):
            a, b, c, d = j * n + i, j * n + i + 1, (j + 1) * n + i, (j + 1) * n + i + 1
            idx += [a, c, b, b, c, d]             # counter-clockwise seen from above
    return np.array(idx, np.uint32)


def sheet_scene(rt, W, H):
    """The built Scene: mesh 0 the floor (two triangles), mesh 1 the sheet (flat), one lit sphere; the camera looks down at
    the sheet so that it covers most of the W x H frame."""
    sc = rt.Scene()
    # (the look-at transform pitches away from its target's height: a target above the camera makes it look down, at (0, 0.5, 0))
    sc.set_camera((0.0, 2.6, -2.2), (0.0, 4.7, 0.0), fov=60.0, aspect=W / H)
    f = 4.0
    floor = np.array([[-f, 0, -f, 0, 1, 0, 0, 0], [f, 0, -f, 0, 1, 0, 1, 0], [-f, 0, f, 0, 1, 0, 0, 1], [f, 0, f, 0, 1, 0, 1, 1]], F32)
    sc.add_mesh_from_data(floor, np.array([0, 2, 1, 1, 2, 3], np.uint32), mat=rt.material(color=(0.6, 0.6, 0.65, 1.0)))
    sc.add_mesh_from_data(sheet_vertices(), sheet_indices(), mat=rt.material(color=(0.8, 0.4, 0.3, 1.0)))
    sc.add_sphere((1.6, 0.9, 1.4), 0.5, rt.material(color=(1, 1, 1, 1), emission_color=(1, 0.95, 0.9, 1), emission_strength=3.0))
    sc.build()
    return sc


def packed_sheet(sc, vertices8, mesh=1):
    """The sheet's packed triangles for `vertices8`, in the built scene's triangle order (what refit_triangles takes)."""
    idx = sheet_indices().reshape(-1, 3)[sc.triangle_order(mesh)]
    v = np.ascontiguousarray(vertices8, F32)
    t = np.zeros(len(idx), tri_dtype())
    for c, (vn, nn) in enumerate((("v1", "n1"), ("v2", "n2"), ("v3", "n3"))):
        t[vn], t[nn] = v[idx[:, c], 0:3], v[idx[:, c], 3:6]
    t["uv10"], t["uv11"] = v[idx[:, 0], 6], v[idx[:, 0], 7]
    t["uv20"], t["uv21"] = v[idx[:, 1], 6], v[idx[:, 1], 7]
    t["uv30"], t["uv31"] = v[idx[:, 2], 6], v[idx[:, 2], 7]
    return t
