"""An independent numpy restatement of temporal accumulation with a motion table (include/rt_abi.h:
rt_temporal_accumulate_moving) and of rt_object_motions, and the frames their tests run on.

`reference` carries the texels of the moved objects into the previous frame's world in numpy float32 -- one rounded binary32
ufunc per operation, in the order the definition gives -- and hands the carried planes to the restatement of the rest
(tests/_temporal_reference.py: reference).  `object_motions` restates the table.  Neither shares code with csrc/.  `stats`
reports which of the new rules fired where, which the tests use to show that their inputs meet every one.

`synthetic_case` is the 24x16 pair of frames of tests/_temporal_reference.py with object words and records for every new
rule; `moved_mesh` / `guides` give the Cornell fixture with meshes moved, and its planes from oracle.intersect."""
import functools

import numpy as np

import _temporal_reference as R

F32 = R.F32
NO_OBJECT = R.NO_OBJECT


def motion_dtype():
    from ray_tracer_2_amd import _abi as A
    return A.OBJECT_MOTION_DTYPE


def table(n):
    """n records that stand still (identity matrices, moved 0)."""
    t = np.zeros(n, motion_dtype())
    t["d"][:, :3] = np.eye(3, dtype=F32)
    t["nt"][:] = np.eye(3, dtype=F32)
    return t


def record(t, k, linear=None, translation=(0, 0, 0), nt=None):
    """Sets record k of table t to the moved map X' = linear X + translation (float64 3x3, rows by columns) with the normal
    matrix nt (default: the inverse transpose of `linear`), rounded to float32."""
    linear = np.eye(3) if linear is None else np.asarray(linear, np.float64)
    nt = np.linalg.inv(linear).T if nt is None else np.asarray(nt, np.float64)
    t["d"][k, :3] = linear.T            # [col][row]
    t["d"][k, 3] = translation
    t["nt"][k] = nt.T
    t["moved"][k] = 1


def carry(point, normal, obj, motions, stats=None):
    """The carried point and normal planes of the definition, with the texels that take the "no history" result made
    unreprojectable (a zero normal); the texels that are not reprojectable to begin with stay as they are."""
    X, n = np.ascontiguousarray(point, F32), np.ascontiguousarray(normal, F32)
    obj = np.ascontiguousarray(obj, np.uint32)
    n_objects = len(motions)
    with np.errstate(all="ignore"):
        rep = (n != 0).any(-1) & np.isfinite(n).all(-1) & np.isfinite(X).all(-1) & (obj != NO_OBJECT)
        inside = obj < n_objects
        k = np.where(inside, obj, 0)
        moved = rep & inside & (motions["moved"][k] != 0)
        d, nt = motions["d"][k].astype(F32), motions["nt"][k].astype(F32)     # (H, W, 4, 3), (H, W, 3, 3): [col][row]
        Xp = np.stack([((d[..., 0, r] * X[..., 0] + d[..., 1, r] * X[..., 1]) + d[..., 2, r] * X[..., 2]) + d[..., 3, r] for r in range(3)], -1)
        m = np.stack([(nt[..., 0, r] * n[..., 0] + nt[..., 1, r] * n[..., 1]) + nt[..., 2, r] * n[..., 2] for r in range(3)], -1)
        length = np.sqrt((m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2])
        np_ = m / length[..., None]
        assert Xp.dtype == F32 and np_.dtype == F32 and length.dtype == F32
        bad_x, bad_n = ~np.isfinite(Xp).all(-1), ~np.isfinite(np_).all(-1)
        lost = (rep & ~inside) | (moved & (bad_x | bad_n))
        X2 = np.where(moved[..., None], Xp, X)
        n2 = np.where(lost[..., None], F32(0), np.where(moved[..., None], np_, n))
        X2 = np.where(lost[..., None], F32(0), X2)
    if stats is not None:
        stats.update(table_still=rep & inside & ~moved, table_moved=moved, outside_table=rep & ~inside, carried_point_bad=moved & bad_x,
                     zero_length=moved & (length == 0), carried_normal_bad=moved & bad_n, lost=lost)
    return X2.astype(F32), n2.astype(F32)


def reference(planes, prev_camera, motions, max_history=np.inf, point_tolerance=0.01, normal_cos=0.9, stats=None):
    """planes: a dict of R.INPUTS (`object` required, `prev_object` optional); motions: the table.  Returns out, out_history,
    motion; stats receives R.reference's masks and the new rules'."""
    own = {}
    X2, n2 = carry(planes["point"], planes["normal"], planes["object"], motions, own)
    st = {} if stats is None else stats
    res = R.reference(dict(planes, point=X2, normal=n2), prev_camera, max_history, point_tolerance, normal_cos, stats=st)
    st.update(own)
    return res


def mat4_mul(a, b):
    """glam's Mat4 * Mat4 over stacks of column-major float32 matrices [..., col, row]."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    out = np.zeros(a.shape, F32)
    for c in range(4):
        for r in range(4):
            out[..., c, r] = ((a[..., 0, r] * b[..., c, 0] + a[..., 1, r] * b[..., c, 1]) + a[..., 2, r] * b[..., c, 2]) + a[..., 3, r] * b[..., c, 3]
    return out


def object_motions(prev_meshes, meshes, prev_spheres, spheres):
    """rt_object_motions in numpy float32, from MESH_DTYPE / SPHERE_DTYPE arrays."""
    nm, ns = len(meshes), len(spheres)
    t = np.zeros(nm + ns, motion_dtype())
    if nm:
        D = mat4_mul(prev_meshes["model_to_world"], meshes["world_to_model"])
        N = mat4_mul(meshes["model_to_world"], prev_meshes["world_to_model"])
        t["d"][:nm] = D[:, :, :3]
        t["nt"][:nm] = np.swapaxes(N[:, :3, :3], 1, 2)
        bits = lambda a: np.ascontiguousarray(a, F32).view(np.uint32).reshape(nm, -1)   # noqa: E731
        t["moved"][:nm] = ((bits(prev_meshes["world_to_model"]) != bits(meshes["world_to_model"])).any(-1) |
                           (bits(prev_meshes["model_to_world"]) != bits(meshes["model_to_world"])).any(-1))
    if ns:
        with np.errstate(all="ignore"):
            s = prev_spheres["radius"].astype(F32) / spheres["radius"].astype(F32)
            for r in range(3):
                t["d"][nm:, r, r] = s
                t["d"][nm:, 3, r] = prev_spheres["pos"][:, r].astype(F32) - s * spheres["pos"][:, r].astype(F32)
                t["nt"][nm:, r, r] = 1
        u = lambda a: np.ascontiguousarray(a, F32).view(np.uint32)   # noqa: E731
        t["moved"][nm:] = (u(prev_spheres["pos"]) != u(spheres["pos"])).any(-1) | (u(prev_spheres["radius"]) != u(spheres["radius"]))
    return t


def same_records(a, b):
    """Two tables bit for bit (a NaN equals any NaN in the matrices)."""
    return (R.same_bits(a["d"], b["d"]).all() and R.same_bits(a["nt"], b["nt"]).all() and np.array_equal(a["moved"], b["moved"])
            and not a["_p"].any() and not b["_p"].any())


N_OBJECTS = 8
OUTSIDE = 9   # an object word past the table


@functools.lru_cache(maxsize=None)
def synthetic_case():
    """The 24x16 frames of R.synthetic_case with a table of 8 records: 1 (the wall) stands still; 2 (the box) is a moved mesh
    -- rotation, non-uniform scale and translation, its current points and normals placed so that they are carried onto the
    previous box --; 3 is a moved sphere record with a radius change (a patch of the wall in both frames); 4 lands behind
    the previous camera; 5 sends the point to infinity; 6 annihilates the normal; 7 lands off screen; and three texels
    carry the word 9, past the table.  Returns (planes, prev_camera, motions, notes), read-only."""
    planes, cam, notes = R.synthetic_case()
    p = {k: v.copy() for k, v in planes.items()}
    notes = dict(notes)
    c2w = np.array(cam.cam_to_world, np.float64).reshape(4, 4)
    right, forward = c2w[0, :3], c2w[2, :3]
    t = table(N_OBJECTS)
    obj, X, n = p["object"], p["point"].astype(np.float64), p["normal"].astype(np.float64)
    # 2: the box, a moved mesh.  X' = L X + T; the current points are L^-1 (P - T) of the points P that fall on the previous
    # box, the current normals L^T n' normalised, so that the carried ones are the synthetic case's again, to rounding
    a, b = 0.3, -0.2
    rot = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    L, T = rot @ np.diag([1.5, 0.75, 1.25]), np.array([0.4, -0.3, 0.2])
    record(t, 2, L, T)
    box = obj == 2
    X[box] = (X[box] - T) @ np.linalg.inv(L).T
    nb = n[box] @ L                     # (L^T n per row)
    n[box] = nb / np.linalg.norm(nb, axis=-1, keepdims=True)
    # 3: a sphere that shrank to 0.8 of its radius and moved: X' = s X + t with s = 1.25
    s, ts = 1.25, np.array([-0.5, 0.25, 0.125])
    t["d"][3, :3] = np.eye(3, dtype=F32) * F32(s)
    t["d"][3, 3] = ts
    t["moved"][3] = 1
    patch = (slice(10, 12), slice(8, 14))
    obj[patch] = 3
    p["prev_object"][10:13, 10:18] = 3
    X[patch] = (X[patch] - ts) / s
    notes["sphere"] = (10, 9)
    # single texels of row 0 (wall texels that find history in the synthetic case)
    obj[0, 10:13] = OUTSIDE
    notes["outside_table"] = (0, 11)
    record(t, 4, translation=-8.0 * forward)          # behind the previous camera
    obj[0, 22:24] = 4
    notes["moved_behind"] = (0, 22)
    record(t, 5, np.eye(3) * 3e38, (3e38, 3e38, 3e38), nt=np.eye(3))   # X' overflows
    obj[0, 14:16] = 5
    notes["to_infinity"] = (0, 14)
    record(t, 6, nt=np.zeros((3, 3)))                  # len == 0
    obj[0, 17:19] = 6
    notes["no_normal"] = (0, 17)
    record(t, 7, translation=40.0 * right)             # off the previous screen, to the right
    obj[0, 20:22] = 7
    notes["moved_off_screen"] = (0, 20)
    p["point"], p["normal"] = X.astype(F32), n.astype(F32)
    for v in (*p.values(), t):
        v.setflags(write=False)
    return p, cam, t, notes


def small_case(W, H):
    """R.small_case with its one object moved: record 1 a translation, the current points shifted against it."""
    planes, cam = R.small_case(W, H)
    t = table(2)
    shift = np.array([0.25, -0.5, 0.125])
    record(t, 1, translation=shift)
    planes = dict(planes, point=(planes["point"].astype(np.float64) - shift).astype(F32))
    return planes, cam, t


def moved_mesh(arrays, moves):
    """The scene arrays with meshes moved in the world: moves = {mesh index: 4x4 float64 world transform, rows by columns},
    applied on top of the mesh's own -- model_to_world' = T model_to_world, world_to_model' = its float64 inverse."""
    meshes = arrays.meshes.copy()
    for k, T in moves.items():
        m2w = np.array(meshes["model_to_world"][k], np.float64).T      # [col][row] -> rows by columns
        new = np.asarray(T, np.float64) @ m2w
        meshes["model_to_world"][k] = new.T
        meshes["world_to_model"][k] = np.linalg.inv(new).T
    return type(arrays)(arrays.uniform, arrays.spheres, meshes, arrays.triangles, arrays.nodes, arrays.textures)


def rigid(translation=(0, 0, 0), angle=0.0, pivot=(0, 0, 0)):
    """A turn by `angle` about the vertical (y) axis through `pivot`, then a translation: 4x4, rows by columns."""
    c, s = np.cos(angle), np.sin(angle)
    T = np.eye(4)
    T[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    pivot = np.asarray(pivot, np.float64)
    T[:3, 3] = pivot - T[:3, :3] @ pivot + np.asarray(translation, np.float64)
    return T


def centroid(arrays, k):
    """The world centroid of mesh k's vertices."""
    m = arrays.meshes[k]
    tri = arrays.triangles[int(m["triangle_offset"]):int(m["triangle_offset"]) + int(m["triangles"])]
    v = np.concatenate([tri["v1"], tri["v2"], tri["v3"]]).astype(np.float64)
    m2w = np.array(m["model_to_world"], np.float64).T
    return (v @ m2w[:3, :3].T + m2w[:3, 3]).mean(0)


def guides(oracle, arrays, cam, W=67, H=45):
    """R.cornell_guides for scene arrays of the caller's (not cached: the arrays are part of the question here)."""
    from oracle import independent_f64 as F
    arrays = R.with_camera(arrays, cam)
    ro, rd = F.primary_rays(F.Scene(arrays), W, H)
    rec = oracle.intersect(arrays, ro.astype(F32), rd.astype(F32))
    hit = (rec[:, 0] != 0) & np.isfinite(rec[:, 1].view(F32))
    return dict(normal=np.where(hit[:, None], rec[:, 5:8].view(F32), F32(0)).reshape(H, W, 3).astype(F32),
                point=np.where(hit[:, None], rec[:, 2:5].view(F32), F32(0)).reshape(H, W, 3).astype(F32),
                object=np.where(hit, rec[:, 11], np.uint32(NO_OBJECT)).reshape(H, W).astype(np.uint32))
