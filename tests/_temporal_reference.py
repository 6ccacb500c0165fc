"""An independent numpy restatement of temporal accumulation's definition (include/rt_abi.h: rt_temporal_accumulate), and the
frames its tests run on.

`reference` evaluates the definition over the whole frame in numpy float32 -- every operation one rounded binary32 ufunc,
in the order the definition gives, nothing fused; the matrix inverse cofactor by cofactor in float32 (`inverse`).  It
shares no code with csrc/rt_temporal.h.  It also reports which rule fired where (`stats`), which the tests use to show
that their inputs meet every rule.

`synthetic_case` is a 24x16 pair of frames built to meet every rule; `cornell_guides` gives the Cornell fixture's planes
under a camera of the caller's from oracle.intersect on the texel rays."""
import ctypes as C
import functools

import numpy as np

F32 = np.float32
SNAP = F32(1 / 64)
NO_OBJECT = 0xFFFFFFFF
INPUTS = ("color", "point", "normal", "object", "prev_color", "prev_history", "prev_point", "prev_normal", "prev_object")


def inverse(m):
    """glam's scalar Mat4::inverse of the column-major m[col][row], in float32, cofactor by cofactor."""
    m = np.asarray(m, F32)
    (m00, m01, m02, m03), (m10, m11, m12, m13), (m20, m21, m22, m23), (m30, m31, m32, m33) = m
    c00 = m22 * m33 - m32 * m23
    c02 = m12 * m33 - m32 * m13
    c03 = m12 * m23 - m22 * m13
    c04 = m21 * m33 - m31 * m23
    c06 = m11 * m33 - m31 * m13
    c07 = m11 * m23 - m21 * m13
    c08 = m21 * m32 - m31 * m22
    c10 = m11 * m32 - m31 * m12
    c11 = m11 * m22 - m21 * m12
    c12 = m20 * m33 - m30 * m23
    c14 = m10 * m33 - m30 * m13
    c15 = m10 * m23 - m20 * m13
    c16 = m20 * m32 - m30 * m22
    c18 = m10 * m32 - m30 * m12
    c19 = m10 * m22 - m20 * m12
    c20 = m20 * m31 - m30 * m21
    c22 = m10 * m31 - m30 * m11
    c23 = m10 * m21 - m20 * m11
    f0, f1, f2 = np.array([c00, c00, c02, c03], F32), np.array([c04, c04, c06, c07], F32), np.array([c08, c08, c10, c11], F32)
    f3, f4, f5 = np.array([c12, c12, c14, c15], F32), np.array([c16, c16, c18, c19], F32), np.array([c20, c20, c22, c23], F32)
    v0, v1 = np.array([m10, m00, m00, m00], F32), np.array([m11, m01, m01, m01], F32)
    v2, v3 = np.array([m12, m02, m02, m02], F32), np.array([m13, m03, m03, m03], F32)
    sa, sb = np.array([1, -1, 1, -1], F32), np.array([-1, 1, -1, 1], F32)
    inv = np.stack([((v1 * f0 - v2 * f1) + v3 * f2) * sa, ((v0 * f0 - v2 * f3) + v3 * f4) * sb,
                    ((v0 * f1 - v1 * f3) + v3 * f5) * sa, ((v0 * f2 - v1 * f4) + v2 * f5) * sb]).astype(F32)   # inv[col][row]
    det = ((m00 * inv[0][0] + m01 * inv[1][0]) + m02 * inv[2][0]) + m03 * inv[3][0]
    return (inv * (F32(1) / det)).astype(F32)


def camera_arrays(cam):
    """cam_to_world (4, 4) [col][row] and view_params (3,) of a CameraUniform, float32."""
    return np.array(cam.cam_to_world, F32).reshape(4, 4), np.array(cam.view_params, F32)


def reference(planes, prev_camera, max_history=np.inf, point_tolerance=0.01, normal_cos=0.9, stats=None):
    """planes: a dict of INPUTS (the object planes optional).  Returns out (H, W, 4), out_history (H, W), motion (H, W, 2).
    stats (a dict, optional) receives boolean (H, W) masks of where each rule fired."""
    p = {k: np.ascontiguousarray(planes[k], np.uint32 if "object" in k else F32) for k in INPUTS if planes.get(k) is not None}
    color, X, n = p["color"], p["point"], p["normal"]
    H, W = color.shape[:2]
    obj, pobj = p.get("object"), p.get("prev_object")
    c2w, (pw, ph, fd) = camera_arrays(prev_camera)
    V = inverse(c2w)
    tol, ncos, cap = F32(point_tolerance), F32(normal_cos), F32(max_history)
    yy, xx = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        rep = (n != 0).any(-1) & np.isfinite(n).all(-1) & np.isfinite(X).all(-1)
        if obj is not None:
            rep &= obj != NO_OBJECT
        l0, l1, l2 = (((V[0][k] * X[..., 0] + V[1][k] * X[..., 1]) + V[2][k] * X[..., 2]) + V[3][k] for k in range(3))
        fx = (((l0 / l2) * fd) / pw + F32(0.5)) * (F32(W) - F32(1))
        fy = (((l1 / l2) * fd) / ph + F32(0.5)) * (F32(H) - F32(1))
        on = rep & (l2 > 0) & (fx > -1) & (fx < F32(W)) & (fy > -1) & (fy < F32(H))

        def snap(f):
            f = np.where(on, f, F32(0)).astype(F32)
            fl = np.floor(f)
            i0, t = fl.astype(np.int64), f - fl
            lo = t <= SNAP
            hi = ~lo & (t >= F32(1) - SNAP)
            return i0 + hi, np.where(lo | hi, F32(0), t).astype(F32), lo & on, hi & on

        x0, tx, xlo, xhi = snap(fx)
        y0, ty, ylo, yhi = snap(fy)
        motion = np.stack([(x0.astype(F32) + tx) - xx.astype(F32), (y0.astype(F32) + ty) - yy.astype(F32)], -1)
        motion = np.where(on[..., None], motion, F32(np.nan)).astype(F32)
        reach = tol * l2
        total, hsum, wsum = np.zeros((H, W, 4), F32), np.zeros((H, W), F32), np.zeros((H, W), F32)
        fired = {k: np.zeros((H, W), bool) for k in ("outside", "prev_miss", "prev_nan", "history_low", "object", "plane", "normal")}
        nvalid = np.zeros((H, W), int)
        for i in range(4):
            dx, dy = i & 1, i >> 1
            b = (tx if dx else F32(1) - tx) * (ty if dy else F32(1) - ty)
            qx, qy = x0 + dx, y0 + dy
            inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            Q = (np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1))
            m, px, pc, phist = p["prev_normal"][Q], p["prev_point"][Q], p["prev_color"][Q], p["prev_history"][Q]
            live = on & (b > 0)
            hit = (m != 0).any(-1)
            fin = np.isfinite(m).all(-1) & np.isfinite(px).all(-1) & np.isfinite(pc).all(-1) & np.isfinite(phist)
            enough = phist >= 1
            same = np.ones((H, W), bool) if obj is None or pobj is None else pobj[Q] == obj
            a = px - X
            plane = np.abs((a[..., 0] * n[..., 0] + a[..., 1] * n[..., 1]) + a[..., 2] * n[..., 2]) <= reach
            cosine = ((n[..., 0] * m[..., 0] + n[..., 1] * m[..., 1]) + n[..., 2] * m[..., 2]) >= ncos
            valid = live & inside & hit & fin & enough & same & plane & cosine
            total += np.where(valid[..., None], b[..., None] * pc, F32(0))
            hsum += np.where(valid, b * phist, F32(0))
            wsum += np.where(valid, b, F32(0))
            nvalid += valid
            good = live & inside & hit & fin   # (the later rules are counted where the earlier ones let the tap through)
            fired["outside"] |= live & ~inside
            fired["prev_miss"] |= live & inside & ~hit
            fired["prev_nan"] |= live & inside & hit & ~fin
            fired["history_low"] |= good & ~enough
            fired["object"] |= good & enough & ~same
            fired["plane"] |= good & enough & same & ~plane
            fired["normal"] |= good & enough & same & plane & ~cosine
        have = on & (wsum > 0)
        prev = total / wsum[..., None]
        hist = hsum / wsum
        n_c = np.where(hist < cap, hist, cap).astype(F32)
        w = F32(1) / (n_c + F32(1))
        blended = prev * (F32(1) - w)[..., None] + color * w[..., None]
        sample_ok = np.isfinite(color).all(-1)
        out = np.where(have[..., None], np.where(sample_ok[..., None], blended, prev), color).astype(F32)
        out_history = np.where(have, np.where(sample_ok, n_c + F32(1), n_c), F32(1)).astype(F32)
    if stats is not None:
        stats.update(fired, reprojectable=rep, on_screen=on, behind=rep & ~(l2 > 0), left=rep & (l2 > 0) & (fx <= -1),
                     right=rep & (l2 > 0) & (fx >= F32(W)), below=rep & (l2 > 0) & (fy <= -1), above=rep & (l2 > 0) & (fy >= F32(H)),
                     snap_x_down=xlo, snap_x_up=xhi, snap_y_down=ylo, snap_y_up=yhi, have=have, dropped_sample=have & ~sample_ok,
                     capped=have & ~(hist < cap), valid_taps=np.where(on, nvalid, -1))
    return out, out_history, motion


def same_bits(a, b):
    """Bit for bit; a NaN equals any NaN."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def make_camera(A, cam_to_world, view_params):
    cam = A.CameraUniform()
    for c in range(4):
        for r in range(4):
            cam.cam_to_world[c][r] = float(cam_to_world[c][r])
    for k in range(3):
        cam.view_params[k] = float(view_params[k])
    return cam


def moved_camera(cam, right=0.0, up=0.0, forward=0.0):
    """A copy of the CameraUniform translated along its own axes (world units)."""
    new = type(cam).from_buffer_copy(bytes(cam))
    m = np.array(cam.cam_to_world, np.float64).reshape(4, 4)
    t = m[3, :3] + right * m[0, :3] + up * m[1, :3] + forward * m[2, :3]
    for k in range(3):
        new.cam_to_world[3][k] = float(t[k])
    return new


def unproject(cam, fx, fy, depth, W, H):
    """The world point at view depth `depth` that the camera sees at the (fractional) texel position (fx, fy): float64."""
    m = np.array(cam.cam_to_world, np.float64).reshape(4, 4)
    pw, ph, fd = (float(v) for v in cam.view_params)
    fx, fy, depth = np.broadcast_arrays(np.asarray(fx, np.float64), np.asarray(fy, np.float64), np.asarray(depth, np.float64))
    # (a frame one texel wide or high has fx = ux * 0: every position falls on its texel 0)
    local = np.stack([(fx / max(W - 1, 1) - 0.5) * pw, (fy / max(H - 1, 1) - 0.5) * ph, np.full(fx.shape, fd)], -1) * (depth / fd)[..., None]
    return local @ m[:3, :3] + m[3, :3]


def small_case(W, H, seed=7):
    """A W x H wall at depth 4 whose texels fall 0.3 texel right of and above themselves in the previous frame (planes,
    prev_camera): frames of one row or one column."""
    from ray_tracer_2_amd import _abi as A
    rng = np.random.default_rng(seed)
    c2w = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0.5, 0.25, -1, 1]], np.float64)
    cam = make_camera(A, c2w, (1.2, 0.8, 1.5))
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    normal = np.broadcast_to(-c2w[2, :3], (H, W, 3))
    planes = dict(color=rng.uniform(0, 3, (H, W, 4)), point=unproject(cam, xx + 0.3, yy + 0.3, 4.0, W, H), normal=normal,
                  object=np.ones((H, W)), prev_color=rng.uniform(0, 3, (H, W, 4)), prev_history=rng.integers(1, 9, (H, W)),
                  prev_point=unproject(cam, xx, yy, 4.0, W, H), prev_normal=normal, prev_object=np.ones((H, W)))
    return {k: np.ascontiguousarray(v, np.uint32 if "object" in k else F32) for k, v in planes.items()}, cam


@functools.lru_cache(maxsize=None)
def synthetic_case():
    """24x16: a wall at view depth 4 of the previous camera (object 1) with a box in front of it at depth 2.5 (object 2) that
    covers other texels in the two frames; the current texels' hit points are placed by where they are to fall in the
    previous frame -- 2.3 texels right and 0.4 up in general, at chosen fractions, edges and outside positions for single
    texels -- and single texels of every plane carry misses, NaNs, tilted normals, short histories.  Returns (planes,
    prev_camera, notes) with read-only planes; notes names the texels the self-check looks at."""
    from ray_tracer_2_amd import _abi as A
    W, H = 24, 16
    rng = np.random.default_rng(2014)
    a = 0.02   # a slight yaw, so that V is not a pure translation
    c2w = np.array([[np.cos(a), 0, -np.sin(a), 0], [0, 1, 0, 0], [np.sin(a), 0, np.cos(a), 0], [0.3, -0.2, 0.1, 1]], np.float64)
    cam = make_camera(A, c2w, (1.2, 0.8, 1.5))
    facing = -c2w[2, :3]   # both surfaces face the camera
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    # the previous frame: the wall, the box over columns 15 .. 19 of rows 2 .. 9
    pbox = (xx >= 15) & (xx <= 19) & (yy >= 2) & (yy <= 9)
    # (and a recess of the wall, depth 5, under columns 0 .. 4 of rows 4 .. 9: the same object on another plane)
    recess = (xx <= 4) & (yy >= 4) & (yy <= 9)
    prev_point = unproject(cam, xx, yy, np.where(pbox, 2.5, np.where(recess, 5.0, 4.0)), W, H)
    prev_normal = np.broadcast_to(facing, (H, W, 3)).copy()
    prev_object = np.where(pbox, 2, 1).astype(np.uint32)
    prev_color = np.concatenate([rng.uniform(0, 3, (H, W, 3)), rng.uniform(0, 1, (H, W, 1))], -1)
    prev_history = rng.integers(1, 11, (H, W)).astype(np.float64)
    # the current frame: where each texel falls in the previous one; the box now covers columns 10 .. 14 of rows 2 .. 9 and
    # falls onto the previous box (columns 15.3 ..), so the wall texels beside it fall where the box was
    box = (xx >= 10) & (xx <= 14) & (yy >= 2) & (yy <= 9)
    tx = xx + np.where(box, 5.3, 2.3)
    ty = yy + 0.4
    depth = np.where(box, 2.5, 4.0)
    obj = np.where(box, 2, 1).astype(np.uint32)
    notes = {}

    def place(name, y, x, fx, fy):
        tx[y, x], ty[y, x] = fx, fy
        notes[name] = (y, x)

    place("one_tap_down", 1, 1, 3.004, 2.01)        # both axes snap down: one tap
    place("one_tap_up", 1, 2, 3.99, 1.995)          # both snap up
    place("two_taps_x", 1, 3, 5.5, 3.0)             # y snaps: two taps along x
    place("two_taps_y", 1, 4, 6.0, 3.5)             # x snaps: two taps along y
    place("left_edge", 11, 0, -0.5, 11.25)          # on screen, the left taps outside the frame
    place("right_edge", 11, 1, W - 0.5, 11.25)
    place("bottom_edge", 11, 2, 4.25, -0.75)
    place("top_edge", 11, 3, 4.25, H - 0.25)
    place("off_left", 13, 0, -3.0, 5.0)
    place("off_right", 13, 1, W + 2.0, 5.0)
    place("off_below", 13, 2, 5.0, -2.0)
    place("off_above", 13, 3, 5.0, H + 1.0)
    point = unproject(cam, tx, ty, depth, W, H)
    normal = np.broadcast_to(facing, (H, W, 3)).copy()
    color = np.concatenate([rng.uniform(0, 3, (H, W, 3)), rng.uniform(0, 1, (H, W, 1))], -1)
    point[13, 4] = c2w[3, :3] - 2.0 * c2w[2, :3]    # behind the previous camera
    notes["behind"] = (13, 4)
    # misses: row 14 of the current frame, rows 12 and 13 of columns 8 .. 23 of the previous one
    normal[14] = 0
    point[14] = 0
    obj[14] = NO_OBJECT
    prev_normal[12:14, 8:] = 0
    prev_point[12:14, 8:] = 0
    prev_object[12:14, 8:] = NO_OBJECT
    obj[15, 5] = NO_OBJECT                           # the object word alone says miss
    notes["object_says_miss"] = (15, 5)
    # a NaN (or infinity) in each plane
    normal[15, 7, 1] = np.nan
    point[15, 8, 0] = np.inf
    color[4, 3, 1] = np.nan                          # (valid history: the sample is dropped)
    color[4, 4, 3] = np.inf
    notes["dropped"] = (4, 3)
    prev_color[5, 6, 2] = np.nan
    prev_color[6, 2, 3] = np.inf
    prev_history[7, 5] = np.nan
    prev_history[8, 3] = np.inf
    prev_point[9, 6, 1] = np.nan
    prev_normal[9, 9, 0] = np.nan
    # tilted previous normals (37 degrees), short previous histories
    tilt = 0.8 * facing + 0.6 * c2w[0, :3]
    prev_normal[3, 8:11] = tilt
    prev_history[5, 8:11] = 0.5
    prev_history[6, 8] = 0.0
    planes = dict(color=color.astype(F32), point=point.astype(F32), normal=normal.astype(F32), object=obj,
                  prev_color=prev_color.astype(F32), prev_history=prev_history.astype(F32), prev_point=prev_point.astype(F32),
                  prev_normal=prev_normal.astype(F32), prev_object=prev_object)
    for v in planes.values():
        v.setflags(write=False)
    return planes, cam, notes


_guides = {}


def cornell_guides(oracle, arrays, cam, W=67, H=45):
    """The Cornell fixture's `point`, `normal` (zeros on a miss) and `object` (0xffffffff on a miss) planes at W x H under
    the CameraUniform `cam`, from oracle.intersect on the texel rays.  Computed once per camera and size."""
    key = (bytes(cam), W, H)
    if key in _guides:
        return _guides[key]
    from oracle import independent_f64 as F
    arrays = with_camera(arrays, cam)
    ro, rd = F.primary_rays(F.Scene(arrays), W, H)
    rec = oracle.intersect(arrays, ro.astype(F32), rd.astype(F32))
    hit = (rec[:, 0] != 0) & np.isfinite(rec[:, 1].view(F32))
    g = dict(normal=np.where(hit[:, None], rec[:, 5:8].view(F32), F32(0)).reshape(H, W, 3).astype(F32),
             point=np.where(hit[:, None], rec[:, 2:5].view(F32), F32(0)).reshape(H, W, 3).astype(F32),
             object=np.where(hit, rec[:, 11], np.uint32(NO_OBJECT)).reshape(H, W).astype(np.uint32))
    for v in g.values():
        v.setflags(write=False)
    _guides[key] = g
    return g


def with_camera(arrays, cam):
    """The scene arrays under another camera (the arrays themselves are shared)."""
    u = type(arrays.uniform).from_buffer_copy(bytes(arrays.uniform))
    C.memmove(C.byref(u.camera), C.byref(cam), C.sizeof(cam))
    return type(arrays)(u, arrays.spheres, arrays.meshes, arrays.triangles, arrays.nodes, arrays.textures)
