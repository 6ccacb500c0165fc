"""An independent numpy restatement of guided upsampling's definition (include/rt_abi.h: rt_upsample), and the frames its
tests run on.

`reference` evaluates the definition over the whole high frame in numpy float32 -- every operation one rounded binary32
ufunc, in the order the definition gives, nothing fused.  It shares no code with csrc/rt_upsample.h.  It also reports which
rule fired where (`stats`), which the tests use to show that their inputs meet every rule.

`pair` builds a low and a high frame of one procedural scene at any two sizes; `synthetic_case` is the 24x16 -> 61x37 pair
with single texels changed to meet every rule, `snap_case` the 2x2 -> 65x65 pair whose positions hit both snap thresholds
exactly, `cornell_pair` the Cornell fixture's planes at two sizes from the oracle."""
import functools

import numpy as np

F32 = np.float32
SNAP = F32(1 / 64)
NO_OBJECT = 0xFFFFFFFF
FLOOR = F32(2.0 ** -10)
REASONS = ("outside", "color", "object", "lo_miss", "lo_nan", "plane", "normal")


def same_bits(a, b):
    """Bit for bit; a NaN equals any NaN."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def ratio(lo, hi):
    return F32(0) if hi == 1 else (F32(lo) - F32(1)) / (F32(hi) - F32(1))


def snap(f):
    fl = np.floor(f)
    i0, t = fl.astype(np.int64), (f - fl).astype(F32)
    lo = t <= SNAP
    hi = ~lo & (t >= F32(1) - SNAP)
    return i0 + hi, np.where(lo | hi, F32(0), t).astype(F32), lo, hi


def reference(lo, hi, point_tolerance=0.02, normal_cos=0.9, stats=None):
    """lo: color, point, normal, object[, albedo] of the low frame; hi: depth, point, normal, object[, albedo][, emission]
    of the high one.  Returns out (H, W, 4) float32 and coverage (H, W) uint8."""
    lc, lx, ln = (np.ascontiguousarray(lo[k], F32) for k in ("color", "point", "normal"))
    lobj = np.ascontiguousarray(lo["object"], np.uint32)
    depth, X, n = (np.ascontiguousarray(hi[k], F32) for k in ("depth", "point", "normal"))
    obj = np.ascontiguousarray(hi["object"], np.uint32)
    assert ("albedo" in lo) == ("albedo" in hi)
    lal = np.ascontiguousarray(lo["albedo"], F32) if "albedo" in lo else None
    al = np.ascontiguousarray(hi["albedo"], F32) if "albedo" in hi else None
    em = np.ascontiguousarray(hi["emission"], F32) if "emission" in hi else None
    h, w = lobj.shape
    H, W = obj.shape
    tol, ncos = F32(point_tolerance), F32(normal_cos)
    with np.errstate(all="ignore"):
        x0, tx, xlo, xhi = snap(np.arange(W, dtype=F32) * ratio(w, W))
        y0, ty, ylo, yhi = snap(np.arange(H, dtype=F32) * ratio(h, H))
        x0, tx = np.broadcast_to(x0[None, :], (H, W)), np.broadcast_to(tx[None, :], (H, W))
        y0, ty = np.broadcast_to(y0[:, None], (H, W)), np.broadcast_to(ty[:, None], (H, W))
        guided = (n != 0).any(-1) & np.isfinite(n).all(-1) & np.isfinite(X).all(-1) & np.isfinite(depth) & (depth > 0) & (obj != NO_OBJECT)
        if em is not None:
            guided &= (em[..., :3] == 0).all(-1)
        demod = guided & (al is not None)
        reach = tol * depth
        if lal is not None:
            ldem = lc.copy()
            ldem[..., :3] = lc[..., :3] / np.where(lal[..., :3] > FLOOR, lal[..., :3], FLOOR)
        fired = {k: np.zeros((H, W), bool) for k in REASONS}
        alone = {k: np.zeros((H, W), bool) for k in REASONS}

        def c_of(Q):
            return np.where(demod[..., None], ldem[Q], lc[Q]).astype(F32) if lal is not None else lc[Q]

        def ring(taps, count_where):
            total, wsum, nvalid = np.zeros((H, W, 4), F32), np.zeros((H, W), F32), np.zeros((H, W), int)
            for qx, qy, b in taps:
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                Q = (np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1))
                c, m, px = lc[Q], ln[Q], lx[Q]
                a = px - X
                fails = {"outside": ~inside, "color": ~np.isfinite(c).all(-1), "object": lobj[Q] != obj,
                         "lo_miss": guided & ~(m != 0).any(-1), "lo_nan": guided & ~(np.isfinite(m).all(-1) & np.isfinite(px).all(-1)),
                         "plane": guided & ~(np.abs((a[..., 0] * n[..., 0] + a[..., 1] * n[..., 1]) + a[..., 2] * n[..., 2]) <= reach),
                         "normal": guided & ~(((n[..., 0] * m[..., 0] + n[..., 1] * m[..., 1]) + n[..., 2] * m[..., 2]) >= ncos)}
                live = b > 0
                valid = live.copy()
                for f in fails.values():
                    valid &= ~f
                total += np.where(valid[..., None], b[..., None] * c_of(Q), F32(0))
                wsum += np.where(valid, b, F32(0))
                nvalid += valid
                # (a zero or non-finite normal or point also fails the plane or the cosine test, which read it: a tap refused
                # for what the low texel holds is "alone" when nothing but those two joins it)
                nfail = sum(f.astype(int) for f in fails.values())
                implied = fails["plane"].astype(int) + fails["normal"].astype(int)
                for k, f in fails.items():
                    fired[k] |= live & f & count_where
                    alone[k] |= live & f & ((nfail - implied if k in ("lo_miss", "lo_nan") else nfail) == 1) & count_where
            return total, wsum, nvalid

        one = F32(1)
        taps1 = [(x0 + (i & 1), y0 + (i >> 1), ((tx if i & 1 else one - tx) * (ty if i >> 1 else one - ty)).astype(F32)) for i in range(4)]
        s1, w1, nvalid = ring(taps1, np.ones((H, W), bool))
        have1 = w1 > 0
        taps2 = [(x0 + i, y0 + j, ((one - np.abs(F32(i) - tx) * F32(0.5)) * (one - np.abs(F32(j) - ty) * F32(0.5))).astype(F32))
                 for j in range(-1, 3) for i in range(-1, 3)]
        s2, w2, nvalid2 = ring(taps2, ~have1)
        have2 = ~have1 & (w2 > 0)
        near = (np.clip(y0 + (ty > F32(0.5)), 0, h - 1), np.clip(x0 + (tx > F32(0.5)), 0, w - 1))
        v = np.where(have1[..., None], s1 / w1[..., None], np.where(have2[..., None], s2 / w2[..., None], c_of(near))).astype(F32)
        out = v.copy()
        if al is not None:
            out[..., :3] = np.where(demod[..., None], v[..., :3] * al[..., :3], v[..., :3])
        coverage = np.where(have1, 2, np.where(have2, 1, 0)).astype(np.uint8)
    if stats is not None:
        stats.update(fired=fired, alone=alone, guided=guided, demod=demod, valid_taps=nvalid, valid_taps2=np.where(have1, -1, nvalid2),
                     snap_x_down=np.broadcast_to(xlo[None, :], (H, W)), snap_x_up=np.broadcast_to(xhi[None, :], (H, W)),
                     snap_y_down=np.broadcast_to(ylo[:, None], (H, W)), snap_y_up=np.broadcast_to(yhi[:, None], (H, W)),
                     x0=x0, y0=y0, tx=tx, ty=ty)
    return out, coverage


# ---- frames ----
def _scene(nx, ny):
    """The procedural scene at nx x ny texels: six slanted panels (objects 1 .. 6) at their own depths, a corner of misses."""
    u = (np.arange(nx, dtype=np.float64) / (nx - 1)) if nx > 1 else np.zeros(1)
    v = (np.arange(ny, dtype=np.float64) / (ny - 1)) if ny > 1 else np.zeros(1)
    u, v = np.meshgrid(u, v)
    obj = (1 + np.floor(u * 2.999) + 3 * np.floor(v * 1.999)).astype(np.uint32)
    px, py = 2 * u - 1, 1.5 * v - 0.75
    z = 3 + 0.5 * obj + 0.3 * px
    point = np.stack([px, py, z], -1)
    normal = np.broadcast_to(np.array([0.3, 0, -1]) / np.hypot(0.3, 1), point.shape).copy()
    depth = z.copy()
    albedo = np.stack([0.2 + 0.6 * u, 0.8 - 0.5 * v, 0.3 + 0.4 * u * v, np.ones_like(u)], -1)
    miss = (u > 0.8) & (v > 0.8)
    obj[miss] = NO_OBJECT
    point[miss] = 0
    normal[miss] = 0
    depth[miss] = 0
    albedo[miss] = 0
    return dict(object=obj, point=point, normal=normal, depth=depth, albedo=albedo, emission=np.zeros(albedo.shape))


def _finish(lo, hi):
    lo = {k: np.ascontiguousarray(v, np.uint32 if k == "object" else F32) for k, v in lo.items() if k in ("color", "point", "normal", "object", "albedo")}
    hi = {k: np.ascontiguousarray(v, np.uint32 if k == "object" else F32) for k, v in hi.items()}
    for d in (lo, hi):
        for v in d.values():
            v.setflags(write=False)
    return lo, hi


def _raw_pair(w, h, W, H, seed):
    rng = np.random.default_rng(seed)
    lo, hi = _scene(w, h), _scene(W, H)
    lo["color"] = np.concatenate([rng.uniform(0, 3, (h, w, 3)), rng.uniform(0, 1, (h, w, 1))], -1)
    return lo, hi


@functools.lru_cache(maxsize=None)
def pair(w, h, W, H, seed=5):
    """(lo, hi): read-only planes of the procedural scene at the two sizes, the low frame with a random colour."""
    return _finish(*_raw_pair(w, h, W, H, seed))


def without(d, *names):
    return {k: v for k, v in d.items() if k not in names}


@functools.lru_cache(maxsize=None)
def synthetic_case():
    """24x16 -> 61x37 (panels of 8 x 8 low texels), single low texels three apart changed so that each reason a tap is
    refused occurs alone, a foreign 2 x 2 block (ring 2) and a 4 x 4 one (a hole), a lamp, albedos at and below the floor,
    and single high texels that are PLAIN for each reason.  Returns (lo, hi, notes): notes names the texels (low
    coordinates (y, x) for the low frame's, high ones for the high frame's)."""
    w, h, W, H = 24, 16, 61, 37
    lo, hi = _raw_pair(w, h, W, H, 2018)
    tilt = np.array([0.3, 0.75, -1.0])
    notes = dict(color_nan=(2, 2), color_inf=(2, 5), object=(5, 2), lo_miss=(5, 5), normal_nan=(2, 10), point_inf=(2, 13), plane=(5, 10),
                 tilt=(5, 13), floor_a=(10, 10), floor_b=(10, 13), floor_c=(13, 10), floor_nan=(13, 13))
    lo["color"][2, 2, 1] = np.nan
    lo["color"][2, 5, 3] = np.inf
    lo["object"][5, 2] = 99
    lo["normal"][5, 5] = 0
    lo["normal"][2, 10, 0] = np.nan
    lo["point"][2, 13, 2] = np.inf
    lo["point"][5, 10, 2] += 1.0
    lo["normal"][5, 13] = tilt / np.linalg.norm(tilt)
    lo["object"][0:2, 18:20] = 9           # a foreign block of 2 x 2 at the frame's edge: the texels over it reach ring 2, and outside
    lo["object"][10:14, 2:6] = 9           # ... of 4 x 4: those over its middle find nothing
    lo["albedo"][10, 10, :3] = [1e-4, 0.5, 2.0 ** -10]
    lo["albedo"][10, 13, :3] = [0, -1, 0.25]
    lo["albedo"][13, 10, :3] = 2.0 ** -11
    lo["albedo"][13, 13, 0] = np.nan
    # a lamp: object 50 on both sides, emissive on the high one
    lo["object"][5:7, 21:23] = 50
    fx, fy = np.arange(W) * (w - 1) / (W - 1), np.arange(H) * (h - 1) / (H - 1)
    lamp = ((np.rint(fy) >= 5) & (np.rint(fy) <= 6))[:, None] & ((np.rint(fx) >= 21) & (np.rint(fx) <= 22))[None, :]
    hi["object"][lamp] = 50
    hi["emission"][lamp] = [5, 4, 3, 1]
    notes["lamp"] = lamp
    # PLAIN high texels, and one of an object the low frame does not hold
    hi["normal"][20, 30, 1] = np.nan
    hi["point"][20, 34, 0] = np.inf
    hi["depth"][20, 38] = 0
    hi["depth"][20, 42] = np.nan
    hi["object"][24, 30] = 77
    hi["albedo"][24, 34, :3] = 0
    notes.update(hi_normal_nan=(20, 30), hi_point_inf=(20, 34), hi_depth_zero=(20, 38), hi_depth_nan=(20, 42), hi_alone=(24, 30),
                 hi_black=(24, 34))
    return (*_finish(lo, hi), notes)


@functools.lru_cache(maxsize=None)
def snap_case():
    """2x2 -> 65x65 on one panel: rx = 1/64 exactly, so t = 1/64 at X = 1 (snaps down) and 63/64 at X = 63 (snaps up)."""
    lo, hi = _raw_pair(2, 2, 65, 65, 11)
    for d in (lo, hi):
        d["object"][:] = 1
        d["normal"][:] = [0, 0, -1]
        d["point"][..., 2] = 4
        d["depth"][:] = 4
        d["albedo"][:] = 0.5
    return _finish(lo, hi)


_cornell = {}


def cornell_planes(oracle, arrays, W, H):
    """The Cornell fixture's G-buffer at W x H from oracle.intersect on the texel rays: depth (the ray's t), point, normal
    (zeros on a miss), object (0xffffffff on a miss), emission (the winning object's material) and an albedo of ones."""
    if (W, H) in _cornell:
        return _cornell[(W, H)]
    from oracle import independent_f64 as F
    ro, rd = F.primary_rays(F.Scene(arrays), W, H)
    rec = oracle.intersect(arrays, ro.astype(F32), rd.astype(F32))
    hit = (rec[:, 0] != 0) & np.isfinite(rec[:, 1].view(F32))
    mats = np.concatenate([arrays.meshes["material"], arrays.spheres["material"]])
    emission = np.zeros((H * W, 4), F32)
    m = mats[rec[hit, 11]]
    emission[hit] = (m["emission_color"] * m["emission_strength"][:, None]).astype(F32)
    g = dict(depth=np.where(hit, rec[:, 1].view(F32), F32(0)).reshape(H, W).astype(F32),
             point=np.where(hit[:, None], rec[:, 2:5].view(F32), F32(0)).reshape(H, W, 3).astype(F32),
             normal=np.where(hit[:, None], rec[:, 5:8].view(F32), F32(0)).reshape(H, W, 3).astype(F32),
             object=np.where(hit, rec[:, 11], np.uint32(NO_OBJECT)).reshape(H, W).astype(np.uint32),
             albedo=np.ones((H, W, 4), F32), emission=emission.reshape(H, W, 4))
    for v in g.values():
        v.setflags(write=False)
    _cornell[(W, H)] = g
    return g
