"""Helpers of the ray-query tests (tests/test_gpu_ray_query.py): the probe's 16-word records side by side with rt_hit
records, the texture coordinates of a triangle hit recomputed in binary32, and a float64 brute force over ALL hits of a
ray (not only the closest), which tells which rays have some hit near a given distance."""
import numpy as np

F32 = np.float32


def hits_as_probe_words(hits):
    """rt_hit records -> the words of the probe's record (include/rt_test_abi.h) they must equal: hit, dst, point,
    normal, u, v, backface, winner.  (n, 12) u32."""
    n = len(hits)
    w = np.zeros((n, 12), np.uint32)
    hit = (hits["flags"] & 1) != 0
    w[:, 0] = hit
    w[:, 1] = hits["t"].view(np.uint32)
    w[:, 2:5] = hits["point"].view(np.uint32)
    w[:, 5:8] = hits["normal"].view(np.uint32)
    w[:, 8] = hits["tex_u"].view(np.uint32)
    w[:, 9] = hits["tex_v"].view(np.uint32)
    w[:, 10] = (hits["flags"] >> 1) & 1
    w[:, 11] = hits["object"]
    return w


def filtered_probe_words(rec, tmax):
    """The probe's records (words 0..11) with a hit at t >= tmax turned into the query's miss record."""
    w = rec[:, :12].copy()
    t = rec[:, 1].view(F32)
    keep = (rec[:, 0] != 0) & (t < np.asarray(tmax, F32))
    miss = np.zeros(12, np.uint32)
    miss[1] = np.array(np.inf, F32).view(np.uint32)
    miss[11] = 0xFFFFFFFF
    w[~keep] = miss
    return w, keep


def tex_uv_f32(tri, bu, bv):
    """isect_finish's texture coordinates in binary32: w = (1 - u) - v, uv = (uv1 w + uv2 u) + uv3 v, in that order."""
    u, v = F32(bu), F32(bv)
    w = (F32(1.0) - u) - v
    tu = (F32(tri["uv10"]) * w + F32(tri["uv20"]) * u) + F32(tri["uv30"]) * v
    tv = (F32(tri["uv11"]) * w + F32(tri["uv21"]) * u) + F32(tri["uv31"]) * v
    return F32(tu), F32(tv)


def _mat(m, key):
    return np.asarray(m[key], np.float64)   # [col][row]


def _apply(c, p, w):
    return p @ c[:3, :3] + w * c[3, :3]


def hit_distances_f64(arrays, ro, rd, ray_block=512):
    """Float64, per ray, the world distances of every triangle and sphere the ray meets (both faces, t > 0): a list of
    1-D arrays.  A brute force over all primitives: meant for small scenes."""
    ro = np.asarray(ro, np.float64)
    rd = np.asarray(rd, np.float64)
    rd = rd / np.linalg.norm(rd, axis=1, keepdims=True)
    n = len(ro)
    out = [[] for _ in range(n)]
    for m in arrays.meshes:
        w2m, m2w = _mat(m, "world_to_model"), _mat(m, "model_to_world")
        t0, nt = int(m["triangle_offset"]), int(m["triangles"])
        tr = arrays.triangles[t0:t0 + nt]
        v1, v2, v3 = (np.asarray(tr[k], np.float64) for k in ("v1", "v2", "v3"))
        e1, e2 = v2 - v1, v3 - v1
        for b in range(0, n, ray_block):
            lo = _apply(w2m, ro[b:b + ray_block], 1.0)
            ld = _apply(w2m, rd[b:b + ray_block], 0.0)
            ld = ld / np.linalg.norm(ld, axis=1, keepdims=True)
            p = np.cross(ld[:, None, :], e2[None, :, :])
            det = np.einsum("tk,rtk->rt", e1, p)
            with np.errstate(divide="ignore", invalid="ignore"):
                inv = 1.0 / det
                s = lo[:, None, :] - v1[None, :, :]
                u = np.einsum("rtk,rtk->rt", s, p) * inv
                q = np.cross(s, e1[None, :, :])
                v = np.einsum("rk,rtk->rt", ld, q) * inv
                t = np.einsum("tk,rtk->rt", e2, q) * inv
            ok = (np.abs(det) > 1e-12) & (u >= -1e-6) & (v >= -1e-6) & (u + v <= 1 + 1e-6) & (t > 0)
            for r, j in zip(*np.nonzero(ok)):
                pw = _apply(m2w, lo[r] + ld[r] * t[r, j], 1.0)
                out[b + r].append(np.linalg.norm(pw - ro[b + r]))
    for s in arrays.spheres:
        c, rad = np.asarray(s["pos"], np.float64), float(s["radius"])
        oc = ro - c
        bq = np.einsum("rk,rk->r", oc, rd)
        disc = bq * bq - (np.einsum("rk,rk->r", oc, oc) - rad * rad)
        for r in np.flatnonzero(disc >= 0):
            sq = np.sqrt(disc[r])
            for t in (-bq[r] - sq, -bq[r] + sq):
                if t > 0:
                    out[r].append(t)
    return [np.asarray(x) for x in out]


def near_band(dists, tmax, rel=1e-5):
    """Per ray: does some hit lie within a relative `rel` of tmax (where occlusion may legitimately disagree with the
    filtered closest hit: the world distance of a binary32 t is not exactly monotone)?"""
    tmax = np.broadcast_to(np.asarray(tmax, np.float64), (len(dists),))
    return np.array([bool(len(d)) and bool(np.isfinite(tm)) and bool(np.any(np.abs(d - tm) <= rel * tm))
                     for d, tm in zip(dists, tmax)], bool)
