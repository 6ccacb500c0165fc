"""independent_f64.py -- TEST INFRASTRUCTURE: a second, independent restatement of the path-trace loop of
/root/reference/shaders/ray_tracer.wgsl in float64 numpy: meshes, spheres, glass, textured materials, depth of field (the
Cornell box of BASELINE configs[0..1] and the scene library's `room`, `metal`, `balls`, `texture_test`).

Why it exists.  oracle/shader_oracle.cpp and the HIP kernels compile the same headers (csrc/rt_transc.h,
rt_texture.h): the polynomials for log / sin / cos / pow, the two-step normalize and the rounding of every operation
are DEFINED there, so the kernels' bit-for-bit parity with the oracle cannot notice a wrong definition.  This file
shares nothing with them: double precision, numpy / libm `log`, `cos`, `sin`, `sqrt`, `power`, true division, the
shader's literal constants, and no BVH at all (every triangle of every mesh is tested: in exact arithmetic the BVH
only skips triangles that cannot be the closest hit).  It pins the canonical float32 arithmetic STATISTICALLY -- the
closest available stand-in for north_star's "within 1e-5 of the reference render", which cannot be evaluated here
(the reference cannot be built or run: SURVEY.md section 8c) -- and guards later redefinitions of that arithmetic.

Only tests/ may import this module (and tests/golden/make_f64_pin.py, which writes the committed statistics).
PARITY UNPINNED like the rest of oracle/ (no vectors exist in the reference).

Each function cites the wgsl lines it follows (all `file:line` relative to /root/reference/shaders/ray_tracer.wgsl).
"""
import numpy as np

EPSILON = 1e-5                     # :131
INF = float.fromhex("0x1p+127")    # :132
PI = 3.1415926                     # the shader's literal (:182,203)
SKY_HORIZON = np.array([1.0, 1.0, 1.0, 0.0])                   # :126
SKY_ZENITH = np.array([0.0788092, 0.36480793, 0.7264151, 0.0])  # :127
GROUND_COLOR = np.array([0.35, 0.3, 0.35, 0.0])                # :128


class Rng:
    """:195-200 on a vector of u32 states (exact integer arithmetic); rand :164-166 as a double division."""

    def __init__(self, state):
        self.s = state.astype(np.uint64)

    def next(self, mask=None):
        m = np.uint64(0xffffffff)
        s = (self.s * np.uint64(747796405) + np.uint64(2891336453)) & m
        if mask is not None:
            s = np.where(mask, s, self.s)
        self.s = s
        r = (((s >> ((s >> np.uint64(28)) + np.uint64(4))) ^ s) * np.uint64(277803737)) & m
        return (r >> np.uint64(22)) ^ r

    def rand(self, mask=None):
        return self.next(mask).astype(np.float64) / 4294967295.0   # :165 (2^32 - 1, exactly, in double)

    def in_unit_disk(self, mask=None):   # :202-206
        angle = self.rand(mask) * 2.0 * PI
        r = np.sqrt(self.rand(mask))
        return np.cos(angle) * r, np.sin(angle) * r


def dot(a, b):
    return (a * b).sum(-1)


def normalize(v):
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.sqrt(dot(v, v))[..., None]


def smoothstep(lo, hi, x):   # WGSL builtin
    t = np.clip((x - lo) / (hi - lo), 0.0, 1.0)
    return t * t * (3.0 - 2.0 * t)


def mix(a, b, t):
    return a * (1.0 - t) + b * t


def environment_light(d):   # :214-221
    y = d[:, 1]
    sky_t = np.power(smoothstep(0.0, 0.4, y), 0.35)
    g2s = smoothstep(-0.01, 0.0, y)
    sky = mix(SKY_HORIZON[None, :], SKY_ZENITH[None, :], sky_t[:, None])
    sun = np.power(np.maximum(0.0, dot(d, np.array([0.1, 1.0, 0.1]))), 500.0) * 0.1
    return mix(GROUND_COLOR[None, :], sky, g2s[:, None]) + (sun * (g2s >= 1.0))[:, None]


MAT_FIELDS = ("color", "emission_color", "specular_color", "absorption", "absorption_strength", "emission_strength", "smoothness",
              "specular", "ior", "flag", "diffuse_index")


class Scene:
    """The reference's arrays (MeshUniform / PackedTriangle / Sphere / textures, include/rt_abi.h section 1) as doubles.
    Triangles are taken per mesh by walking the mesh's BVH nodes for their leaf ranges only -- the boxes are never used.
    Materials: mesh materials first, then the spheres' (index = number of meshes + sphere index)."""

    def __init__(self, arrays):
        self.cam_to_world = np.array(arrays.uniform.camera.cam_to_world, np.float64)   # [col][row]
        self.view_params = np.array(arrays.uniform.camera.view_params, np.float64)
        self.defocus = float(arrays.uniform.camera.defocus_strength)
        self.diverge = float(arrays.uniform.camera.diverge_strength)
        self.meshes = []
        t = arrays.triangles
        mats = []
        for m in arrays.meshes:
            idx = self._leaf_triangles(arrays.nodes, int(m["node_offset"]), int(m["triangle_offset"]))
            f = lambda k: t[k][idx].astype(np.float64)  # noqa: E731
            self.meshes.append(dict(
                w2m=np.array(m["world_to_model"], np.float64), m2w=np.array(m["model_to_world"], np.float64),
                v1=f("v1"), v2=f("v2"), v3=f("v3"), n1=f("n1"), n2=f("n2"), n3=f("n3"),
                uv1=np.stack([f("uv10"), f("uv11")], -1), uv2=np.stack([f("uv20"), f("uv21")], -1),
                uv3=np.stack([f("uv30"), f("uv31")], -1), glass=int(m["material"]["flag"]) == 1))
            mats.append(m["material"])
        self.sphere_pos = np.array([sp["pos"] for sp in arrays.spheres], np.float64).reshape(-1, 3)
        self.sphere_radius = np.array([sp["radius"] for sp in arrays.spheres], np.float64)
        mats += [sp["material"] for sp in arrays.spheres]
        self.n_meshes = len(self.meshes)
        for k in MAT_FIELDS:
            setattr(self, "mat_" + k, np.array([np.asarray(mm[k]) for mm in mats], np.float64 if k not in ("flag", "diffuse_index") else np.int64))
        self.textures = [np.asarray(tex, np.uint8) for tex in arrays.textures]   # (H, W, 4) sRGB, already flipped by the loader

    @staticmethod
    def _leaf_triangles(nodes, node_offset, tri_offset):
        out, st = [], [0]
        while st:
            n = nodes[node_offset + st.pop()]
            if n["count"] > 0:
                out.extend(range(tri_offset + int(n["first"]), tri_offset + int(n["first"]) + int(n["count"])))
            else:
                st.extend([int(n["right"]), int(n["left"])])
        return np.array(out, np.int64)


def srgb_to_linear(c8):
    """The sRGB decode of an Rgba8UnormSrgb texture fetch (src/rendering/ray_tracer.rs:253), from the IEC 61966-2-1 formula."""
    c = c8.astype(np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, np.power((c + 0.055) / 1.055, 2.4))


def sample_texture(tex, u, v):
    """textureSampleLevel(.., uv, 0.0) with the reference's sampler (src/rendering/ray_tracer.rs:197-205): bilinear, repeat,
    texel centres at (i + 0.5) / size, sRGB decoded before filtering, alpha linear.  wgsl:455."""
    h, w = tex.shape[:2]
    px, py = u * w - 0.5, v * h - 0.5
    x0, y0 = np.floor(px), np.floor(py)
    fx, fy = (px - x0)[:, None], (py - y0)[:, None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)

    def texel(x, y):
        t = tex[np.mod(y, h), np.mod(x, w)]
        return np.concatenate([srgb_to_linear(t[:, :3]), t[:, 3:4].astype(np.float64) / 255.0], -1)
    top = texel(x0, y0) * (1.0 - fx) + texel(x0 + 1, y0) * fx
    bot = texel(x0, y0 + 1) * (1.0 - fx) + texel(x0 + 1, y0 + 1) * fx
    return top * (1.0 - fy) + bot * fy


def mat_point(m, v, w):   # (mat4 * vec4(v, w)).xyz, m[col][row]
    return v[:, 0:1] * m[0, :3] + v[:, 1:2] * m[1, :3] + v[:, 2:3] * m[2, :3] + w * m[3, :3]


# Ray-triangle tests are evaluated for blocks of rays x triangles of at most this many pairs (memory stays bounded: the
# dragon stand-in's 78 k triangles against 10^5 rays would be 10^10 doubles per array at once).
PAIRS_PER_BLOCK = 1 << 21
TRIS_PER_CHUNK = 256


def _chunk_bounds(m):
    """Bounding spheres of consecutive runs of TRIS_PER_CHUNK triangles (the leaf order keeps a run compact): centre, and
    a radius enlarged by 1 % + 1e-6 of the mesh's scale so that no triangle a test below can count as (nearly) hit is
    outside it."""
    if "chunks" not in m:
        nt = m["v1"].shape[0]
        scale = max(float(np.abs(np.concatenate([m["v1"], m["v2"], m["v3"]])).max(initial=0.0)), 1e-30)
        out = []
        for a in range(0, nt, TRIS_PER_CHUNK):
            b = min(nt, a + TRIS_PER_CHUNK)
            pts = np.concatenate([m["v1"][a:b], m["v2"][a:b], m["v3"][a:b]])
            c = 0.5 * (pts.min(0) + pts.max(0))
            rad = np.sqrt(((pts - c) ** 2).sum(-1).max())
            out.append((a, b, c, rad * 1.01 + 1e-6 * scale))
        m["chunks"] = out
    return m["chunks"]


def _triangle_chunks(m, lo, ld):
    """ray_triangle :258-290 of every (ray, triangle) pair that can matter, in blocks: yields (ray rows, triangle indices,
    dict of (rows, triangles) arrays keep / det / dst / u / v / w / nrm_len / eab_len / eac_len).  A block holds the rays
    whose half-line passes within a run's bounding sphere (all others miss every triangle of the run, with room to spare);
    the triangles come in increasing index order."""
    for a, b, c, rad in _chunk_bounds(m):
        oc = c - lo
        t = np.maximum(dot(oc, ld), 0.0)
        near = np.sqrt(np.maximum(dot(oc, oc) - 2.0 * t * dot(oc, ld) + t * t, 0.0))
        rows_all = np.flatnonzero(near <= rad)
        if rows_all.size == 0:
            continue
        tris = np.arange(a, b)
        step = max(1, PAIRS_PER_BLOCK // tris.size)
        for s0 in range(0, rows_all.size, step):
            rows = rows_all[s0:s0 + step]
            v1 = m["v1"][a:b]
            eab, eac = m["v2"][a:b] - v1, m["v3"][a:b] - v1        # :261-262
            nrm = np.cross(eab, eac)                                # :263
            l0, d0 = lo[rows], ld[rows]
            ao = l0[:, None, :] - v1[None, :, :]                    # :264
            dao = np.cross(ao, d0[:, None, :])                      # :265
            det = -(d0[:, None, :] * nrm[None]).sum(-1)             # :266
            keep = (np.abs(det) >= 1e-8) if m["glass"] else (det >= 1e-8)   # :268 (cull_backface = not glass, :375)
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                inv = 1.0 / det
                dst = (ao * nrm[None]).sum(-1) * inv
                u = (eac[None] * dao).sum(-1) * inv
                v = -(eab[None] * dao).sum(-1) * inv
            w = 1.0 - u - v
            yield rows, tris, dict(keep=keep, det=det, dst=dst, u=u, v=v, w=w, nrm_len=np.sqrt(dot(nrm, nrm))[None, :],
                                   eab_len=np.sqrt(dot(eab, eab))[None, :], eac_len=np.sqrt(dot(eac, eac))[None, :])


def closest_hit(scene, ro, rd):
    """calculate_ray_collions :353-396: ray_sphere :223-256 over the spheres, then ray_triangle :258-290 over ALL triangles
    of every mesh.  Returns hit mask, world distance, world hit point, world normal, uv, material index, backface."""
    n = ro.shape[0]
    best = np.full(n, INF)
    hit = np.zeros(n, bool)
    point = np.zeros((n, 3))
    normal = np.zeros((n, 3))
    uv = np.zeros((n, 2))
    which = np.full(n, -1)
    backface = np.zeros(n, bool)
    for si in range(scene.sphere_pos.shape[0]):             # :359-367
        oc = ro - scene.sphere_pos[si]
        a = dot(rd, rd)
        b = 2.0 * dot(oc, rd)
        c = dot(oc, oc) - scene.sphere_radius[si] ** 2
        disc = b * b - 4.0 * a * c
        ok = disc >= 0.0
        with np.errstate(invalid="ignore", divide="ignore"):
            sq = np.sqrt(np.where(ok, disc, 0.0))
            near = np.maximum(0.0, (-b - sq) / (2.0 * a))
            far = (-b + sq) / (2.0 * a)
        ok &= far >= 0.001
        inside = near == 0.0
        dst = np.where(inside, far, near)
        better = ok & (dst < best)                          # :362
        hp = ro + rd * dst[:, None]
        nrm = normalize(hp - scene.sphere_pos[si])
        nrm = np.where(inside[:, None], -nrm, nrm)
        with np.errstate(invalid="ignore"):
            theta = np.arccos(np.clip(-nrm[:, 1], -1.0, 1.0))
        phi = np.arctan2(-nrm[:, 2], -nrm[:, 0]) + PI
        suv = np.stack([phi / (2.0 * PI), theta / PI], -1)
        best = np.where(better, dst, best)
        hit |= better
        point = np.where(better[:, None], hp, point)
        normal = np.where(better[:, None], nrm, normal)
        uv = np.where(better[:, None], suv, uv)
        which = np.where(better, scene.n_meshes + si, which)
        backface = np.where(better, inside, backface)
    r = np.arange(n)
    for mi, m in enumerate(scene.meshes):
        lo = mat_point(m["w2m"], ro, 1.0)                  # :371
        ld = normalize(mat_point(m["w2m"], rd, 0.0))       # :372
        # the closest triangle of the mesh (ray_BVH keeps strictly closer hits): the first minimum in triangle order,
        # gathered chunk by chunk (a later chunk wins only when strictly closer)
        tk = np.full(n, np.inf)
        k = np.zeros(n, np.int64)
        uk, vk, wk, dk = np.zeros(n), np.zeros(n), np.zeros(n), np.ones(n)
        for rows, tris, c in _triangle_chunks(m, lo, ld):
            ok = c["keep"] & (c["dst"] > EPSILON) & (c["u"] >= 0.0) & (c["v"] >= 0.0) & (c["w"] >= 0.0)   # :280
            t = np.where(ok, c["dst"], np.inf)
            j = t.argmin(1)
            rj = np.arange(rows.size)
            closer = t[rj, j] < tk[rows]
            sel = rows[closer]
            tk[sel] = t[rj, j][closer]
            k[sel] = tris[j[closer]]
            uk[sel], vk[sel], wk[sel], dk[sel] = (c[q][rj, j][closer] for q in ("u", "v", "w", "det"))
        mesh_hit = np.isfinite(tk)
        ln = normalize(m["n1"][k] * wk[:, None] + m["n2"][k] * uk[:, None] + m["n3"][k] * vk[:, None]) * np.sign(dk)[:, None]   # :282
        luv = m["uv1"][k] * wk[:, None] + m["uv2"][k] * uk[:, None] + m["uv3"][k] * vk[:, None]
        lhp = lo + ld * np.where(mesh_hit, tk, 0.0)[:, None]      # :379
        whp = mat_point(m["m2w"], lhp, 1.0)                       # :380
        d = ro - whp
        wdst = np.sqrt(dot(d, d))                                 # :381
        better = mesh_hit & (wdst < best)                         # :383
        best = np.where(better, wdst, best)
        hit |= better
        point = np.where(better[:, None], whp, point)
        normal = np.where(better[:, None], normalize(mat_point(m["m2w"], ln, 0.0)), normal)   # :386
        uv = np.where(better[:, None], luv, uv)
        which = np.where(better, mi, which)
        backface = np.where(better, dk < 0.0, backface)           # :283
    return hit, best, point, normal, uv, which, backface


# ---- when may binary32 legitimately disagree with this file? ------------------------------------------------------------
U32 = 2.0 ** -24     # binary32 unit roundoff
C_LOCAL = 32.0       # local-space budget, in units of U32 * scale (see ambiguity)
C_WORLD = 64.0       # world-distance budget, in units of U32 * (scale + distance) * condition of the transform


def ambiguity(scene, ro, rd):
    """Per ray, how far the float64 decisions of closest_hit are from flipping under binary32 arithmetic: each margin is
    |quantity - threshold| / tolerance, so a margin below 1 means binary32 may legitimately decide the other way.
    Returns a dict of per-ray arrays (+inf where nothing is in reach):

      bary    min |smallest barycentric| of the winning triangle and of every triangle (nearly) hit within reach
      det     min ||det| - 1e-8| of those triangles (the cull threshold, wgsl:268)
      eps     min |dst - EPSILON| of those triangles (wgsl:280)
      gap     relative gap between the best and the second-best world distance over every primitive (nearly) hit,
              two triangles of one mesh included
      disc    min |discriminant| of the spheres (nearly) hit within reach (wgsl:235)
      far     min |far - 0.001| of those spheres (wgsl:239), and of dst_near against 0 (the inside test, wgsl:240)
      ambiguous   any margin < 1
      dst_tol, uv_tol, normal_tol   how far binary32's distance (and hit point), uv and world normal of the winner may
              stray: for a triangle its distance's tolerance below and its barycentrics' tolerance times the change of
              the attribute across the triangle (a small triangle far from the origin has barycentrics good to
              ~ u |ao| / size, and an interpolated normal that turns fast across it carries that into the normal); for a
              sphere its distance's tolerance, carried into the normal by 1 / radius and into uv by the derivatives of
              acos / atan2 (1 at the seam of atan2, where u jumps from 0 to 1)

    The tolerances are first-order bounds of binary32's error, with the scene's coordinate scale S (per mesh and ray: the
    largest |component| of the local origin and of the mesh's vertices) and u = 2^-24:
      * the local ray: lo = W ro + c carries <= 4u (|W| |ro| + |c|) <= 4u S per component, ld = normalize(W rd) <= 6u;
        ao = lo - v1 adds u |ao|, cross(ao, ld) 2u |ao|, a 3-term dot 3u: every numerator of wgsl:266-278 (dot(ao, n),
        dot(eac, dao), dot(eab, dao), all bounded by |e| |ao| or |n| |ao|, |ao| <= 2S) is good to <= 16u S |e| (|n| for the
        distance), doubled for the neglected higher-order terms: C_LOCAL = 32;
      * det = -dot(ld, n): n = cross(eab, eac) is exact up to 3u |n| (edges of binary32 vertices, rounded once), the dot 3u,
        ld 6u: |det| good to 12u |n| (<= C_LOCAL u |n| used);
      * u, v = numerator / det: absolute tolerance (C_LOCAL u S |e| + |u| C_LOCAL u |n|) / |det| -- grazing rays (small |det|)
        get wide margins, as they should; w = (1 - u) - v the sum of both; dst likewise with |n| for |e|;
      * world distances: M lhp + m and the norm add <= 8u (|M| (S + t) + |m|) relative to the condition of the transform:
        tolerance C_WORLD u kappa (S_world + d), S_world = largest |component| of ro and of the world hit point;
      * spheres: b^2 - 4ac is good to 8u (b^2 + |4ac|) (operands first rounded to 2u (|oc|^2 + r^2)), dst_far and dst_near
        to C_LOCAL u (|oc| + r) (plus the square root's share of the discriminant's error, within the disc margin).
    A triangle is "nearly hit" when every test of wgsl:268-280 passes within its tolerance, and it is "within reach" when its
    world distance is at most the best one plus the world tolerance: exactly the triangles whose outcome binary32 may
    decide differently and still compete for the closest hit."""
    n = ro.shape[0]
    inf = np.full(n, np.inf)
    out = {k: inf.copy() for k in ("bary", "det", "eps", "gap", "disc", "far")}
    out["dst_tol"], out["uv_tol"], out["normal_tol"] = np.zeros(n), np.zeros(n), np.zeros(n)
    hit, best, _p, _n, _uv, which, _bf = closest_hit(scene, ro, rd)
    sw = np.maximum(np.abs(ro).max(-1), np.where(hit, np.abs(_p).max(-1), 0.0))
    # every primitive's world distance when (nearly) hit, to find the runner-up: (ray, distance, tolerance)
    cand_r, cand_d, cand_t = [], [], []
    for si in range(scene.sphere_pos.shape[0]):
        oc = ro - scene.sphere_pos[si]
        rr = scene.sphere_radius[si]
        a = dot(rd, rd)
        b = 2.0 * dot(oc, rd)
        c = dot(oc, oc) - rr ** 2
        disc = b * b - 4.0 * a * c
        tol_disc = 8.0 * U32 * (b * b + np.abs(4.0 * a * c)) + 8.0 * U32 * (dot(oc, oc) + rr ** 2) * np.abs(b)
        sq = np.sqrt(np.maximum(disc, 0.0))
        near = (-b - sq) / (2.0 * a)
        far = (-b + sq) / (2.0 * a)
        tol_t = C_LOCAL * U32 * (np.sqrt(dot(oc, oc)) + rr) + np.sqrt(np.maximum(tol_disc, 0.0)) / (2.0 * a)
        nearly = (disc >= -tol_disc) & (far >= 0.001 - tol_t)
        dst = np.where(np.maximum(0.0, near) == 0.0, far, np.maximum(0.0, near))
        tol_w = C_WORLD * U32 * (sw + np.abs(dst))
        reach = nearly & (dst <= best + tol_w)
        out["disc"] = np.where(reach, np.minimum(out["disc"], np.abs(disc) / np.maximum(tol_disc, 1e-300)), out["disc"])
        m_far = np.minimum(np.abs(far - 0.001), np.abs(near)) / tol_t
        out["far"] = np.where(reach, np.minimum(out["far"], m_far), out["far"])
        won = hit & (which == scene.n_meshes + si) & (dst == best)
        if won.any():
            hp = ro[won] + rd[won] * dst[won][:, None]
            nrm = normalize(hp - scene.sphere_pos[si])
            t_n = 2.0 * (tol_t[won] + C_LOCAL * U32 * (np.abs(hp).max(-1) + np.abs(scene.sphere_pos[si]).max())) / rr
            rho = np.sqrt(nrm[:, 0] ** 2 + nrm[:, 2] ** 2)
            seam = (np.abs(nrm[:, 2]) <= t_n) & (nrm[:, 0] > 0.0)
            out["dst_tol"][won] = tol_t[won]
            out["normal_tol"][won] = t_n
            out["uv_tol"][won] = np.where(seam, 1.0, t_n * (1.5 / PI) / np.maximum(rho, 1e-300))
        cand_r.append(np.flatnonzero(reach))
        cand_d.append(dst[reach])
        cand_t.append(tol_w[reach])
    for mi, m in enumerate(scene.meshes):
        lo = mat_point(m["w2m"], ro, 1.0)
        ld = normalize(mat_point(m["w2m"], rd, 0.0))
        a3 = m["m2w"][:3, :3]
        kappa = max(1.0, float(np.linalg.norm(a3, 2) * np.linalg.norm(np.linalg.inv(a3), 2)))
        sv = float(np.abs(np.concatenate([m["v1"], m["v2"], m["v3"]])).max(initial=0.0))
        smax = np.maximum(np.abs(lo).max(-1), sv)
        for rows, _tris, c in _triangle_chunks(m, lo, ld):
            S = smax[rows][:, None]
            e = np.maximum(c["eab_len"], c["eac_len"])
            adet = np.maximum(np.abs(c["det"]), 1e-300)
            tol_det = np.broadcast_to(C_LOCAL * U32 * c["nrm_len"], c["det"].shape)
            tol_b = (C_LOCAL * U32 * S * e + C_LOCAL * U32 * c["nrm_len"]) / adet
            tol_d = (C_LOCAL * U32 * S * c["nrm_len"] + np.abs(c["dst"]) * C_LOCAL * U32 * c["nrm_len"]) / adet
            det_ok = (np.abs(c["det"]) if m["glass"] else c["det"]) >= 1e-8 - tol_det
            bmin = np.minimum(np.minimum(c["u"], c["v"]), c["w"])
            with np.errstate(invalid="ignore"):
                nearly = det_ok & (bmin >= -2.0 * tol_b) & (c["dst"] > EPSILON - tol_d) & np.isfinite(c["dst"])
            if not nearly.any():
                continue
            ri, ti = np.nonzero(nearly)
            rows_i = rows[ri]
            t = c["dst"][ri, ti]
            lhp = lo[rows_i] + ld[rows_i] * t[:, None]
            whp = mat_point(m["m2w"], lhp, 1.0)
            wd = np.sqrt(dot(ro[rows_i] - whp, ro[rows_i] - whp))
            tol_w = C_WORLD * U32 * kappa * (sw[rows_i] + wd) + kappa * tol_d[ri, ti]
            reach = wd <= best[rows_i] + tol_w
            ri, ti, rows_i, wd, tol_w = ri[reach], ti[reach], rows_i[reach], wd[reach], tol_w[reach]
            won = (which[rows_i] == mi) & (wd == best[rows_i])   # the winning triangle (closest_hit's arithmetic)
            if won.any():
                wr, wt, tb = rows_i[won], _tris[ti[won]], 2.0 * tol_b[ri[won], ti[won]]
                du = np.abs(m["uv2"][wt] - m["uv1"][wt]).max(-1) + np.abs(m["uv3"][wt] - m["uv1"][wt]).max(-1)
                n1, n2, n3 = m["n1"][wt], m["n2"][wt], m["n3"][wt]
                uu, vv = c["u"][ri[won], ti[won]], c["v"][ri[won], ti[won]]
                ni = np.sqrt(dot(*(2 * [n1 * (1.0 - uu - vv)[:, None] + n2 * uu[:, None] + n3 * vv[:, None]])))
                dn = (np.sqrt(dot(n2 - n1, n2 - n1)) + np.sqrt(dot(n3 - n1, n3 - n1))) / np.maximum(ni, 1e-300)
                out["dst_tol"][wr] = tol_w[won]
                out["uv_tol"][wr] = tb * du
                out["normal_tol"][wr] = tb * dn * kappa
            mb = np.abs(bmin[ri, ti]) / (2.0 * tol_b[ri, ti])
            ad = np.abs(np.abs(c["det"][ri, ti]) if m["glass"] else c["det"][ri, ti])
            md = np.abs(ad - 1e-8) / tol_det[ri, ti]
            me = np.abs(c["dst"][ri, ti] - EPSILON) / tol_d[ri, ti]
            np.minimum.at(out["bary"], rows_i, mb)
            np.minimum.at(out["det"], rows_i, md)
            np.minimum.at(out["eps"], rows_i, me)
            cand_r.append(rows_i)
            cand_d.append(wd)
            cand_t.append(tol_w)
    if cand_r:
        r = np.concatenate(cand_r)
        d = np.concatenate(cand_d)
        tw = np.concatenate(cand_t)
        order = np.lexsort((d, r))
        r, d, tw = r[order], d[order], tw[order]
        first = np.r_[True, r[1:] != r[:-1]]
        second = np.r_[False, ~first[1:]] & np.r_[False, first[:-1]]   # the runner-up of each ray
        idx2 = np.flatnonzero(second)
        out["gap"][r[idx2]] = (d[idx2] - d[idx2 - 1]) / (tw[idx2] + tw[idx2 - 1])
    out["ambiguous"] = np.zeros(n, bool)
    for k in ("bary", "det", "eps", "gap", "disc", "far"):
        out["ambiguous"] |= out[k] < 1.0
    return out


def primary_rays(scene, W, H, rng=None):
    """frag :473-495 for every pixel (x fastest); with rng: the four jitter draws per sample."""
    y, x = np.mgrid[0:H, 0:W]
    px = np.stack([x.reshape(-1), y.reshape(-1)], -1).astype(np.float64)
    uv = px / (np.array([W, H], np.float64) - 1.0)                          # :479
    c2w = scene.cam_to_world
    origin = np.broadcast_to(c2w[3, :3], (W * H, 3)).copy()
    local = np.concatenate([uv - 0.5, np.ones((W * H, 1))], -1) * scene.view_params   # :481
    focus = mat_point(c2w, local, 1.0)                                       # :482
    if rng is not None:
        right, up = c2w[0, :3], c2w[1, :3]
        jx, jy = rng.in_unit_disk()                                          # :488
        origin = origin + right * (jx * scene.defocus / W)[:, None] + up * (jy * scene.defocus / W)[:, None]
        kx, ky = rng.in_unit_disk()                                          # :492
        focus = focus + right * (kx * scene.diverge / W)[:, None] + up * (ky * scene.diverge / W)[:, None]
    return origin, normalize(focus - origin)                                 # :494


# ---- one segment behind the intersection: trace :405-468 for given hits ------------------------------------------------------
F32_MAX = float(np.finfo(np.float32).max)
PIN_TOL = 1e-5       # the comparison tolerance the ill-conditioning bounds are measured against (tests/test_f64_pin.py)


def r32(x):
    """x with binary32's RANGE: what overflows there is infinite here too (a double holds 2^129 and 1 / 1e-40; the shader's
    numbers do not, and inf * 0 or inf - inf further on are NaN for it).  The precision stays the double's."""
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(x) > F32_MAX, np.copysign(np.inf, x), x)


def _len(v):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt(r32(dot(v, v)))


def _unit(v, err_v, ops):
    """normalize(v) and a bound of binary32's error of it, as a fraction of the unit length: v itself is off by err_v (absolute,
    propagated from its operands) plus `ops` roundings of at most 2^-24 |v|_max each on the way to it, and dividing by the
    length |v| turns an absolute error e into e / |v| -- (err_v + ops * 2^-24 * |v|_max) / |v| + 3 * 2^-24 for the dot, the
    square root and the scaling.  A short sum of long operands (|v| << |v|_max is impossible, but |v| << its operands is
    what mix() of two opposite directions gives: the caller passes the operands' size in err_v) is what this catches."""
    ln = _len(v)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        u = v / ln[..., None]
        err = (err_v + ops * U32 * np.abs(v).max(-1)) / ln + 3.0 * U32
    return u, np.where(np.isfinite(err), err, 0.0)   # (a zero or non-finite v: NaN on both sides, nothing to bound)


def wsign(x):
    """WGSL sign() with the one choice it leaves open made as both comparisons failing make it: sign(NaN) = 0."""
    with np.errstate(invalid="ignore"):
        return np.where(x > 0.0, 1.0, np.where(x < 0.0, -1.0, 0.0))


def _sphere(rng, mask):
    """rand_unit_sphere :168-174 (three rand_normal_dist :181-185, then normalize) for the states under `mask`, and E_s: the
    bound of binary32's error of the result per unit length (scatter's docstring).  Per component x = rho cos(theta): theta
    carries 6e-7 (10u) and cos_ 2u, so rho 12u; rho = sqrt(-2 log r) carries delta(rho^2) = 2 delta(r) / r = 2u, that is
    2u / (2 rho) -- and never more than sqrt(2u), reached at rho = 0 (r rounds to 1.0 in binary32 and not here)."""
    comps, errs = [], []
    for _ in range(3):
        theta = 2.0 * PI * rng.rand(mask)
        with np.errstate(divide="ignore", invalid="ignore"):
            rho = np.sqrt(-2.0 * np.log(rng.rand(mask)))
            comps.append(rho * np.cos(theta))
            errs.append(12.0 * U32 * rho + np.minimum(U32 / rho, np.sqrt(2.0 * U32)))
    xyz = np.stack(comps, -1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ln = np.sqrt(dot(xyz, xyz))
        e = np.sqrt(sum(x * x for x in errs)) / ln + 3.0 * U32
        unit = xyz / ln[:, None]
    return unit, np.where(np.isfinite(e), e, 0.0)


def scatter(scene, cases, skybox=1):
    """trace :405-468 for given hits: the sky on a miss (:406-411), glass (:414-436), everything else (:437-460) and the russian
    roulette with its rescale (:462-466), on arrays of n cases.  cases: dict of rd (n, 3), T (n, 4), light (n, 4), rng (n u32
    states), hit (n bool), dst (n), point (n, 3), normal (n, 3), uv (n, 2), backface (n bool), which (n material indices: mesh
    materials first, then the spheres'), and optionally ro (n, 3; default zero).  Returns dict of ro, rd, T, light, rng (the
    states afterwards), goes_on (n bool: hit and survived the roulette) and ambiguous (n bool).

    ambiguous: binary32 may legitimately decide or land elsewhere.  Every decision has a margin |quantity - threshold| and a
    tolerance, a first-order bound of binary32's error of the quantity with u = 2^-24; a case is ambiguous when a margin is
    below its tolerance:
      specular >= r, r >= p   r = f32(bits) * 2^-32 there against bits / (2^32 - 1) here: u r + 2^-32 apart, doubled; p is a
                              product of two or three binary32 factors (absorption: an exp_ as well, a texture: the bilinear
                              filter's 12 operations): 16 u |p|
      reflectance > r         cos_theta is a 3-term dot of unit vectors (3u), (1 - cos)^5 carries 5 x 4u (1 - cos)^4 <= 20u and
                              the pow_ polynomial a few u more; r0 a reciprocal, a quotient and a square (8u max(1, r0)); the sum
                              and the product 3u: under 40u max(1, reflectance), 64u used
      ior * sin > 1           1 - cos^2 is good to 8u (absolute), so sin = sqrt(.) to 4u / sin, and to sqrt(8u) where sin^2 < 8u;
                              the product adds 4u |ior sin|
      k < 0                   k = 1 - eta^2 (1 - d^2): d is a 3-term dot of unit vectors (3u absolute), so d^2 carries 6u |d| and
                              1 - d^2 another u; eta^2 2u of itself (eta may be a rounded reciprocal) and the product u: eta^2
                              (6 |d| + 2 + 3 (1 - d^2)) u, and the last difference u |k|
      the hemisphere flip     sign(dot(n, s)) of the unit-sphere sample s: its angle theta = 2 pi r is off by up to 3 roundings of
                              2 pi 2^-25 (r, the product, the constant) = 6e-7 and cos_ by 2u, so a component of the unnormalised
                              (x, y, z) by rho (10u + 2u) and, through log near r = 1, u / rho (_sphere): E_s per unit length;
                              tolerance 2 E_s |n|
      the origin offset       sign(dot(n, rd')) of the new direction: 4u |n| + 2 |n| (rd's bound below)
    and when an OUTPUT is ill-conditioned: a normalised vector whose bound from _unit (operation count x 2^-24 / length, plus
    what its operands carry) exceeds the comparison tolerance PIN_TOL, or a light sum that cancels: light + emitted * T with
    the product rounded twice and the sum once is off by u (2 |product| + |sum|), more than PIN_TOL max(|sum|, 1e-3)."""
    n = cases["rd"].shape[0]
    f = lambda k: np.array(cases[k], np.float64)  # noqa: E731
    rd, T, light = f("rd"), f("T"), f("light")
    ro = f("ro") if "ro" in cases else np.zeros((n, 3))
    hit = np.asarray(cases["hit"], bool)
    rng = Rng(np.asarray(cases["rng"]))
    amb = np.zeros(n, bool)
    goes_on = np.zeros(n, bool)
    miss = ~hit
    if skybox and miss.any():                               # :406-411
        env = environment_light(rd[miss])
        new_light = r32(light[miss] + r32(T[miss] * env))
        # the sun is pow(m, 500) of a 3-term dot m (3u, and the pow_ polynomial's own few u on a logarithm that is multiplied
        # by 500): good to 500 x 4u of itself -- 1e-4 where the ray looks into it; the rest of the sky to 16u
        with np.errstate(invalid="ignore", over="ignore"):
            sun = np.power(np.maximum(0.0, dot(rd[miss], np.array([0.1, 1.0, 0.1]))), 500.0) * 0.1
            e = np.abs(T[miss]) * (2000.0 * U32 * sun + 16.0 * U32 * np.abs(env).max(-1))[:, None] + U32 * np.abs(new_light)
            amb[miss] |= (np.isfinite(e) & (e > PIN_TOL * np.maximum(np.abs(new_light), 1e-3))).any(-1)
        light[miss] = new_light
    if not hit.any():
        return dict(ro=ro, rd=rd, T=T, light=light, rng=rng.s.astype(np.uint32), goes_on=goes_on, ambiguous=amb)
    wm = np.asarray(cases["which"], np.int64)
    nrm, dsth, bf, uvm, point = f("normal"), f("dst"), np.asarray(cases["backface"], bool), f("uv"), f("point")
    ro = np.where(hit[:, None], point, ro)                  # :413
    nlen = np.sqrt(dot(nrm, nrm))
    glass = hit & (scene.mat_flag[wm] == 1)
    err_rd = np.zeros(n)
    p_tol = np.zeros(n)
    tex_err = np.zeros(n)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        # ---- glass :414-436 ----
        g = np.nonzero(glass)[0]
        if g.size:
            mi = wm[g]
            e = r32(r32(-dsth[g][:, None] * scene.mat_absorption[mi][:, :3]) * scene.mat_absorption_strength[mi][:, None])
            Tg_in = np.concatenate([r32(T[g][:, :3] * np.exp(e)), np.ones((g.size, 1))], -1)
            T[g] = np.where(bf[g][:, None], Tg_in, T[g])                                # :415-418
            p_tol[g] = np.where(bf[g], 16.0, 2.0)
            ior = np.where(bf[g], scene.mat_ior[mi], r32(1.0 / scene.mat_ior[mi]))      # :420
            d_in, ng = rd[g], nrm[g]
            refl = d_in - 2.0 * dot(ng, d_in)[:, None] * ng                             # :422
            dd = dot(ng, d_in)                                                          # refract :423 (WGSL builtin)
            eta2 = r32(ior * ior)
            k = 1.0 - r32(eta2 * (1.0 - dd * dd))
            refr = r32(ior[:, None] * d_in) - r32(r32(ior * dd) + np.sqrt(np.maximum(k, 0.0)))[:, None] * ng
            refr = np.where((k < 0.0)[:, None], 0.0, refr)
            tol_k = U32 * (np.abs(eta2) * (6.0 * np.abs(dd) + 2.0 + 3.0 * np.abs(1.0 - dd * dd)) + np.abs(k))
            tol_k = np.where(np.isfinite(tol_k), tol_k, 0.0)
            amb[g] |= np.isfinite(k) & (np.abs(k) < tol_k)
            err_refr = np.where(np.isfinite(k) & (k > 0.0), tol_k / (2.0 * np.sqrt(np.maximum(k, tol_k))), 0.0) + 8.0 * U32 * (1.0 + np.abs(ior))
            err_refr = np.where(np.isfinite(err_refr), err_refr, 0.0)
            cos_t = np.minimum(dot(-d_in, ng), 1.0)
            s2 = 1.0 - cos_t * cos_t
            sin_t = np.sqrt(s2)
            cannot = r32(ior * sin_t) > 1.0
            sin_safe = np.sqrt(np.maximum(s2, 0.0))
            tol_sin = 4.0 * U32 / np.maximum(sin_safe, np.sqrt(8.0 * U32))
            q = r32(ior * sin_safe)
            amb[g] |= np.isfinite(q) & (np.abs(q - 1.0) < np.abs(ior) * tol_sin + 4.0 * U32 * np.abs(q))
            r0 = r32(r32((1.0 - ior) / (1.0 + ior)) ** 2)
            schlick = r0 + r32((1.0 - r0) * np.power(1.0 - cos_t, 5.0))                  # :208-212
            draw = np.zeros(n, bool)
            draw[g[~cannot]] = True                                                     # `||` short-circuits: no draw when cannot_refract (:428)
            rr = rng.rand(draw)[g]
            follow = cannot | (schlick > rr)
            amb[g] |= ~cannot & np.isfinite(schlick) & (np.abs(schlick - rr) < 64.0 * U32 * np.maximum(1.0, np.abs(schlick)))
            gm = np.zeros(n, bool)
            gm[g] = True
            sph, e_s = _sphere(rng, gm)                                                 # :430 (rand_direction :187-193)
            sph, e_s = sph[g], e_s[g]
            diffuse, e_d = _unit(ng + sph, e_s, 1.0)
            spec, smooth = scene.mat_specular[mi], scene.mat_smoothness[mi]
            e_in = np.abs(1.0 - spec) * e_d + np.abs(spec) * 8.0 * U32 * (1.0 + nlen[g] ** 2) + 3.0 * U32 * (np.abs(1.0 - spec) + np.abs(spec))
            refl, e_refl = _unit(mix(diffuse, refl, spec[:, None]), np.where(np.isfinite(e_in), e_in, 0.0), 0.0)       # :432
            e_in = np.abs(1.0 - smooth) * e_d + np.abs(smooth) * err_refr + 3.0 * U32 * (np.abs(1.0 - smooth) + np.abs(smooth))
            refr, e_refr = _unit(mix(-diffuse, refr, smooth[:, None]), np.where(np.isfinite(e_in), e_in, 0.0), 0.0)    # :433
            nd = np.where(follow[:, None], refl, refr)
            err_rd[g] = np.where(follow, e_refl, e_refr)
            rd[g] = nd
            sg = dot(ng, nd)
            amb[g] |= np.isfinite(sg) & (np.abs(sg) < nlen[g] * (4.0 * U32 + 2.0 * err_rd[g]))
            ro[g] = point[g] + 1e-4 * ng * wsign(sg)[:, None]                         # :436
        # ---- everything else :437-460 ----
        o = np.nonzero(hit & ~glass)[0]
        if o.size:
            om = np.zeros(n, bool)
            om[o] = True
            mi = wm[o]
            r1 = rng.rand(om)[o]
            spc = scene.mat_specular[mi]
            is_spec = spc >= r1                                                          # :438
            amb[o] |= np.isfinite(spc) & (np.abs(spc - r1) < 2.0 * (U32 * np.maximum(r1, np.abs(spc)) + 2.0 ** -32))
            sph, e_s = _sphere(rng, om)                                                 # :448 (rand_hemisphere :176-179)
            sph, e_s = sph[o], e_s[o]
            no = nrm[o]
            sd = dot(no, sph)
            amb[o] |= np.isfinite(sd) & (np.abs(sd) < 2.0 * e_s * nlen[o])
            diffuse = sph * wsign(sd)[:, None]
            specular_dir = rd[o] - 2.0 * dot(no, rd[o])[:, None] * no                    # reflect :449
            emitted = r32(scene.mat_emission_color[mi] * scene.mat_emission_strength[mi][:, None])
            add = r32(emitted * T[o])
            new_light = r32(light[o] + add)                                              # :452
            amb[o] |= (U32 * (2.0 * np.abs(add) + np.abs(new_light)) > PIN_TOL * np.maximum(np.abs(new_light), 1e-3)).any(-1)
            light[o] = new_light
            t = scene.mat_smoothness[mi] * is_spec
            e_in = np.abs(1.0 - t) * e_s + np.abs(t) * 8.0 * U32 * (1.0 + nlen[o] ** 2) + 3.0 * U32 * (np.abs(1.0 - t) + np.abs(t))
            rd[o], err_rd[o] = _unit(mix(diffuse, specular_dir, t[:, None]), np.where(np.isfinite(e_in), e_in, 0.0), 0.0)   # :451
            col = scene.mat_color[mi].copy()
            tex = (scene.mat_flag[mi] == 2) & (scene.mat_diffuse_index[mi] != -1)          # :454
            p_tol[o] = np.where(tex & ~is_spec, 16.0, 2.0)
            for ti in np.unique(scene.mat_diffuse_index[mi][tex]):
                sel = tex & (scene.mat_diffuse_index[mi] == ti)
                if 0 <= int(ti) < len(scene.textures):
                    tex_ = scene.textures[int(ti)]
                    uu, vv = uvm[o][sel, 0], uvm[o][sel, 1]
                    col[sel] = sample_texture(tex_, uu, vv)                                                    # :455
                    # the sample position u * width - 0.5 is rounded twice (2u of itself, du in u) and the filter's weights
                    # move with it: the colour by what the (piecewise linear) filter gives du and dv away, on either side,
                    # plus the filter's 12 operations on the colour itself
                    du = 2.0 * U32 * (np.abs(uu) + 1.0 / tex_.shape[1])
                    dv = 2.0 * U32 * (np.abs(vv) + 1.0 / tex_.shape[0])
                    moved = [np.abs(sample_texture(tex_, uu + a * du, vv + b * dv) - col[sel]) for a, b in ((1, 0), (-1, 0), (0, 1), (0, -1))]
                    e_c = np.maximum(moved[0], moved[1]) + np.maximum(moved[2], moved[3]) + 12.0 * U32 * np.abs(col[sel])
                    e_c = np.where((np.abs(uu * tex_.shape[1]) + np.abs(vv * tex_.shape[0]) < 2.0 ** 22)[:, None], e_c, 1.0)   # (no fraction left)
                    e_t = np.where(np.isfinite(e_c), e_c, 0.0) * np.abs(T[o][sel]) * ~is_spec[sel][:, None]
                    tex_err[o[sel]] = e_t[:, :3].max(-1)
                    amb[o[sel]] |= (e_t > PIN_TOL * np.maximum(np.abs(T[o][sel] * col[sel]), 1e-3)).any(-1)
                else:
                    col[sel] = 0.0   # (the reference binds 1 x 1 zero textures to the unused slots)
            T[o] = r32(T[o] * np.where(is_spec[:, None], scene.mat_specular_color[mi], col))                   # :459
        amb |= hit & (err_rd > PIN_TOL)
        h = np.nonzero(hit)[0]
        p = np.fmax.reduce(T[h, :3], -1)                    # :462 (max() of WGSL returns the other operand for a NaN)
        r2 = rng.rand(hit)[h]
        die = r2 >= p                                       # :463
        amb[h] |= np.isfinite(p) & (np.abs(r2 - p) < 2.0 * (U32 * r2 + 2.0 ** -32) + p_tol[h] * U32 * np.abs(p) + tex_err[h])
        live = h[~die]
        goes_on[live] = True
        T[live] = r32(T[live] * r32(1.0 / p[~die])[:, None])   # :466
    return dict(ro=ro, rd=rd, T=T, light=light, rng=rng.s.astype(np.uint32), goes_on=goes_on, ambiguous=amb)


def render_frame(scene, W, H, bounces, spp, frames, skybox=1):
    """`frag` :473-500 + `trace` :398-471 for one frame: the per-frame sample image (H, W, 4) in float64."""
    y, x = np.mgrid[0:H, 0:W]
    seed = (y.reshape(-1).astype(np.float64) * W + x.reshape(-1)).astype(np.uint64) + np.uint64(abs(frames)) * np.uint64(719393)   # :475
    rng = Rng(seed & np.uint64(0xffffffff))
    n = W * H
    total = np.zeros((n, 4))
    for _ in range(spp):
        ro, rd = primary_rays(scene, W, H, rng)
        rd = normalize(rd)                                  # :400
        T = np.ones((n, 4))
        light = np.zeros((n, 4))
        alive = np.ones(n, bool)
        for _seg in range(bounces + 1):                     # :404
            if not alive.any():
                break
            idx = np.nonzero(alive)[0]
            hit, dst, point, normal, uvh, which, backface = closest_hit(scene, ro[idx], rd[idx])
            s = scatter(scene, dict(ro=ro[idx], rd=rd[idx], T=T[idx], light=light[idx], rng=rng.s[idx], hit=hit, dst=dst, point=point,
                                    normal=normal, uv=uvh, backface=backface, which=which), skybox)
            ro[idx], rd[idx], T[idx], light[idx] = s["ro"], s["rd"], s["T"], s["light"]
            rng.s[idx] = s["rng"].astype(np.uint64)
            alive[idx] = s["goes_on"]
        total += light                                      # :496
    return (total / spp).reshape(H, W, 4)                   # :498


def debug_view(scene, W, H, mode, scale):
    """debug_trace :502-573 for the views that do not count BVH tests: 1 normals, 2 depth, 3 texcoords, 4 focus distance."""
    ro, rd = primary_rays(scene, W, H)
    hit, dst, _point, normal, uv, _which, _bf = closest_hit(scene, ro, rd)
    out = np.zeros((W * H, 4))
    if mode == 1:
        out[hit] = np.concatenate([normal[hit] * 0.5 + 0.5, np.ones((hit.sum(), 1))], -1)
    elif mode == 2:
        d = dst[hit] / float(scale)
        out[hit] = np.stack([d, d, d, np.ones_like(d)], -1)
    elif mode == 3:
        out[hit] = np.concatenate([uv[hit], np.zeros((hit.sum(), 1)), np.ones((hit.sum(), 1))], -1)
    elif mode == 4:
        s, d = float(scale) / 100.0, dst[hit]
        out[hit] = np.where((d > s)[:, None], np.array([0.0, 1.0, 0.0, 1.0]), np.stack([d, d, d, np.ones_like(d)], -1))
    else:
        raise ValueError("views 5-7 count BVH tests: this restatement has no BVH")
    return out.reshape(H, W, 4), hit.reshape(H, W)
