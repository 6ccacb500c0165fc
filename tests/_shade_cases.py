"""Seeded lane states, hits and material palettes for the per-hit shading tests (tests/test_shade_oracle_f64.py on the CPU,
tests/test_gpu_shade.py on the device).

A render hands path_end the hits its own rays find on a handful of comfortable materials.  The families below aim at the
places where a kernel and a literal restatement of wgsl:405-468 can part ways and images almost never look: the critical
angle from both of its tests, a cosine that rounds past +-1, RNG draws of exactly 0.0 and 1.0 at every decision, roulette
probabilities of 0, 1, subnormal, 2^120 and beyond, NaN and negative throughput, glass with ior 1, below 1, 0, infinite and
NaN, absorption over 2^127, texture coordinates far outside [0, 1) and non-finite, and every boundary of the end-of-sample
bookkeeping.  Everything is deterministic (seeded).

A case is the (32,) u32 record of include/rt_test_abi.h (rt_test_shade); a family is a list of batches
dict(cases=(n, 32) u32, nb=number_of_bounces, rpp=rays_per_pixel, skybox=0 / 1) -- the three are arguments of a probe call.
"""
import numpy as np

import _ray_families as RF
from ray_tracer_2_amd import _abi as A
from ray_tracer_2_amd.ray_tracer import normalize3_f32
from _rng_edge import A_LCG, C_LCG, edge_states
from oracle import independent_f64 as F

F32 = np.float32
STEP_END, STEP_TRAVERSE = 0, 3
NAN, INF = float("nan"), float("inf")
SUB = 1e-40                       # a binary32 subnormal
UP1, DOWN1 = float(np.nextafter(F32(1), F32(2))), float(np.nextafter(F32(1), F32(0)))
# words of a case / of a record (include/rt_test_abi.h)
C_RD, C_T, C_LIGHT, C_TOTAL, C_RNG, C_SEG, C_J, C_MODE, C_HIT, C_DST, C_POINT, C_NORMAL, C_U, C_V, C_BACK, C_OBJ, C_META = \
    0, 3, 7, 11, 15, 16, 17, 18, 19, 20, 21, 24, 27, 28, 29, 30, 31
R_RO, R_RD, R_T, R_LIGHT, R_TOTAL, R_RNG, R_SEG, R_J, R_FRESH, R_RET, R_NSEG, R_META, R_INST, R_DEAD = \
    0, 3, 6, 10, 14, 18, 19, 20, 21, 22, 23, 24, 25, 26
INST_TLAS, INST_SIMPLE, INST_NO_FAST_MISS, INST_LDS, INST_TOTAL_LDS = 1, 2, 32, 64, 128


# ---- palettes -----------------------------------------------------------------------------------------------------------
def mat(flag=A.MATERIAL_DEFAULT, color=(0.7, 0.6, 0.5, 1.0), spec_color=(0.9, 0.9, 0.9, 1.0), emission=(0, 0, 0, 0), emission_s=0.0,
        specular=0.5, smoothness=0.5, ior=1.5, absorption=(0, 0, 0, 0), absorption_s=0.0, diffuse_index=-1):
    m = np.zeros((), A.MATERIAL_DTYPE)
    m["color"], m["specular_color"], m["emission_color"], m["absorption"] = color, spec_color, emission, absorption
    m["emission_strength"], m["absorption_strength"] = emission_s, absorption_s
    m["specular"], m["smoothness"], m["ior"], m["flag"] = specular, smoothness, ior, flag
    m["diffuse_index"], m["normal_index"] = diffuse_index, -1
    return m


H = 2.0 ** 121
PLAIN = [   # (name, material): colours / specular colours at 0, 1, > 1, subnormal, 2^121, a NaN channel, negative; emission
            # strength 0 with a huge colour and the reverse; specular and smoothness in {0, 0.5, 1, -0.25, 1.5}
    ("mid", mat()),
    ("zero", mat(color=(0, 0, 0, 1), spec_color=(0, 0, 0, 1), specular=0.0, smoothness=0.0)),
    ("one", mat(color=(1, 1, 1, 1), spec_color=(1, 1, 1, 1), specular=1.0, smoothness=1.0)),
    ("above_one", mat(color=(1.5, 2.0, 0.5, 1), spec_color=(3, 3, 3, 1), specular=0.5, smoothness=1.5)),
    ("subnormal", mat(color=(SUB, SUB / 2, 0, 1), spec_color=(0, SUB, 0, 1), specular=0.5, smoothness=0.0)),
    ("huge", mat(color=(H, 1, 0.5, 1), spec_color=(0.5, H, H, 1), specular=-0.25, smoothness=0.5)),
    ("nan_x", mat(color=(NAN, 0.5, 0.25, 1), spec_color=(0.5, NAN, 0.8, 1), specular=0.5, smoothness=-0.25)),
    ("nan_z", mat(color=(0.3, 0.6, NAN, 1), spec_color=(0.2, 0.4, NAN, 1), specular=1.5, smoothness=1.0)),
    ("nan_all", mat(color=(NAN, NAN, NAN, NAN), spec_color=(0.5, 0.5, 0.5, 1), specular=0.5, smoothness=0.5)),
    ("negative", mat(color=(-0.5, 0.5, -1.0, 1), spec_color=(-1, -1, -1, 1), specular=0.5, smoothness=0.5)),
    ("dark_lamp", mat(emission=(H, H, H, 1), emission_s=0.0)),
    ("zero_lamp", mat(emission=(0, 0, 0, 0), emission_s=H, color=(0.9, 0.9, 0.9, 1))),
    ("lamp", mat(emission=(1.0, 0.9, -0.8, 1), emission_s=5.0, color=(0.2, 0.2, 0.2, 1), specular=0.0, smoothness=1.0)),
    ("below_one", mat(color=(DOWN1, 0.5, 0.5, 1), spec_color=(1, 0.5, 0.25, 1), specular=0.0, smoothness=1.0)),
    ("mirror_half", mat(color=(0.5, 0.5, 0.5, 1), spec_color=(1, 0.5, 0.25, 1), specular=1.0, smoothness=0.5)),
]
IORS = [("1", 1.0), ("1+", UP1), ("1-", DOWN1), ("1.5", 1.5), ("0.5", 0.5), ("0", 0.0), ("-1.5", -1.5), ("inf", INF), ("nan", NAN),
        ("sub", SUB)]
GLASS_SETTINGS = [("clear", dict(specular=1.0, smoothness=1.0)),
                  ("frosted", dict(specular=0.5, smoothness=0.5, absorption=(0.2, 0.5, 1.0, 0), absorption_s=2.0)),
                  ("matte", dict(specular=0.0, smoothness=0.0, absorption=(0.0, 1e30, -1.0, 0), absorption_s=1e20))]
GLASS_EXTRA = [("1.5_inf_absorb", dict(ior=1.5, specular=1.0, smoothness=1.0, absorption=(0.0, 1.0, 0.5, 0), absorption_s=INF)),
               ("1.5_nan_absorb", dict(ior=1.5, specular=1.0, smoothness=0.5, absorption=(NAN, 0.1, 0.0, 0), absorption_s=1.0)),
               ("1.5_outside", dict(ior=1.5, specular=1.5, smoothness=-0.25)),
               ("0.5_outside", dict(ior=0.5, specular=-0.25, smoothness=1.5))]
TEXTURED = [("tex_none", dict(diffuse_index=-1)), ("tex_1x1", dict(diffuse_index=0)), ("tex_5x3", dict(diffuse_index=1, specular=0.0)),
            ("tex_dummy", dict(diffuse_index=2)), ("tex_last", dict(diffuse_index=63, specular=0.25))]


def general_spheres():
    out = [(f"glass_{n}_{s}", mat(A.MATERIAL_GLASS, ior=ior, **kw)) for n, ior in IORS for s, kw in GLASS_SETTINGS]
    out += [(f"glass_{n}", mat(A.MATERIAL_GLASS, **kw)) for n, kw in GLASS_EXTRA]
    out += [(n, mat(A.MATERIAL_TEXTURE, **kw)) for n, kw in TEXTURED]
    return out


def textures():
    rng = np.random.default_rng(53)
    return [np.array([[[200, 100, 50, 255]]], np.uint8), rng.integers(0, 256, (3, 5, 4), dtype=np.uint8)]


_SCENES = {}


def palette(name):
    """(SceneArrays, material names in object-index order) of the "plain" or the "general" palette.  plain: one small quad
    per material, each under a transform of its own (15 meshes: no top-level tree, no root culling -- a few-mesh scene, so
    the SIMPLE and the scene-in-LDS kernels apply).  general: the same quads under ONE transform (a run of 15: the top-level
    tree, unless option tlas = 0) and a sphere per glass / texture material."""
    if name not in _SCENES:
        meshes = []
        for i, (_n, m) in enumerate(PLAIN):
            c = (0.5 * (i % 4) - 1.0, 0.5 * (i // 4) - 1.0, 0.0)
            q = RF.quad((0, 0, 0) if name == "plain" else c, (0.2, 0, 0), (0, 0.2, 0))
            # (a root with two leaves in the general palette: root leaves are not gathered under a top-level tree)
            meshes.append(dict(tris=q, bvh=("rootleaf",) if name == "plain" else ("median", 1), m2w=RF.trs(pos=c) if name == "plain" else None, mat=m))
        spheres = [] if name == "plain" else [((0.3 * (i % 8) - 1.0, 0.3 * (i // 8) - 1.0, 2.0), 0.1, m) for i, (_n, m) in enumerate(general_spheres())]
        arrays = RF.make_arrays(meshes, spheres)
        if name == "general":
            arrays.textures = [np.ascontiguousarray(t) for t in textures()]
        _SCENES[name] = (arrays, [n for n, _ in PLAIN] + ([] if name == "plain" else [n for n, _ in general_spheres()]))
    return _SCENES[name]


def materials_of(arrays):
    return [m["material"] for m in arrays.meshes] + [s["material"] for s in arrays.spheres]


# ---- records ------------------------------------------------------------------------------------------------------------
def bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def make(n, **k):
    """(n, 32) u32 case records from broadcastable fields; defaults: a front-face hit of object 0 at the origin, normal +y,
    straight incidence, T = 1, no light, total 0, RNG state 1, seg 0, j 0, STEP_TRAVERSE, meta 0."""
    d = dict(rd=(0, -1, 0), T=(1, 1, 1, 1), light=(0, 0, 0, 0), total=(0, 0, 0, 0), rng=1, seg=0, j=0, mode=STEP_TRAVERSE, hit=1,
             dst=1.0, point=(0, 0, 0), normal=(0, 1, 0), u=0.25, v=0.75, backface=0, obj=0, meta=0)
    assert not set(k) - set(d), set(k) - set(d)
    d.update(k)
    c = np.zeros((n, 32), np.uint32)
    for key, w, m in (("rd", C_RD, 3), ("T", C_T, 4), ("light", C_LIGHT, 4), ("total", C_TOTAL, 4), ("point", C_POINT, 3), ("normal", C_NORMAL, 3)):
        c[:, w:w + m] = bits(np.broadcast_to(np.asarray(d[key], F32), (n, m)))
    for key, w in (("dst", C_DST), ("u", C_U), ("v", C_V)):
        c[:, w] = bits(np.broadcast_to(np.asarray(d[key], F32), (n,)))
    for key, w in (("rng", C_RNG), ("mode", C_MODE), ("hit", C_HIT), ("backface", C_BACK), ("obj", C_OBJ), ("meta", C_META)):
        c[:, w] = np.broadcast_to(np.asarray(d[key], np.int64), (n,)).astype(np.uint32)
    for key, w in (("seg", C_SEG), ("j", C_J)):
        c[:, w] = np.broadcast_to(np.asarray(d[key], np.int64), (n,)).astype(np.int32).view(np.uint32)
    return c


def cross(*parts):
    """Every combination of the rows of the given (n_i, 32) records: a later part's NON-DEFAULT words overwrite (parts are
    made with `make`, whose defaults mark the words a part does not set)."""
    base = make(1)[0]
    out = parts[0]
    for p in parts[1:]:
        a = np.repeat(out, len(p), 0)
        b = np.tile(p, (len(out), 1))
        setw = (p != base[None, :]).any(0)
        a[:, setw] = b[:, setw]
        out = a
    return out


def unit(rng, n):
    return normalize3_f32(rng.normal(size=(n, 3)))


def facing(rng, n, positive):
    """Unit normals and unit directions with dot(rd, n) < 0, and > 0 where `positive`."""
    nrm, rd = unit(rng, n), unit(rng, n)
    d = (nrm.astype(np.float64) * rd).sum(-1)
    flip = (d > 0) != (np.asarray(positive) != 0)
    rd[flip] = -rd[flip]
    return nrm, rd


def step_back(states, k):
    """The states k LCG steps earlier (wgsl:196: s' = s * A + C mod 2^32)."""
    s = np.asarray(states, np.uint64)
    ainv = np.uint64(pow(A_LCG, -1, 2 ** 32))
    for _ in range(k):
        s = ((s - np.uint64(C_LCG)) * ainv) & np.uint64(0xffffffff)
    return s.astype(np.uint32)


def step_forward(states, k):
    s = np.asarray(states, np.uint64)
    for _ in range(k):
        s = (s * np.uint64(A_LCG) + np.uint64(C_LCG)) & np.uint64(0xffffffff)
    return s.astype(np.uint32)


def _f32dot(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def overshooting_units(n, seed=7):
    """Binary32 unit vectors v (outputs of the kernels' normalize) whose dot(v, v), summed as the kernels sum it, rounds
    ABOVE 1: rd = -v, normal = v gives dot(-rd, n) > 1 (where min_ clamps), rd = v gives dot(-rd, n) < -1 (where
    1 - cos^2 < 0 and the square root is NaN)."""
    rng = np.random.default_rng(seed)
    v = unit(rng, 200 * n)
    v = v[_f32dot(v, v) > F32(1)]
    assert len(v) >= n, "no unit vector whose squared length rounds above 1 was found"
    return v[:n]


# ---- families -----------------------------------------------------------------------------------------------------------
NB, RPP = 4, 4


def _batch(cases, nb=NB, rpp=RPP, skybox=1):
    return dict(cases=np.ascontiguousarray(cases), nb=nb, rpp=rpp, skybox=skybox)


def _states(rng, n):
    return rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)


def _all_objects(arrays):
    return make(len(materials_of(arrays)), obj=np.arange(len(materials_of(arrays))))


def _is_glass(arrays):
    return np.array([int(m["flag"]) == A.MATERIAL_GLASS for m in materials_of(arrays)])


def fam_random(arrays, n):
    rng = np.random.default_rng(101)
    nm = len(materials_of(arrays))
    back = (rng.uniform(size=n) < 0.4).astype(np.uint32)
    # (A render's backface hit carries a normal turned against the ray, dot(rd, n) < 0; a fifth of them here have it > 0.
    # Not more: with the ray on the normal's side the reflected and the diffuse direction face each other, their mix is
    # short far more often, and the frosted glass materials went past the cap on ill-conditioned cases -- 4 % of such hits
    # against 1 % of the others.)
    nrm, rd = facing(rng, n, back & (rng.uniform(size=n) < 0.2))
    T = np.concatenate([1.0 - rng.uniform(size=(n, 3)), np.ones((n, 1))], -1)
    return [_batch(make(n, obj=np.arange(n) % nm, rd=rd, normal=nrm, backface=back, T=T, light=rng.uniform(0, 2, (n, 4)),
                        total=rng.uniform(0, 10, (n, 4)), rng=_states(rng, n), seg=rng.integers(0, NB + 1, n), j=rng.integers(0, RPP, n),
                        dst=rng.uniform(0.01, 5, n), point=rng.uniform(-3, 3, (n, 3)), u=rng.uniform(0, 1, n), v=rng.uniform(0, 1, n),
                        meta=rng.integers(0, 100, n)))]


def fam_incidence(arrays):
    rng = np.random.default_rng(102)
    geo = []
    for nrm in [np.array([[0, 1, 0]], F32), np.array([[0, 0, -1]], F32), unit(rng, 2)]:   # rd = -n exactly
        geo.append(make(len(nrm), normal=nrm, rd=-nrm))
        geo.append(make(len(nrm), normal=nrm, rd=nrm, backface=1))
    geo.append(make(2, normal=(0, 1, 0), rd=[(1, 0, 0), (0, 0, -1)]))                      # dot exactly 0
    geo.append(make(1, normal=(0.6, 0.8, 0), rd=(0, 0, 1), backface=1))
    for k in range(1, 25):                                                                 # |dot| = 2^-k
        c = 2.0 ** -k
        geo.append(make(1, normal=(0, 1, 0), rd=(np.sqrt(1 - c * c), -c, 0)))
        geo.append(make(1, normal=(0, 1, 0), rd=(0, c, -np.sqrt(1 - c * c)), backface=1))
    v = overshooting_units(16)
    assert (_f32dot(v, v) > F32(1)).all() and (-_f32dot(v, v) < F32(-1)).all()
    geo.append(make(len(v), normal=v, rd=-v))                                              # dot(-rd, n) rounds above 1
    geo.append(make(len(v), normal=v, rd=v, backface=1))                                   # ... below -1
    geo = np.concatenate(geo)
    n_st = 8 if len(materials_of(arrays)) < 20 else 3
    st = make(n_st, rng=_states(rng, n_st))
    return [_batch(cross(geo, _all_objects(arrays), st))]


def _critical_geometry(eta, n_frames, rng):
    """Unit (n, rd) pairs within a few ulps of the critical angle of relative index eta > 1, on both of its sides, and what
    the shader's two tests of it say in binary32: ior * sin_theta > 1 (wgsl:427) and refract's k < 0."""
    eta32 = F32(eta)
    thc = np.arcsin(1.0 / float(eta32))
    nrm = np.repeat(unit(rng, n_frames), 81, 0).astype(np.float64)
    t = np.cross(nrm, np.repeat(unit(rng, n_frames), 81, 0))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    # (steps of one binary32 ulp of ior * sin_theta: d(eta sin) / d(theta) = sqrt(eta^2 - 1) at the critical angle; near
    # eta = 1 that angle is a few steps from grazing, where the scan stops)
    step = 6e-8 / np.sqrt(float(eta32) ** 2 - 1.0)
    th = np.clip(thc + np.tile(np.arange(-40, 41) * step, n_frames), 0.0, np.pi / 2)
    rd = (np.sin(th)[:, None] * t - np.cos(th)[:, None] * nrm).astype(F32)   # (the normal is turned against the ray, as a render's is)
    nrm = nrm.astype(F32)
    cos_t = np.minimum(_f32dot(-rd, nrm), F32(1))
    with np.errstate(invalid="ignore"):
        sin_t = np.sqrt(F32(1) - cos_t * cos_t)
        cannot = eta32 * sin_t > F32(1)
        d = _f32dot(nrm, rd)
        k = F32(1) - (eta32 * eta32) * (F32(1) - d * d)
    return nrm, rd, cannot, k < 0


def fam_critical(arrays):
    """Per glass material with a critical angle (relative index > 1 on the side it is hit from), directions within a few ulps
    of it.  Asserts that the cases where `cannot_refract` and refract's `k < 0` disagree are present."""
    rng = np.random.default_rng(103)
    out, disagree, sides = [], 0, 0
    for obj, m in enumerate(materials_of(arrays)):
        if int(m["flag"]) != A.MATERIAL_GLASS:
            continue
        ior = F32(m["ior"])
        for backface in (0, 1):
            with np.errstate(divide="ignore", over="ignore"):
                eta = ior if backface else F32(1) / ior
            if not (np.isfinite(eta) and eta > 1):
                continue
            nrm, rd, cannot, kneg = _critical_geometry(eta, 8, rng)
            assert cannot.any() and not cannot.all() and kneg.any() and not kneg.all(), (obj, backface)
            disagree += int((cannot != kneg).sum())
            sides += 1
            out.append(make(len(rd), obj=obj, normal=nrm, rd=rd, backface=backface, rng=_states(rng, len(rd)), dst=0.5))
    assert sides and disagree, "the critical family holds no case where ior * sin_theta > 1 and k < 0 disagree"
    return [_batch(np.concatenate(out))]


def fam_edge_draws(arrays, names):
    """RNG states whose d-th draw is exactly 0.0 or rounds to 1.0, for the draw d of each decision, on the materials whose
    threshold there is exactly 0 or 1."""
    E = edge_states()
    rng = np.random.default_rng(104)
    ix = {n: i for i, n in enumerate(names)}
    out = []

    gn, gd = facing(rng, 3, np.zeros(3))

    def add(draw, objs, **k):
        st = make(len(E), rng=step_back(E, draw - 1))
        geo = k.pop("geo", None)   # (default: straight incidence and three others)
        for g in [geo] if geo is not None else [dict()] + [dict(normal=gn[i], rd=gd[i]) for i in range(3)]:
            out.append(cross(make(len(objs), obj=objs, **g, **k), st))
    plain_edges = [ix[n] for n in ("zero", "one", "below_one", "mirror_half", "mid")]
    add(1, plain_edges)                                   # specular >= rand with specular 0 / 1
    for d in (3, 5, 7):                                   # each Box-Muller second draw: log(0), log(1)
        add(d, [ix["mid"], ix["one"]])
    add(8, plain_edges, T=(1, 1, 1, 1))                   # rand >= p with p = 0 / 1
    add(8, plain_edges, T=(0.5, 1, 0.25, 1))
    if "glass_1_clear" in ix:
        g = [ix[n] for n in ("glass_1_clear", "glass_inf_clear", "glass_0_clear", "glass_1.5_clear", "glass_1.5_frosted", "glass_1+_matte")]
        nrm, rd = facing(rng, 1, [0])
        for k in (dict(), dict(normal=nrm, rd=rd), dict(normal=(0, 1, 0), rd=(0, 1, 0), backface=1)):
            add(1, g, geo=k)                              # reflectance > rand with reflectance 0 (ior 1, rd = -n) / 1 (ior 0, inf)
            for d in (3, 5, 7, 8):
                add(d, g[3:5], geo=k)
        graze = dict(normal=(0, 1, 0), rd=(np.sqrt(1 - 0.01), 0.1, 0), backface=1)   # total internal reflection: no Schlick draw
        for d in (2, 4, 6, 7):
            add(d, g[3:5], geo=graze)
    return [_batch(np.concatenate(out))]


def fam_throughput(arrays, names):
    rng = np.random.default_rng(105)
    ix = {n: i for i, n in enumerate(names)}
    Ts = []
    for p in (0.0, SUB, 2.0 ** -121, 1.0, UP1, 2.0 ** 120, 2.0 ** 121, INF):
        for w in (1.0, 0.5, 7.0):
            Ts += [(p, p / 2, p / 4, w), (p / 4, p, p / 2, w), (p / 2, p / 4, p, w)]
    for q in (NAN, -1.0, -0.0, -INF):
        Ts += [(q, 0.5, 0.25, 1), (0.5, q, 0.25, 1), (0.5, 0.25, q, 1), (q, q, 0.5, 1), (q, q, q, 1), (0.5, 0.25, 0.75, q)]
    objs = [ix[n] for n in ("one", "mid", "nan_x", "negative", "lamp")] + ([ix["glass_1.5_clear"], ix["glass_1.5_frosted"], ix["tex_5x3"]] if "tex_5x3" in ix else [])
    nrm, rd = facing(rng, 24, np.zeros(24))
    geo = make(24, normal=nrm, rd=rd, rng=_states(rng, 24), light=rng.uniform(0, 1, (24, 4)))
    return [_batch(cross(make(len(Ts), T=np.array(Ts)), make(len(objs), obj=objs), geo))]


def fam_absorption(arrays):
    rng = np.random.default_rng(106)
    g = np.flatnonzero(_is_glass(arrays))
    if g.size == 0:
        return []
    nrm, rd = facing(rng, 60, np.arange(60) % 2)
    geo = make(60, normal=nrm, rd=rd, backface=1, rng=_states(rng, 60), T=np.concatenate([1.0 - rng.uniform(size=(60, 3)), np.ones((60, 1))], -1))
    dst = make(5, dst=[0.0, 1e-5, 10.0, 2.0 ** 127, 0.3])
    return [_batch(cross(make(len(g), obj=g), dst, geo))]


def fam_texture(arrays, names):
    rng = np.random.default_rng(107)
    objs = [i for i, n in enumerate(names) if n.startswith("tex_")]
    if not objs:
        return []
    vals = [0.0, 0.5, DOWN1, 1.0, -0.25, 3.75, 0.1, 1e6, -1e6, 1e30, INF, -INF, NAN]
    uv = np.array([(a, b) for a in vals for b in vals], F32)
    nrm, rd = facing(rng, 12, np.zeros(12))
    geo = make(12, normal=nrm, rd=rd, rng=_states(rng, 12))
    return [_batch(cross(make(len(uv), u=uv[:, 0], v=uv[:, 1]), make(len(objs), obj=objs), geo))]


def fam_misses(arrays):
    rng = np.random.default_rng(108)
    sun = normalize3_f32([[0.1, 1.0, 0.1]])[0]
    dirs = np.concatenate([np.array([(0, 1, 0), (0, -1, 0), (1, 0, 0), (0, 0, -1), (1, -0.0, 0), sun, -sun], F32),
                           normalize3_f32([(1, 1e-3, 0), (1, -1e-3, 0), (1, -0.009, 0), (1, -0.011, 0), (1, 0.4, 0), (1, 0.45, 0)]),
                           normalize3_f32(sun[None, :] + 0.05 * rng.normal(size=(40, 3))), unit(rng, 400)])
    n = len(dirs) * 24
    c = make(n, hit=0, rd=np.repeat(dirs, 24, 0), T=rng.uniform(0, 1.5, (n, 4)), light=rng.uniform(0, 2, (n, 4)), total=rng.uniform(0, 10, (n, 4)),
             rng=_states(rng, n), seg=rng.integers(0, NB + 1, n), j=rng.integers(0, RPP, n), obj=np.arange(n) % len(materials_of(arrays)))
    return [_batch(c, skybox=1), _batch(c, skybox=0)]


def fam_bookkeeping(arrays, names):
    rng = np.random.default_rng(109)
    ix = {n: i for i, n in enumerate(names)}
    out = []
    for nb, rpp in ((4, 4), (0, 1), (2, 8)):
        segs = sorted({0, max(nb - 1, 0), nb, nb + 1})
        js = sorted({0, max(rpp - 2, 0), rpp - 1})
        parts = [make(len(segs), seg=segs), make(len(js), j=js), make(2, mode=[STEP_END, STEP_TRAVERSE]),
                 make(5, meta=[0, 0xfffe, 0xffff, 0x12340005, 0x0678fffe]), make(2, hit=[0, 1]),
                 make(3, obj=[ix["one"], ix["zero"], ix["mid"]])]
        nrm, rd = facing(rng, 7, np.zeros(7))
        parts.append(make(7, normal=nrm, rd=rd, rng=_states(rng, 7), light=rng.uniform(0, 1, (7, 4)), total=rng.uniform(0, 5, (7, 4))))
        out.append(_batch(cross(*parts), nb=nb, rpp=rpp))
    return out


def families(which, n_random=None):
    """{family: [batch, ...]} of the palette `which` ("plain" / "general")."""
    arrays, names = palette(which)
    n_random = n_random or (30000 if which == "plain" else 66000)
    f = dict(random=fam_random(arrays, n_random), incidence=fam_incidence(arrays), critical=fam_critical(arrays) if which == "general" else [],
             edge_draws=fam_edge_draws(arrays, names), throughput=fam_throughput(arrays, names), absorption=fam_absorption(arrays),
             texture=fam_texture(arrays, names), misses=fam_misses(arrays), bookkeeping=fam_bookkeeping(arrays, names))
    f = {k: v for k, v in f.items() if v}
    for k, v in f.items():
        total = sum(len(b["cases"]) for b in v)
        assert total <= 100000, (k, total)
    return f


# ---- the roulette skip ----------------------------------------------------------------------------------------------------
def roulette_cases(arrays, names, rpp):
    """Cases for the probe's roulette-skip mode on the PLAIN materials of a palette (+ the materials it must refuse, when the
    palette has them): j in {0, rpp - 1}, random states and the edge states aligned to draw 5 (is_spec) and draw 12 (the
    roulette), counted from the start of the sample (four jitter draws first)."""
    rng = np.random.default_rng(110 + rpp)
    E = edge_states()
    st = np.concatenate([_states(rng, 150), step_back(E, 4), step_back(E, 11)])
    n = len(st)
    objs = [i for i, n_ in enumerate(names)]
    parts = [make(len(objs), obj=objs), make(len(sorted({0, rpp - 1})), j=sorted({0, rpp - 1})),
             make(n, rng=st, total=rng.uniform(0, 4, (n, 4)), meta=rng.choice([0, 3, 0xfffd, 0xfffe, 0xffff, 0x00a80002], n))]
    return cross(*parts)


def roulette_expected(oracle, arrays, cases, rpp):
    """What roulette_skip must leave for `cases`: oracle.shade stepped sample by sample from the same state (four LCG steps
    for the jitter draws, then the primary hit with T = 1, no light, seg 0) until the first survivor.  Glass and textured
    materials are refused: nothing moves.  Returns the words the probe reports: total (4), RNG state, j, return value,
    n_segments, meta, dead count."""
    mats = materials_of(arrays)
    refused = np.array([int(m["flag"]) == A.MATERIAL_GLASS or (int(m["flag"]) == A.MATERIAL_TEXTURE and int(m["diffuse_index"]) != -1) for m in mats])
    cur = cases.copy()
    cur[:, C_T:C_T + 4] = bits(np.ones((len(cur), 4)))
    cur[:, C_LIGHT:C_LIGHT + 4] = 0
    cur[:, C_SEG] = 0
    cur[:, C_MODE] = STEP_TRAVERSE
    cur[:, C_HIT] = 1
    dead = np.zeros(len(cur), np.uint32)
    going = ~refused[cases[:, C_OBJ]] & (cur[:, C_J].view(np.int32) < rpp)
    for _ in range(rpp):
        if not going.any():
            break
        trial = cur[going].copy()
        trial[:, C_RNG] = step_forward(trial[:, C_RNG], 4)
        r = oracle.shade(arrays, trial, number_of_bounces=4, rays_per_pixel=rpp)
        died = (r[:, R_FRESH] == 1)      # (seg 0 of 4 bounces: the path only ends here by dying)
        idx = np.flatnonzero(going)
        d = idx[died]
        cur[d, C_TOTAL:C_TOTAL + 4] = r[died, R_TOTAL:R_TOTAL + 4]
        cur[d, C_RNG] = r[died, R_RNG]
        cur[d, C_J] = r[died, R_J]
        cur[d, C_META] = r[died, R_META]
        dead[d] += 1
        going[idx[~died]] = False
        going &= cur[:, C_J].view(np.int32) < rpp
    out = np.zeros((len(cur), 10), np.uint32)
    out[:, 0:4] = cur[:, C_TOTAL:C_TOTAL + 4]
    out[:, 4] = cur[:, C_RNG]
    out[:, 5] = cur[:, C_J]
    out[:, 6] = (dead > 0) & (cur[:, C_J].view(np.int32) >= rpp)
    out[:, 7] = dead
    out[:, 8] = cur[:, C_META]
    out[:, 9] = dead
    return out


ROULETTE_WORDS = [R_TOTAL, R_TOTAL + 1, R_TOTAL + 2, R_TOTAL + 3, R_RNG, R_J, R_RET, R_NSEG, R_META, R_DEAD]


# ---- against the float64 reference ------------------------------------------------------------------------------------------
TOL, FLOOR = 1e-5, 1e-3   # the pin of tests/test_f64_pin.py: |a - b| <= TOL max(|b|, FLOOR)


def as_f64(words):
    return np.ascontiguousarray(words).view(np.float32).astype(np.float64)


def reference(fscene, cases, nb, rpp, skybox):
    """independent_f64.scatter on the case records + path_end's bookkeeping: dict of the record's fields, and `ambiguous`."""
    c = cases
    i32 = lambda w: c[:, w].view(np.int32).astype(np.int64)  # noqa: E731
    shaded = c[:, C_MODE] != STEP_END
    hit = (c[:, C_HIT] != 0) & shaded
    s = F.scatter(fscene, dict(rd=as_f64(c[:, 0:3]), T=as_f64(c[:, 3:7]), light=as_f64(c[:, 7:11]), rng=c[:, C_RNG], hit=hit, dst=as_f64(c[:, C_DST]),
                               point=as_f64(c[:, 21:24]), normal=as_f64(c[:, 24:27]), uv=as_f64(c[:, 27:29]), backface=c[:, C_BACK] != 0,
                               which=c[:, C_OBJ].astype(np.int64)), skybox=skybox)
    # (STEP_END: nothing is shaded -- the sky of those cases' misses is taken back)
    light = np.where(shaded[:, None], s["light"], as_f64(c[:, 7:11]))
    seg = i32(C_SEG) + s["goes_on"]
    end = ~s["goes_on"] | (seg > nb)
    total_in = as_f64(c[:, 11:15])
    with np.errstate(invalid="ignore", over="ignore"):
        total = np.where(end[:, None], F.r32(total_in + light), total_in)
        # (total += light: light carries at most four roundings, the sum one more -- a sum that cancels below that is ambiguous)
        cancel = end & (F.U32 * (4.0 * np.abs(light) + np.abs(total)) > TOL * np.maximum(np.abs(total), FLOOR)).any(-1)
    j = i32(C_J) + end
    meta = c[:, C_META].astype(np.int64)
    meta = np.where(shaded & ((meta & 0xffff) != 0xffff), meta + 1, meta)
    return dict(ro=s["ro"], rd=s["rd"], T=s["T"], light=light, total=total, rng=s["rng"], seg=seg, j=j, fresh=end, ret=end & (j >= rpp),
                nseg=shaded.astype(np.int64), meta=meta, ambiguous=s["ambiguous"] | cancel)


def compare(fscene, records, cases, nb, rpp, skybox):
    """Indices of the unambiguous cases whose record (the oracle's or the kernel's) departs from the float64 reference, with
    what departed; and the ambiguous mask."""
    ref = reference(fscene, cases, nb, rpp, skybox)
    r = records
    bad = {}

    def note(name, mask):
        mask = mask & ~ref["ambiguous"]
        if mask.any():
            bad[name] = np.flatnonzero(mask)
    for name, w, signed in (("rng", R_RNG, False), ("seg", R_SEG, True), ("j", R_J, True), ("fresh", R_FRESH, False),
                            ("ret", R_RET, False), ("nseg", R_NSEG, False), ("meta", R_META, False)):
        got = r[:, w].view(np.int32).astype(np.int64) if signed else r[:, w].astype(np.int64)
        note(name, got != np.asarray(ref[name]).astype(np.int64))
    # Every float output is held to the pin per value, with ONE exception: for the new direction rd, |b| is the vector's
    # largest component.  binary32's error of a component of a unit vector is a fraction of the vector's length, not of the
    # component -- the sphere sample's angle 2 pi r alone is off by 6e-7 through the rounding of r, so a component of 1e-3 is
    # good to 1e-7 and not to 1e-8 -- and a per-component bound would measure the reference's own rounding (it departs on
    # 1.6 % of the general palette's random family).  The origin ro = point + 1e-4 n sign is good to its own ulp per
    # component and is held per component, like T, light and total.
    for name, w, m, vector in (("ro", R_RO, 3, False), ("rd", R_RD, 3, True), ("T", R_T, 4, False), ("light", R_LIGHT, 4, False),
                               ("total", R_TOTAL, 4, False)):
        a, b = as_f64(r[:, w:w + m]), ref[name]
        fa, fb = np.isfinite(a), np.isfinite(b)
        with np.errstate(invalid="ignore", over="ignore"):
            size = np.abs(np.where(fb, b, 0.0))
            if vector:
                size = np.broadcast_to(size.max(-1, keepdims=True), size.shape)
            off = np.abs(a - b) > TOL * np.maximum(size, FLOOR)
        note(name, ((fa != fb) | (fa & fb & off)).any(-1))
    return bad, ref["ambiguous"]
