"""An independent numpy restatement of the denoiser's definition (include/rt_abi.h: rt_denoise), and the two frames the
denoiser's tests run on.

`reference` evaluates the filter tap by tap over the whole image in numpy float32 -- every operation one rounded binary32
ufunc, in the order the definition gives, nothing fused -- and takes its exponential from the oracle
(oracle.transc("exp", ...): rt_transc.h's exp_ compiled for the CPU).  It shares no code with csrc/rt_denoise.h.

`synthetic_case` is a 24x16 frame built to meet every rule; `cornell_case` is the Cornell fixture at 67x45 with guides from
oracle.intersect on the texel rays and colour from one oracle.render frame at 8 spp and 4 bounces."""
import functools

import numpy as np

F32 = np.float32
H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], F32)
FLOOR = F32(2.0 ** -10)


def classify(color, normal, point, emission):
    """The filterable texels, (H, W) bool."""
    ok = (normal != 0).any(-1)   # (a NaN is non-zero; the next line refuses it)
    ok &= np.isfinite(normal).all(-1) & np.isfinite(point).all(-1) & np.isfinite(color[..., :3]).all(-1)
    if emission is not None:
        ok &= (emission[..., :3] == 0).all(-1)
    return ok


def _d2(a, P, Q):
    d = a[P] - a[Q]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def reference(oracle, color, normal, point, albedo, emission, iterations, sigma_color, sigma_normal, sigma_point, stats=None):
    """out (H, W, 4) float32.  stats (a dict, optional) receives counts over the tap pairs that were evaluated -- q inside
    the frame, p and q filterable, q != p --: `pairs`, `rejected` (exp_(-e) < 0.01) and `accepted` (exp_(-e) > 0.5)."""
    color, normal, point = (np.ascontiguousarray(a, F32) for a in (color, normal, point))
    H, W = color.shape[:2]
    ok = classify(color, normal, point, emission)
    with np.errstate(all="ignore"):
        k_c = F32(1) / (F32(sigma_color) * F32(sigma_color))
        k_n = F32(1) / (F32(sigma_normal) * F32(sigma_normal))
        k_x = F32(1) / (F32(sigma_point) * F32(sigma_point))
        if albedo is None:
            a = np.ones((H, W, 3), F32)
        else:
            al = np.ascontiguousarray(albedo, F32)[..., :3]
            a = np.where(al > FLOOR, al, FLOOR).astype(F32)
        c = color[..., :3] / a
        pairs = rejected = accepted = 0
        for i in range(iterations):
            s = 1 << i
            k_ci = k_c * F32(4 ** i)
            total = np.zeros((H, W, 3), F32)
            wsum = np.zeros((H, W), F32)
            for dy in range(-2, 3):
                y0, y1 = max(0, -s * dy), min(H, H - s * dy)
                for dx in range(-2, 3):
                    x0, x1 = max(0, -s * dx), min(W, W - s * dx)
                    if y0 >= y1 or x0 >= x1:
                        continue
                    P = (slice(y0, y1), slice(x0, x1))
                    Q = (slice(y0 + s * dy, y1 + s * dy), slice(x0 + s * dx, x1 + s * dx))
                    both = ok[P] & ok[Q]
                    e = (_d2(c, P, Q) * k_ci + _d2(normal, P, Q) * k_n) + _d2(point, P, Q) * k_x
                    ex = oracle.transc("exp", np.ascontiguousarray(-e)).reshape(e.shape)
                    w = (H5[dx + 2] * H5[dy + 2]) * ex
                    take = both & (w > 0)
                    # (a skipped tap adds +0, which leaves a sum that started at +0 as it is)
                    total[P] += np.where(take[..., None], w[..., None] * c[Q], F32(0))
                    wsum[P] += np.where(take, w, F32(0))
                    if stats is not None and (dx or dy):
                        pairs += int(both.sum())
                        rejected += int((both & (ex < 0.01)).sum())
                        accepted += int((both & (ex > 0.5)).sum())
            c = np.where(ok[..., None], total / wsum[..., None], c).astype(F32)
        out = color.copy()
        out[..., :3] = np.where(ok[..., None], c * a, color[..., :3])
    if stats is not None:
        stats.update(pairs=pairs, rejected=rejected, accepted=accepted)
    return out


def same_bits(a, b):
    """Bit for bit; a NaN equals any NaN."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


@functools.lru_cache(maxsize=None)
def synthetic_case():
    """24x16: two planes that meet at a crease (x = 12), a band of misses (rows 6 and 7), an emissive patch, texels whose
    albedo is below 2^-10 (and one that is zero, one negative), one NaN normal, one infinite colour, random colours with a
    few fireflies.  Returns a dict of read-only planes."""
    W, H = 24, 16
    rng = np.random.default_rng(2013)
    y, x = np.mgrid[0:H, 0:W].astype(F32)
    left = x < 12
    normal = np.where(left[..., None], F32([0, 0, 1]), F32([0.6, 0, 0.8])).astype(F32)
    point = np.stack([np.where(left, x * F32(0.1), F32(1.2) + (x - 12) * F32(0.08)), y * F32(0.1),
                      np.where(left, F32(0), (x - 12) * F32(-0.06))], -1).astype(F32)
    albedo = np.concatenate([rng.uniform(0.2, 0.9, (H, W, 3)), np.ones((H, W, 1))], -1).astype(F32)
    emission = np.zeros((H, W, 4), F32)
    color = np.concatenate([rng.uniform(0, 3, (H, W, 3)), rng.uniform(0, 1, (H, W, 1))], -1).astype(F32)
    fire = rng.random((H, W)) < 0.05
    color[fire, :3] *= F32(20)
    miss = (y == 6) | (y == 7)
    normal[miss] = 0
    point[miss] = 0
    albedo[miss] = 0
    emission[10:13, 3:6] = F32([5, 4, 3, 1])
    albedo[2, 15] = F32([1e-4, 0.5, 2.0 ** -10, 1])
    albedo[3, 16] = F32([0, -1, 0.25, 1])
    albedo[12, 20] = F32([2.0 ** -11, 2.0 ** -11, 2.0 ** -11, 1])
    normal[3, 20] = F32([np.nan, 0, 1])
    color[2, 8, 0] = np.inf
    color[13, 9, 3] = np.nan    # (alpha is carried, never examined)
    case = dict(color=color, normal=normal, point=point, albedo=albedo, emission=emission)
    for v in case.values():
        v.setflags(write=False)
    return case


_cornell = {}


def cornell_case(rt, oracle, arrays, W=67, H=45):
    """The Cornell fixture at 67x45: `normal` and `point` from oracle.intersect on the texel rays (zeros on a miss),
    `emission` from the material of the winning object, `albedo` all ones, `color` one oracle.render frame at 8 spp and 4
    bounces, and `converged`, the mean of 256 such frames.  Computed once."""
    key = (W, H)
    if key in _cornell:
        return _cornell[key]
    from oracle import independent_f64 as F
    ro, rd = F.primary_rays(F.Scene(arrays), W, H)
    rec = oracle.intersect(arrays, ro.astype(F32), rd.astype(F32))
    hit = (rec[:, 0] != 0) & np.isfinite(rec[:, 1].view(F32))
    normal = np.where(hit[:, None], rec[:, 5:8].view(F32), F32(0)).reshape(H, W, 3).astype(F32)
    point = np.where(hit[:, None], rec[:, 2:5].view(F32), F32(0)).reshape(H, W, 3).astype(F32)
    mats = np.concatenate([arrays.meshes["material"], arrays.spheres["material"]])
    emission = np.zeros((H * W, 4), F32)
    m = mats[rec[hit, 11]]
    emission[hit] = (m["emission_color"] * m["emission_strength"][:, None]).astype(F32)
    emission = emission.reshape(H, W, 4)
    albedo = np.ones((H, W, 4), F32)
    color, _ = oracle.render(rt.make_params(W, H, 4, 8, skybox=1, frames=0), arrays)
    color = color.copy()
    acc = None
    for f in range(256):
        acc, _ = oracle.render(rt.make_params(W, H, 4, 8, skybox=1, frames=f), arrays, image=acc)
    case = dict(color=color, normal=normal, point=point, albedo=albedo, emission=emission, converged=acc)
    for v in case.values():
        v.setflags(write=False)
    _cornell[key] = case
    return case
