"""An independent numpy restatement of adaptive sampling (include/rt_abi.h: rt_adaptive_plan, rt_adaptive_merge), sharing no
code with csrc/rt_adaptive.h: the quantisation in numpy float32 (sqrt and division correctly rounded, one operation per
rounding), F = floor(c R / S) in Python integers, the merge in numpy float32 one sample index at a time.  Both give an account
of which rules the input met, for the tests to assert that their planes meet every one."""
import numpy as np

F32, U32 = np.float32, np.uint32
RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("seed", "<u4"), ("dir", "<f4", 3), ("_p0", "<u4")])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype.itemsize == 4 and b.dtype.itemsize == 4 and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    return a.view(U32) == b.view(U32)


def plan(variance, dirs, origin, budget, min_samples, max_samples, first_frame, stats=None):
    """-> counts (H, W) u32, offsets (H, W) u32, rays (budget,) RAY_DTYPE, totals (4,) u32."""
    v = np.ascontiguousarray(variance, F32)
    H, W = v.shape
    flat = v.ravel()
    with np.errstate(all="ignore"):
        takes = np.isfinite(flat) & (flat > 0)
    q = np.zeros(H * W, np.int64)
    if takes.any():
        M = flat[takes].max()
        with np.errstate(all="ignore"):
            ratio = (np.sqrt(flat[takes]) / np.sqrt(M)).astype(F32)
            q[takes] = (ratio * F32(1048576.0)).astype(F32).astype(np.int64)   # (truncation of a value in 0 .. 2^20)
    S = int(q.sum())
    R = int(budget) - int(min_samples) * H * W
    assert R >= 0
    counts = np.zeros(H * W, np.int64)
    clamped = 0
    c = 0
    wanted = np.zeros(H * W, np.int64)
    for p in range(H * W):
        e = 0
        if S:
            e = ((c + int(q[p])) * R) // S - (c * R) // S
        c += int(q[p])
        wanted[p] = min_samples + e
        counts[p] = min(wanted[p], max_samples)
        clamped += wanted[p] > max_samples
    offsets = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    total = int(counts.sum())
    assert total <= budget
    rays = np.zeros(int(budget), RAY_DTYPE)
    d = np.ascontiguousarray(dirs, F32).reshape(H * W, 3)
    owner = np.repeat(np.arange(H * W, dtype=np.int64), counts)
    k = np.arange(total, dtype=np.int64) - offsets[owner]
    rays["origin"][:total] = np.asarray(origin, F32)
    rays["dir"][:total] = d[owner]
    rays["seed"][:total] = ((owner + (int(first_frame) + k) * 719393) & 0xFFFFFFFF).astype(U32)
    totals = np.array([total, int((counts > min_samples).sum()), clamped, 0], U32)
    if stats is not None:
        bits = flat.view(U32)
        stats.update(S=S, R=R, q=q.reshape(H, W), wanted=wanted.reshape(H, W), takes=takes.reshape(H, W),
                     zero=int((flat == 0).sum()), negative=int((flat < 0).sum()), nan=int(np.isnan(flat).sum()),
                     pos_inf=int((flat == np.inf).sum()), neg_inf=int((flat == -np.inf).sum()),
                     denormal=int((takes & ((bits & 0x7f800000) == 0)).sum()), at_max=int((q == 1048576).sum()),
                     clamped=clamped, wrapped_seeds=int(((owner + (int(first_frame) + k) * 719393) > 0xFFFFFFFF).sum()),
                     diffused=int(((wanted - min_samples) == 0).sum()))
    return counts.astype(U32).reshape(H, W), offsets.astype(U32).reshape(H, W), rays, totals


def luminance(c):
    return ((F32(0.2126) * c[..., 0] + F32(0.7152) * c[..., 1]).astype(F32) + F32(0.0722) * c[..., 2]).astype(F32)


def merge(radiance, counts, offsets, color, history, max_history=np.inf, albedo=None, moments=None, stats=None):
    """-> out (H, W, 4), out_history (H, W), out_moments (H, W, 4) or None."""
    rad = np.ascontiguousarray(radiance, F32)
    budget = rad.shape[0]
    H, W = counts.shape
    n = counts.ravel().astype(np.int64)
    off = offsets.ravel().astype(np.int64)
    acc = np.ascontiguousarray(color, F32).reshape(H * W, 4).copy()
    hist = np.ascontiguousarray(history, F32).ravel().copy()
    with np.errstate(all="ignore"):
        prior = np.isfinite(hist) & (hist >= 1) & np.isfinite(acc).all(-1)
    hl = np.where(prior, hist, F32(0)).astype(F32)
    m = np.ascontiguousarray(moments, F32).reshape(H * W, 4).copy() if moments is not None else None
    al = np.ones((H * W, 3), F32)
    if albedo is not None:
        a = np.ascontiguousarray(albedo, F32).reshape(H * W, 4)[:, :3]
        with np.errstate(all="ignore"):
            al = np.where(a > F32(2.0 ** -10), a, F32(2.0 ** -10)).astype(F32)
    mh = F32(max_history)
    note = dict(no_prior=int((~prior).sum()), dropped=0, first=0, blended=0, capped=0, untouched=0)
    for k in range(int(n.max()) if n.size else 0):
        idx = off + k
        live = (k < n) & (idx < budget)
        c = rad[np.where(live, idx, 0)]
        with np.errstate(all="ignore"):
            fin = np.isfinite(c).all(-1)
            valid = live & fin
            note["dropped"] += int((live & ~fin).sum())
            first = valid & (hl == 0)
            blend = valid & (hl != 0)
            s = np.zeros((H * W, 4), F32)
            if m is not None:
                l = luminance((c[:, :3] / al).astype(F32))
                s[:, 0] = l
                s[:, 1] = (l * l).astype(F32)
            n_c = np.where(hl < mh, hl, mh).astype(F32)
            note["capped"] += int((blend & ~(hl < mh)).sum())
            w = (F32(1) / (n_c + F32(1)).astype(F32)).astype(F32)
            rest = (F32(1) - w).astype(F32)
            mixed = ((acc * rest[:, None]).astype(F32) + (c * w[:, None]).astype(F32)).astype(F32)
            acc = np.where(first[:, None], c, np.where(blend[:, None], mixed, acc))
            if m is not None:
                mm = ((m * rest[:, None]).astype(F32) + (s * w[:, None]).astype(F32)).astype(F32)
                m = np.where(first[:, None], s, np.where(blend[:, None], mm, m))
            hl = np.where(first, F32(1), np.where(blend, (n_c + F32(1)).astype(F32), hl)).astype(F32)
        note["first"] += int(first.sum())
        note["blended"] += int(blend.sum())
    note["untouched"] = int((hl == 0).sum())
    if stats is not None:
        stats.update(note)
    return acc.reshape(H, W, 4), hl.reshape(H, W), (m.reshape(H, W, 4) if m is not None else None)


def variance_plane(W, H, seed=3, specials=True):
    """A synthetic variance plane: log-normal values over five decades, and -- where the frame has room -- a 0, a negative, a
    NaN, both infinities, a denormal, a -0 and a second texel at the maximum."""
    rng = np.random.default_rng(seed + 131 * W + H)
    v = np.exp(rng.normal(-4.0, 2.5, (H, W))).astype(F32)
    flat = v.ravel()
    if specials:
        special = [0.0, -1.5, np.nan, np.inf, -np.inf, 1e-42, -0.0, None]
        where = rng.permutation(flat.size)[:min(len(special), max(flat.size - 1, 0))]
        for i, s in zip(where, special):
            if s is None:   # (the maximum of what is left, a second time)
                rest = np.delete(flat, where)
                s = rest[np.isfinite(rest)].max()
            flat[i] = F32(s)
    return flat.reshape(H, W)


def dir_plane(W, H, seed=5):
    rng = np.random.default_rng(seed + W)
    d = rng.normal(0, 1, (H, W, 3)).astype(F32)
    d.reshape(-1, 3)[0] = (0.0, 0.0, 0.0)   # (copied bit for bit, whatever it holds)
    d.reshape(-1, 3)[-1] = (np.nan, -0.0, 1e-40)
    return d


def merge_case(W, H, counts, budget, seed=11):
    """Planes for the merge over a plan's `counts`: histories 0, below 1, NaN, infinite and ordinary; non-finite colours; and
    samples that are not finite -- the first, a middle one, and all of a texel's -- where some texel has the samples for it."""
    rng = np.random.default_rng(seed + W * 7 + H)
    n = counts.ravel().astype(np.int64)
    off = np.concatenate([[0], np.cumsum(n)[:-1]])
    rad = rng.uniform(0, 3, (budget, 4)).astype(F32)
    color = rng.uniform(0, 2, (H * W, 4)).astype(F32)
    hist = rng.integers(1, 12, H * W).astype(F32)
    kinds = [0.0, 0.5, np.nan, np.inf, -3.0, 0.999]
    order = rng.permutation(H * W)
    for i, p in enumerate(order[:max(1, (H * W) // 3)]):
        hist[p] = F32(kinds[i % len(kinds)])
    for i, p in enumerate(order[::7][:6]):
        color[p, i % 4] = F32([np.nan, np.inf, -np.inf][i % 3])
    bad = dict(first=0, middle=0, all=0)
    multi = [p for p in order if n[p] >= 3]
    for i, p in enumerate(multi[:9]):
        if i % 3 == 0:
            rad[off[p], 1] = np.nan
            bad["first"] += 1
        elif i % 3 == 1:
            rad[off[p] + 1, 3] = np.inf
            bad["middle"] += 1
        else:
            rad[off[p]:off[p] + n[p], 0] = -np.inf
            bad["all"] += 1
    single = [p for p in order if n[p] == 1]
    for p in single[:2]:
        rad[off[p], 2] = np.nan
        bad["all"] += 1
    albedo = rng.uniform(0.0, 1, (H * W, 4)).astype(F32)
    albedo[order[:3], 0] = np.array([0.0, np.nan, 1e-5], F32)[:len(order[:3])]
    moments = rng.uniform(0, 2, (H * W, 4)).astype(F32)
    return dict(radiance=rad, color=color.reshape(H, W, 4), history=hist.reshape(H, W), albedo=albedo.reshape(H, W, 4),
                moments=moments.reshape(H, W, 4)), bad


# ---- the cases the CPU and the GPU tests share ----
SIZES = [(24, 16), (67, 45), (1, 1), (8, 1), (1, 8)]
ORIGIN = (0.25, -1.5, 3.0)


def plan_cases(W, H):
    """(name, variance, budget, min_samples, max_samples, first_frame) for a W x H frame."""
    T = W * H
    v = variance_plane(W, H)
    spike = np.full((H, W), F32(1e-6))
    spike.ravel()[::5] = F32(4.0)       # a fifth of the texels want everything: max_samples clamps them
    return [
        ("defaults", v, 5 * T, 1, 16, 0),
        ("no clamp", v, 5 * T, 1, 65535, 7),
        ("clamped", spike, 9 * T, 1, 12, 0),
        ("all zero", np.zeros((H, W), F32), 3 * T, 2, 8, 0),
        ("nothing takes part", np.full((H, W), F32(np.nan)), 3 * T, 1, 8, 0),
        ("min 0", v, 4 * T, 0, 16, 3),
        ("R = 0", v, 2 * T, 2, 16, 0),
        ("small budget", v, T + max(1, T // 16), 1, 16, 0),
        ("seed wraps", v, 5 * T, 1, 16, 0xFFFFFFFE),
        ("budget beyond the plan", spike, 40 * T + 3000, 1, 4, 1),
        ("min = max", v, 3 * T, 3, 3, 0),
    ]


def assert_plan_equal(got, want, what):
    for g, w, name in zip(got, want, ("counts", "offsets", "rays", "totals")):
        assert g.shape == w.shape, (what, name)
        assert np.array_equal(np.ascontiguousarray(g).view(np.uint8), np.ascontiguousarray(w).view(np.uint8)), (what, name)


def merge_inputs(W, H):
    """A plan with texels of 0 to 16 samples (and 5 records of tail) and merge_case's planes over it."""
    T = W * H
    v = variance_plane(W, H)
    counts, offsets, _, totals = plan(v, dir_plane(W, H), ORIGIN, 4 * T + 5, 0, 16, 0)
    planes, bad = merge_case(W, H, counts, 4 * T + 5)
    return counts, offsets, planes, bad
