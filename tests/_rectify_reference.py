"""An independent numpy restatement of history rectification's definition (include/rt_abi.h: rt_temporal_rectify), one
rounded float32 ufunc per operation, whole planes at a time; the frames the tests share.  No code in common with
csrc/rt_rectify.h: a tap that does not count leaves the sums as they are by not being added, the window is walked as shifted
views of the planes."""
import functools

import numpy as np

F32 = np.float32
U32 = np.uint32
NO_HISTORY, KEPT, CLIPPED = 0, 1, 2
DEFAULTS = dict(radius=3, clip_sigma=1.0, clip_history=4.0)


def same_bits(a, b):
    """Bit for bit; a NaN equals any NaN."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return (a.view(U32) == b.view(U32)) | (np.isnan(a) & np.isnan(b))


def reference(color, history, history_length, object=None, radius=3, clip_sigma=1.0, clip_history=4.0, moments=None,
              history_moments=None, stats=None):
    """(out, out_history, out_moments or None, out_clipped) of the definition.  stats, when given, receives per texel:
    `have` (a history), `count` (c), `box` (a box was formed), `sd` (H, W, 3), `at_lo` / `at_hi` ((H, W, 3): the channel was
    clamped there), `clipped`, `cut` (the length was cut), `dropped` (a sample with history that is not finite)."""
    color, history, n = (np.ascontiguousarray(v, F32) for v in (color, history, history_length))
    H, W = n.shape
    r = int(radius)
    g, ch = F32(clip_sigma), F32(clip_history)
    fin = np.isfinite
    have = fin(history).all(-1) & fin(n) & (n >= 1)
    rgb = color[..., :3]
    tap_ok = fin(rgb).all(-1)
    s1, s2, c = np.zeros((H, W, 3), F32), np.zeros((H, W, 3), F32), np.zeros((H, W), np.int64)
    with np.errstate(all="ignore"):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                # the texels p whose tap q = p + (dx, dy) is inside the frame, and those taps
                py, px = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
                qy, qx = slice(max(0, -dy) + dy, min(H, H - dy) + dy), slice(max(0, -dx) + dx, min(W, W - dx) + dx)
                if py.start >= py.stop or px.start >= px.stop:
                    continue
                take = tap_ok[qy, qx].copy()
                if object is not None:
                    take &= object[qy, qx] == object[py, px]
                v = rgb[qy, qx]
                s1[py, px] = np.where(take[..., None], s1[py, px] + v, s1[py, px])
                s2[py, px] = np.where(take[..., None], s2[py, px] + v * v, s2[py, px])
                c[py, px] += take
        cf = c.astype(F32)[..., None]
        mu, m2 = s1 / cf, s2 / cf
        var = m2 - mu * mu
        var = np.where(var > 0, var, F32(0))
        sd = np.sqrt(var)
        lo, hi = mu - g * sd, mu + g * sd
        h = history[..., :3]
        box = have & (c >= 2) & bool(g < np.inf)
        at_lo = box[..., None] & (h < lo)
        at_hi = box[..., None] & ~at_lo & (h > hi)
        hp = np.where(at_lo, lo, np.where(at_hi, hi, h)).astype(F32)
        clipped = (hp.view(U32) != h.view(U32)).any(-1)
        cut = clipped & (ch < n)
        n2 = np.where(cut, ch, n).astype(F32)
        w = F32(1) / (n2 + F32(1))
        rest = F32(1) - w
        h4 = np.concatenate([hp, history[..., 3:]], -1)
        sample_ok = fin(color).all(-1)
        blend = h4 * rest[..., None] + color * w[..., None]
        out = np.where(sample_ok[..., None], blend, h4)
        out_history = np.where(sample_ok, n2 + F32(1), n2)
        out = np.where(have[..., None], out, color).astype(F32)
        out_history = np.where(have, out_history, F32(1)).astype(F32)
        out_clipped = np.where(have, np.where(clipped, CLIPPED, KEPT), NO_HISTORY).astype(np.uint8)
        out_moments = None
        if moments is not None:
            m, hm = np.ascontiguousarray(moments, F32), np.ascontiguousarray(history_moments, F32)
            mix = hm * rest[..., None] + m * w[..., None]
            om = np.where(fin(hm).all(-1)[..., None], np.where(fin(m).all(-1)[..., None], mix, hm), m)
            out_moments = np.where(have[..., None], om, m).astype(F32)
    if stats is not None:
        stats.update(have=have, count=c, box=box, sd=np.where(box[..., None], sd, F32(np.nan)), at_lo=at_lo, at_hi=at_hi,
                     clipped=have & clipped, cut=have & cut, dropped=have & ~sample_ok)
    return out, out_history, out_moments, out_clipped


# ---- the synthetic frame ----
SYN_W, SYN_H = 40, 20       # two tiles of 32 x 8 across, three up, partial ones at both seams
EQUAL = (F32(0.5), F32(0.75), F32(3.0))   # the colour of the constant block and the constant island: few mantissa bits


@functools.lru_cache(maxsize=None)
def synthetic_case():
    """A 40 x 20 frame built to meet every rule: colours uniform in [0.2, 1), histories in [0.3, 0.9) (a box of one standard
    deviation then clamps about a channel in four, at either end, and about half the texels); a 9 x 9 block of one colour at columns 2 .. 10 of rows 2 .. 10, whose
    inner 3 x 3 texels see nothing else at radius 3 (sd = 0 without an object plane); the object plane: 1 everywhere, a
    4 x 3 island of object 5 of that one colour inside noise (sd = 0 with the plane only), one lone texel of object 7 (c = 1
    with the plane), a band of misses (0xffffffff, which match each other); NaN and infinities in single colours (taps that
    do not count, samples that are dropped), an infinite alpha alone (the tap counts, the sample is dropped); every form
    of "no history"; placed histories that clamp at lo in one channel and at hi in another, that are cut and that are too
    short to be cut; -0 in colours and histories; moments with each of the two non-finite rules.  Returns (planes, notes):
    planes = color, history, history_length, object, moments, history_moments (read-only), notes names texels (y, x)."""
    W, H = SYN_W, SYN_H
    rng = np.random.default_rng(2031)
    color = rng.uniform(0.2, 1.0, (H, W, 4)).astype(F32)
    history = rng.uniform(0.3, 0.9, (H, W, 4)).astype(F32)
    length = rng.integers(1, 11, (H, W)).astype(F32)
    obj = np.ones((H, W), U32)
    moments = rng.uniform(0.0, 2.0, (H, W, 4)).astype(F32)
    hmoments = rng.uniform(0.0, 2.0, (H, W, 4)).astype(F32)
    notes = {}
    # the constant block; its centre texels: a history inside (kept), above and below (clipped onto the colour exactly)
    color[2:11, 2:11, :3] = EQUAL
    history[5, 5, :3] = EQUAL
    history[6, 6, :3] = (2.0, 2.0, 4.0)
    history[7, 7, :3] = (0.25, 0.25, 0.25)
    notes.update(equal_kept=(5, 5), equal_above=(6, 6), equal_below=(7, 7))
    # the island of object 5 in noise, the lone texel of object 7, the band of misses
    obj[13:16, 20:24] = 5
    color[13:16, 20:24, :3] = EQUAL
    history[14, 21, :3] = (0.125, 1.0, 3.5)
    notes["island"] = (14, 21)
    obj[16, 30] = 7
    history[16, 30, :3] = (9.0, 9.0, 9.0)
    notes["lone"] = (16, 30)
    obj[18, 5:30] = 0xFFFFFFFF
    # taps that do not count; with their own finite histories the samples are dropped
    color[3, 20, 1] = np.nan
    color[3, 24, 2] = np.inf
    color[4, 28, 0] = -np.inf
    color[8, 33, 3] = np.inf          # alpha alone: the tap counts
    notes.update(nan_sample=(3, 20), inf_sample=(3, 24), alpha_sample=(8, 33))
    # no history: every component, every kind; every kind of length
    k = 0
    for comp in range(4):
        for bad in (np.nan, np.inf, -np.inf):
            history[11, 2 + k, comp] = bad
            k += 1
    for x, bad in zip(range(16, 21), (0.0, 0.5, np.nan, np.inf, -np.inf)):
        length[11, x] = bad
    notes["no_history"] = [(11, x) for x in (*range(2, 14), *range(16, 21))]
    # lo in one channel, hi in another, the third inside; long (cut) and short (not cut)
    for name, (y, x), n in (("cut", (9, 20), 9.0), ("short", (9, 26), 2.0), ("edge", (0, 39), 7.0), ("corner", (19, 0), 10.0)):
        history[y, x, :3] = (-5.0, 7.0, color[y, x, 2])
        length[y, x] = n
        notes[name] = (y, x)
    # -0
    color[1, 14:17, 0] = -0.0
    history[1, 15, 0] = -0.0
    history[1, 18, 3] = -0.0
    notes["minus_zero"] = (1, 15)
    # the moments' rules
    hmoments[2, 30, 1] = np.nan
    moments[2, 32, 0] = np.inf
    hmoments[2, 34, 2], moments[2, 34, 3] = -np.inf, np.nan
    notes.update(hm_bad=(2, 30), m_bad=(2, 32), both_bad=(2, 34))
    planes = dict(color=color, history=history, history_length=length, object=obj, moments=moments, history_moments=hmoments)
    for v in planes.values():
        v.setflags(write=False)
    return planes, notes


def small_case(W, H, seed=11):
    """Frames of a texel, a row, a column and a few of each: noise with one object word in two."""
    rng = np.random.default_rng(seed + 64 * W + H)
    f = lambda *s: rng.uniform(0.2, 1.0, s).astype(F32)   # noqa: E731
    return dict(color=f(H, W, 4), history=f(H, W, 4), history_length=rng.integers(1, 9, (H, W)).astype(F32),
                object=(rng.integers(0, 2, (H, W)) + 1).astype(U32), moments=f(H, W, 4), history_moments=f(H, W, 4))


def variants(planes):
    """The optional planes on and off: (name, keyword arguments of the wrappers)."""
    base = {k: planes[k] for k in ("color", "history", "history_length")}
    mom = {k: planes[k] for k in ("moments", "history_moments")}
    yield "all", dict(base, object=planes["object"], **mom)
    yield "no object", dict(base, **mom)
    yield "no moments", dict(base, object=planes["object"])
    yield "neither", base


def check(call, kw, what="", **par):
    """call(**kw, **par, clipped=True) -- a wrapper -- against the reference, bit for bit; and once more without `clipped`.
    Returns the wrapper's outputs as (out, out_history, out_moments or None, out_clipped)."""
    want = reference(kw["color"], kw["history"], kw["history_length"], kw.get("object"), moments=kw.get("moments"),
                     history_moments=kw.get("history_moments"), **par)
    got = call(**kw, **par, clipped=True)
    have_moments = "moments" in kw
    assert len(got) == (4 if have_moments else 3), what
    got = (got[0], got[1], got[2] if have_moments else None, got[-1])
    for a, b, name in zip(got[:3], want[:3], ("out", "out_history", "out_moments")):
        if b is None:
            continue
        bad = ~same_bits(a, b)
        assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert got[3].dtype == np.uint8 and np.array_equal(got[3], want[3]), (what, "out_clipped", np.argwhere(got[3] != want[3])[:4].tolist())
    alone = call(**kw, **par)
    assert len(alone) == (3 if have_moments else 2) and all(same_bits(a, b).all() for a, b in zip(alone, got)), (what, "without out_clipped")
    return got
