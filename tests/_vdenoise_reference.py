"""An independent numpy restatement of the variance-guided denoiser's definition (include/rt_abi.h: rt_denoise_variance,
rt_luminance_moments), and the frames its tests run on.

`reference` evaluates the variance estimate, the prefilter and the filter tap by tap over the whole image in numpy float32
-- every operation one rounded binary32 ufunc, in the order the definition gives, nothing fused -- and takes its
exponential from the oracle (oracle.transc("exp", ...): rt_transc.h's exp_ compiled for the CPU).  It shares no code with
csrc/rt_vdenoise.h; of tests/_denoise_reference.py it uses the classification, the bit comparison and the two frames.

`synthetic_case` is _denoise_reference.synthetic_case() (24x16) with a moments and a history plane built to meet every rule
of the variance estimate; `cornell_history` accumulates N raw Cornell frames and their moments under the unmoved camera."""
import functools

import numpy as np

import _denoise_reference as DR

F32 = DR.F32
H5 = DR.H5
G3 = np.array([1 / 4, 1 / 2, 1 / 4], F32)
FLOOR = DR.FLOOR
EPS = F32(2.0 ** -30)
same_bits = DR.same_bits
classify = DR.classify


def luminance(c):
    return (F32(0.2126) * c[..., 0] + F32(0.7152) * c[..., 1]) + F32(0.0722) * c[..., 2]


def _d2(a, P, Q):
    d = a[P] - a[Q]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _demodulate(color, albedo):
    H, W = color.shape[:2]
    if albedo is None:
        a = np.ones((H, W, 3), F32)
    else:
        al = np.ascontiguousarray(albedo, F32)[..., :3]
        a = np.where(al > FLOOR, al, FLOOR).astype(F32)
    return color[..., :3] / a, a


def _windows(H, W, r, s):
    """(dy, dx, P, Q) for the (2 r + 1)^2 taps at spacing s, dy outer: P the texels whose tap lies inside the frame, Q the taps."""
    for dy in range(-r, r + 1):
        y0, y1 = max(0, -s * dy), min(H, H - s * dy)
        for dx in range(-r, r + 1):
            x0, x1 = max(0, -s * dx), min(W, W - s * dx)
            if y0 >= y1 or x0 >= x1:
                continue
            yield dy, dx, (slice(y0, y1), slice(x0, x1)), (slice(y0 + s * dy, y1 + s * dy), slice(x0 + s * dx, x1 + s * dx))


def moments_reference(color, normal, point, albedo, emission):
    """rt_luminance_moments: (H, W, 4) float32."""
    color, normal, point = (np.ascontiguousarray(a, F32) for a in (color, normal, point))
    ok = classify(color, normal, point, emission)
    with np.errstate(all="ignore"):
        c, _ = _demodulate(color, albedo)
        l = luminance(c)
        out = np.zeros(color.shape, F32)
        out[..., 0] = np.where(ok, l, F32(0))
        out[..., 1] = np.where(ok, l * l, F32(0))
    return out


def reference(oracle, color, normal, point, albedo, emission, iterations, sigma_luminance, sigma_normal, sigma_point,
              moments=None, history=None, min_history=4.0, stats=None):
    """(out (H, W, 4), out_variance (H, W)) float32.  stats (a dict, optional) receives the reference's own account:
    `ok`, `temporal` (the texels whose variance the moments gave), `var0`; `window_outside` and `window_unfilterable`, the
    7 x 7 taps of spatial texels that fell outside the frame or on a texel that is not filterable; and over the tap pairs of
    the passes -- q inside the frame, p and q filterable, q != p -- `pairs`, `lum_rejected` (exp_(-|l_p - l_q| / D) < 0.01)
    and `accepted` (exp_(-e) > 0.5)."""
    color, normal, point = (np.ascontiguousarray(a, F32) for a in (color, normal, point))
    H, W = color.shape[:2]
    ok = classify(color, normal, point, emission)

    def exp_(x):
        return oracle.transc("exp", np.ascontiguousarray(x, F32)).reshape(x.shape)

    with np.errstate(all="ignore"):
        sigma_l = F32(sigma_luminance)
        k_n = F32(1) / (F32(sigma_normal) * F32(sigma_normal))
        k_x = F32(1) / (F32(sigma_point) * F32(sigma_point))
        c, a = _demodulate(color, albedo)
        l = luminance(c)

        # the variance of the input
        temporal = np.zeros((H, W), bool)
        v_t = np.zeros((H, W), F32)
        if moments is not None:
            m = np.ascontiguousarray(moments, F32)
            hist = np.ascontiguousarray(history, F32)
            m1, m2 = m[..., 0], m[..., 1]
            temporal = ok & np.isfinite(hist) & (hist >= F32(min_history)) & np.isfinite(m1) & np.isfinite(m2)
            v_t = (m2 - m1 * m1) / hist
        s1, s2, sw = (np.zeros((H, W), F32) for _ in range(3))
        spatial = ok & ~temporal
        outside = unfilterable = 0
        for dy, dx, P, Q in _windows(H, W, 3, 1):
            u = exp_(-(_d2(normal, P, Q) * k_n + _d2(point, P, Q) * k_x))
            take = ok[P] & ok[Q] & (u > 0)
            s1[P] += np.where(take, u * l[Q], F32(0))
            s2[P] += np.where(take, u * (l[Q] * l[Q]), F32(0))
            sw[P] += np.where(take, u, F32(0))
            outside -= int(spatial[P].sum())
            unfilterable += int((spatial[P] & ~ok[Q]).sum())
        outside += 49 * int(spatial.sum())
        e1, e2 = s1 / sw, s2 / sw
        v = np.where(temporal, v_t, e2 - e1 * e1)
        var = np.where(ok & (v > 0), v, F32(0)).astype(F32)
        var0 = var.copy()

        pairs = lum_rejected = accepted = 0
        for i in range(iterations):
            s = 1 << i
            gs, gw = np.zeros((H, W), F32), np.zeros((H, W), F32)
            for dy, dx, P, Q in _windows(H, W, 1, 1):
                g = G3[dx + 1] * G3[dy + 1]
                gs[P] += np.where(ok[Q], g * var[Q], F32(0))
                gw[P] += np.where(ok[Q], g, F32(0))
            D = sigma_l * np.sqrt(gs / gw) + EPS
            total = np.zeros((H, W, 3), F32)
            vsum, wsum = np.zeros((H, W), F32), np.zeros((H, W), F32)
            for dy, dx, P, Q in _windows(H, W, 2, s):
                both = ok[P] & ok[Q]
                el = np.abs(l[P] - l[Q]) / D[P]
                e = (el + _d2(normal, P, Q) * k_n) + _d2(point, P, Q) * k_x
                ex = exp_(-e)
                w = (H5[dx + 2] * H5[dy + 2]) * ex
                take = both & (w > 0)
                # (a skipped tap adds +0, which leaves a sum that started at +0 as it is)
                total[P] += np.where(take[..., None], w[..., None] * c[Q], F32(0))
                vsum[P] += np.where(take, (w * w) * var[Q], F32(0))
                wsum[P] += np.where(take, w, F32(0))
                if stats is not None and (dx or dy):
                    pairs += int(both.sum())
                    lum_rejected += int((both & (exp_(-el) < 0.01)).sum())
                    accepted += int((both & (ex > 0.5)).sum())
            c = np.where(ok[..., None], total / wsum[..., None], c).astype(F32)
            var = np.where(ok, vsum / (wsum * wsum), var).astype(F32)
            l = luminance(c)
        out = color.copy()
        out[..., :3] = np.where(ok[..., None], c * a, color[..., :3])
        out_variance = np.where(ok, var, F32(0)).astype(F32)
    if stats is not None:
        stats.update(ok=ok, temporal=temporal, var0=var0, window_outside=outside, window_unfilterable=unfilterable, pairs=pairs,
                     lum_rejected=lum_rejected, accepted=accepted)
    return out, out_variance


MIN_HISTORY = 4.0


@functools.lru_cache(maxsize=None)
def synthetic_case():
    """_denoise_reference.synthetic_case() with `moments` and `history`.  Columns 0 .. 11 have a history of 8 frames (the
    moments serve), columns 12 .. 23 of 2 (below MIN_HISTORY: the window serves); single texels have a history that is NaN,
    infinite, 0.5 and 3, moments that are NaN and infinite, and a second moment below the square of the first; rows 0 .. 3 of
    columns 0 .. 4 have m2 = m1 m1 exactly, a variance of 0.  Returns (planes, notes): read-only planes, and where the single
    texels are."""
    base = DR.synthetic_case()
    H, W = base["color"].shape[:2]
    rng = np.random.default_rng(2017)
    mom = moments_reference(base["color"], base["normal"], base["point"], base["albedo"], base["emission"])
    l = mom[..., 0]
    m1 = (l * rng.uniform(0.9, 1.1, (H, W))).astype(F32)
    m2 = (m1 * m1 + rng.uniform(0.0, 4.0, (H, W)).astype(F32)).astype(F32)
    moments = np.stack([m1, m2, np.zeros_like(m1), np.zeros_like(m1)], -1).astype(F32)
    history = np.where(np.arange(W)[None, :] < 12, F32(8), F32(2)) * np.ones((H, 1), F32)
    moments[0:4, 0:5, 0] = F32(2)
    moments[0:4, 0:5, 1] = F32(4)
    notes = dict(history_nan=(9, 2), history_inf=(9, 4), history_below_one=(11, 7), history_short=(13, 3), moment_nan=(14, 5),
                 moment_inf=(5, 8), negative=[(4, 9), (8, 1), (15, 10)], zero=(slice(0, 4), slice(0, 5)))
    history[notes["history_nan"]] = np.nan
    history[notes["history_inf"]] = np.inf
    history[notes["history_below_one"]] = F32(0.5)
    history[notes["history_short"]] = F32(3)
    moments[notes["moment_nan"]][0] = np.nan
    moments[notes["moment_inf"]][1] = np.inf
    for y, x in notes["negative"]:
        moments[y, x, 1] = moments[y, x, 0] * moments[y, x, 0] * F32(0.5)
    planes = dict(base, moments=moments, history=history.astype(F32))
    for k in ("moments", "history"):
        planes[k].setflags(write=False)
    return planes, notes


def accumulate(rt, guides, camera, frames):
    """The running mean of `frames` ((H, W, 4) each) through temporal_accumulate_host under the unmoved camera `camera`:
    (accumulated, history)."""
    out = hist = None
    for k, f in enumerate(frames):
        if k == 0:
            out, hist = f.copy(), np.ones(f.shape[:2], F32)
            continue
        out, hist = rt.temporal_accumulate_host(guides, guides, camera, out, hist, f)
    return out, hist


_histories = {}


def cornell_history(rt, oracle, arrays, case, N, W=67, H=45):
    """N raw frames of the Cornell fixture (8 spp, 4 bounces, frame k the raw sample of seed k: frames = -k), accumulated
    through temporal_accumulate_host under the unmoved camera, and the luminance_moments_host of each accumulated the same
    way.  `case`: _denoise_reference.cornell_case's planes of the same size.  Returns (color, moments, history); once per N."""
    if (N, W, H) in _histories:
        return _histories[(N, W, H)]
    g = {k: case[k] for k in ("normal", "point", "albedo", "emission")}
    raws = []
    for k in range(N):
        raw, _ = oracle.render(rt.make_params(W, H, 4, 8, skybox=1, frames=-k if k else 0), arrays)
        raws.append(raw.copy())
    cam = arrays.uniform.camera
    color, hist = accumulate(rt, g, cam, raws)
    moments, hist2 = accumulate(rt, g, cam, [rt.luminance_moments_host(g, r) for r in raws])
    assert np.array_equal(hist, hist2)
    for v in (color, moments, hist):
        v.setflags(write=False)
    _histories[(N, W, H)] = (color, moments, hist)
    return _histories[(N, W, H)]
