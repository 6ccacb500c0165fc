"""An independent restatement of rt_display and rt_auto_exposure (include/rt_abi.h) in numpy float32 and Python integers, and
the frames the display tests share.  The sRGB thresholds are computed here, from the ENCODING in 50-digit decimal arithmetic by
bisection over the floats -- not by the generator's route (the decode, rounded up), and the generated header is never read."""
import functools
from decimal import Decimal, getcontext

import numpy as np

F32, U32 = np.float32, np.uint32
CLAMP, REINHARD, SRGB, LINEAR, BGRA, TOP_FIRST = 0, 1, 0, 1, 1, 2
INF, NAN = F32(np.inf), F32(np.nan)


def f32_of(bits):
    return np.array(bits, U32).view(F32)


def bits_of(x):
    return np.ascontiguousarray(x, F32).view(U32)


def encode_exact(x):
    """IEC 61966-2-1, linear -> sRGB, of the float x as a Decimal of 50 digits."""
    getcontext().prec = 50
    x = Decimal(float(x))
    return x * Decimal("12.92") if x <= Decimal("0.0031308") else Decimal("1.055") * x ** (Decimal(1) / Decimal("2.4")) - Decimal("0.055")


@functools.lru_cache(None)
def thresholds():
    """T[0 .. 255] as uint32 bit patterns, T[0] = 0: T[k] the smallest float whose exact encoding is >= (k - 1/2) / 255."""
    getcontext().prec = 50
    out = [0]
    for k in range(1, 256):
        want = (Decimal(k) - Decimal("0.5")) / Decimal(255)
        lo, hi = 0, int(bits_of(1.0)[0])   # encode(lo) < want <= encode(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if encode_exact(f32_of(mid)) >= want:
                hi = mid
            else:
                lo = mid
        out.append(hi)
    return np.array(out, U32)


def srgb_byte_f64(t):
    """round(255 srgb(clamp(t))) by the float64 formula: what the thresholds must agree with away from the half-way points."""
    t = np.clip(np.asarray(t, np.float64), 0.0, 1.0)
    s = np.where(t <= 0.0031308, 12.92 * t, 1.055 * np.power(t, 1 / 2.4) - 0.055)
    return np.floor(255.0 * s + 0.5).astype(np.uint8), 255.0 * s


def linear_byte(t):
    with np.errstate(all="ignore"):
        l = np.where(t > 0, np.minimum(t, F32(1)), F32(0)).astype(F32)
        return (l * F32(255) + F32(0.5)).astype(U32).astype(np.uint8)


def display(color, tone=CLAMP, transfer=SRGB, layout=0, exposure=1.0, white=np.inf, exposure_scale=None):
    color = np.ascontiguousarray(color, F32)
    e = F32(exposure)
    if exposure_scale is not None:
        s = F32(np.asarray(exposure_scale, F32).reshape(-1)[0])
        if np.isfinite(s) and s > 0:
            e = F32(e * s)
    with np.errstate(all="ignore"):
        v = color[..., :3] * e
        m = np.where(v >= 0, np.minimum(v, F32(2.0 ** 64)), F32(0)).astype(F32)
        if tone == REINHARD:
            ww = F32(F32(white) * F32(white))
            t = ((m * (F32(1) + m / ww)) / (F32(1) + m)).astype(F32)
        else:
            t = m
    if transfer == SRGB:
        T = thresholds()[1:].view(F32)
        rgb = np.searchsorted(T, np.where(np.isnan(t), F32(0), t), side="right").astype(np.uint8)
    else:
        rgb = linear_byte(t)
    out = np.concatenate([rgb, linear_byte(color[..., 3:])], -1)
    if layout & BGRA:
        out = out[..., [2, 1, 0, 3]]
    if layout & TOP_FIRST:
        out = out[::-1]
    return np.ascontiguousarray(out)


def histogram(color):
    c = np.ascontiguousarray(color, F32).reshape(-1, 4)
    Y = luminance(c)
    counted = (Y > 0) & (Y < INF)
    b = np.clip((bits_of(Y[counted]) >> 20).astype(np.int64) - 888, 0, 255)
    return np.bincount(b, minlength=256).astype(U32)


def meter(n, low, high, key=0.18, min_scale=2.0 ** -10, max_scale=2.0 ** 10, rate=1.0, prev=None):
    """The scale from the counts, in Python integers up to the last operations."""
    n = [int(v) for v in n]
    N = sum(n)
    lo, hi = N * low // 1000, N * high // 1000
    start = kept = S = 0
    for b, nb in enumerate(n):
        k = max(0, min(start + nb, hi) - max(start, lo))
        kept += k
        S += k * b
        start += nb
    target = F32(1)
    if kept:
        mbar = F32(F32(S) / F32(kept))
        ybar = np.array([U32(F32((mbar + F32(888.5)) * F32(1048576.0)))], U32).view(F32)[0]
        with np.errstate(all="ignore"):
            target = F32(min(max(F32(F32(key) / ybar), F32(min_scale)), F32(max_scale)))
    if prev is not None and np.isfinite(prev) and prev > 0:
        prev = F32(prev)
        return F32(prev + F32(F32(target - prev) * F32(rate)))
    return target


def bin_edges(b):
    """The first and last float of bin b among the counted ones (bins 0 and 255 take the clamped ends too)."""
    first = 1 if b == 0 else (888 + b) << 20
    last = 0x7f7fffff if b == 255 else ((889 + b) << 20) - 1
    return f32_of(first), f32_of(last)


SPECIALS = [0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -1.0, -1e30, 1.0, 1.0000001, 2.0, 255.0, 3e38, np.inf, -np.inf, np.nan, 0.5, 0.18]


def threshold_frame(W, H):
    """A W x H frame that holds every T[k] with both neighbours, and the special values, in colour and in alpha, repeated to fill."""
    T = thresholds()[1:].astype(np.int64)
    vals = np.concatenate([f32_of((T[:, None] + np.array([-1, 0, 1])).ravel().astype(U32)), np.array(SPECIALS, F32)])
    n = W * H * 4
    flat = np.resize(vals, n).copy()
    # (a stride that is coprime to four walks every value through every channel)
    flat[3::4] = np.resize(np.roll(vals, 5), W * H)
    return flat.reshape(H, W, 4)


def hdr_frame(W=37, H=19, seed=11):
    """A seeded HDR frame, values 2^-20 .. 2^20 with some negatives, zeros, infinities and NaN sprinkled in."""
    rng = np.random.default_rng(seed)
    c = np.exp2(rng.uniform(-20, 20, (H, W, 4))).astype(F32)
    c[..., 3] = rng.uniform(-0.5, 1.5, (H, W)).astype(F32)
    flat = c.reshape(-1)
    n = min(24, flat.size // 4)   # (a 1 x 1 frame takes one)
    idx = rng.choice(flat.size, n, replace=False)
    flat[idx] = np.resize(np.array(SPECIALS, F32), n)
    return c


def luminance(c):
    c = np.ascontiguousarray(c, F32)
    with np.errstate(all="ignore"):
        return ((F32(0.2126) * c[..., 0] + F32(0.7152) * c[..., 1]) + F32(0.0722) * c[..., 2]).astype(F32)


def color_with_luminance(v):
    """(c0, c1, 0, 1) whose luminance is the float v exactly: green carries it, and where 0.7152 g steps over v, a little red
    makes up the difference before the sum is rounded."""
    v = F32(v)
    if np.float64(v) / 0.7152 > 3e38:   # (green alone would overflow: a grey a few floats around v)
        for d in range(-16, 17):
            x = f32_of(int(bits_of(v)[0]) + d)
            if luminance(np.array([x, x, x, 1], F32)) == v:
                return np.array([x, x, x, 1], F32)
        raise AssertionError(v)
    g = F32(np.float64(v) / 0.7152)
    a = F32(F32(0.7152) * g)
    r = F32(0) if a == v else F32((np.float64(v) - np.float64(a)) / 0.2126)
    c = np.array([r, g, 0, 1], F32)
    assert luminance(c) == v, (v, c)
    return c


def every_bin_frame(W, H):
    """Every bin's first and last float as the luminance of a texel, the uncounted classes, and noise over 2^-18 .. 2^18."""
    rng = np.random.default_rng(3)
    c = np.exp2(rng.uniform(-18, 18, (H, W, 4))).astype(F32)
    flat = c.reshape(-1, 4)
    k = 0
    for b in range(256):
        for v in bin_edges(b):
            flat[k] = color_with_luminance(v)
            k += 1
    for v in (0.0, -1.0, np.nan, np.inf, -np.inf):
        flat[k] = (v, v, v, 1)
        k += 1
    assert k < W * H
    return c


def one_bin_frame(W, H, b=100):
    """Every texel's luminance in bin b: green alone, (0, g, 0), with 0.7152 g inside the bin."""
    lo, hi = (float(v) for v in bin_edges(b))
    g = np.random.default_rng(4).uniform(lo * 1.01, hi * 0.99, (H, W)) / 0.7152
    c = np.zeros((H, W, 4), F32)
    c[..., 1] = g.astype(F32)
    c[..., 3] = 1
    assert np.count_nonzero(histogram(c)) == 1 and histogram(c)[b] == W * H
    return c
