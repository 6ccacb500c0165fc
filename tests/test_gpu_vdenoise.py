"""rt_denoise_variance and rt_luminance_moments (include/rt_abi.h; csrc/rt_vdenoise.hip) against their host forms, bit for
bit, on real planes -- render_gbuffer plus renders of the Cornell fixture -- through the host path; then the scratch shared
with rt_denoise, its bookkeeping, side effects and errors.  The device path (torch tensors, a NULL colour for the handle's
image) runs in a process of its own: tests/_vdenoise_device_path.py."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import _vdenoise_reference as R
from ray_tracer_2_amd import _abi as A

pytestmark = pytest.mark.gpu

F32 = np.float32
SIGMAS = (4.0, 0.3, 1.0)
# 130x70 is wider than any tile in both axes (tiles are 32x8): every step crosses tile seams, step 16 included, and so do
# the 7x7 and 3x3 windows
SIZES = [(67, 45), (24, 16), (130, 70)]
SMALL = [(1, 1), (8, 1), (1, 8)]
CHANNELS = ("normal", "point", "albedo", "emission")

_frames = {}


def frame(rt, tracer, cornell, W, H):
    """Of the Cornell fixture at W x H, rendered once per size: color (one 8 spp, 4 bounce frame), the guides, and a
    moments / history pair that puts both branches of the variance estimate in one frame -- the moments of two raw frames
    (device luminance_moments) blended, a history of 8 on the left half and of 1 on the right."""
    if (W, H) not in _frames:
        tracer.load_scene(cornell)
        g = tracer.render_gbuffer(rt.make_params(W, H, 1, 1), CHANNELS)
        raw = []
        for k in (0, 1):
            tracer.render(rt.make_params(W, H, 4, 8, skybox=1, frames=-k))
            raw.append(tracer.read_image(W, H).copy())
        color = raw[0]
        ok = R.classify(color, g["normal"], g["point"], g["emission"])
        assert 0.3 < ok.mean() < 0.9, (W, H, float(ok.mean()))      # filterable texels, and misses or lamps beside them
        assert (g["emission"][..., :3] != 0).any()                    # the lamp is in view
        lm = [tracer.luminance_moments(g, c) for c in raw]
        moments = (F32(0.5) * lm[0] + F32(0.5) * lm[1]).astype(F32)
        history = np.where(np.arange(W)[None, :] < (W + 1) // 2, F32(8), F32(1)) * np.ones((H, 1), F32)
        _frames[(W, H)] = (color, g, moments, history.astype(F32))
    return _frames[(W, H)]


def crop(rt, tracer, cornell, W, H):
    """A W x H window of the 67x45 frame that straddles the edge of the lamp: filterable and emissive texels."""
    color, g, moments, history = frame(rt, tracer, cornell, 67, 45)
    lamp = np.argwhere((g["emission"][..., :3] != 0).any(-1))
    y0, x0 = (int(v) for v in lamp.min(0))
    y0, x0 = max(0, y0 - H // 2), max(0, x0 - W // 2)
    s = (slice(y0, y0 + H), slice(x0, x0 + W))
    cut = np.ascontiguousarray
    return cut(color[s]), {k: cut(v[s]) for k, v in g.items()}, cut(moments[s]), cut(history[s])


def pick(g, albedo, emission):
    return {k: v for k, v in g.items() if k in ("normal", "point") or (k == "albedo" and albedo) or (k == "emission" and emission)}


def same(got, want, what):
    for a, b, name in zip(got, want, ("out", "out_variance")) if isinstance(got, tuple) else ((got, want, "out"),):
        bad = ~R.same_bits(a, b)
        assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())


@pytest.mark.parametrize("W,H", SIZES)
def test_device_equals_host(rt, tracer, cornell, oracle, W, H):
    """Iterations 1 .. 5 with every optional plane on and off; the moments put both branches in one frame."""
    color, g, moments, history = frame(rt, tracer, cornell, W, H)
    st = {}
    R.reference(oracle, color, g["normal"], g["point"], g["albedo"], g["emission"], 1, *SIGMAS, moments, history, 4.0, stats=st)
    share = st["temporal"].sum() / st["ok"].sum()
    assert 0.2 < share < 0.8, share                                   # both branches, by the reference's account
    assert (st["var0"][st["ok"]] > 0).mean() > 0.5
    for n in range(1, 6):
        for albedo, emission, mom in itertools.product((True, False), repeat=3):
            gg = pick(g, albedo, emission)
            kw = dict(moments=moments, history=history) if mom else {}
            want = rt.denoise_variance_host(gg, color, n, *SIGMAS, out_variance=True, **kw)
            same(tracer.denoise_variance(gg, color, n, *SIGMAS, out_variance=True, **kw), want, (W, H, n, albedo, emission, mom))
            if n == 3 and albedo and emission:
                ok = st["ok"]
                assert (~R.same_bits(want[0][ok][:, :3], color[ok][:, :3])).mean() > 0.9   # (the filter did something)
                same(want[0][~ok], color[~ok], "copied through")
                assert (want[1][~ok] == 0).all() and (want[1][ok] > 0).mean() > 0.5
    kw = dict(moments=moments, history=history)
    # eight passes (steps up to 128, beyond the frame), another min_history, no out_variance, and out = color
    same(tracer.denoise_variance(g, color, 8, *SIGMAS, out_variance=True, **kw),
         rt.denoise_variance_host(g, color, 8, *SIGMAS, out_variance=True, **kw), (W, H, 8))
    same(tracer.denoise_variance(g, color, 2, *SIGMAS, min_history=9.0, **kw),
         rt.denoise_variance_host(g, color, 2, *SIGMAS, min_history=9.0, **kw), (W, H, "min_history 9"))
    same(tracer.denoise_variance(g, color, 2, *SIGMAS, min_history=1.0, **kw),
         rt.denoise_variance_host(g, color, 2, *SIGMAS, min_history=1.0, **kw), (W, H, "min_history 1"))
    buf = color.copy()
    assert tracer.denoise_variance(g, buf, 3, *SIGMAS, out=buf, **kw) is buf
    same(buf, rt.denoise_variance_host(g, color, 3, *SIGMAS, **kw), (W, H, "out is color"))


@pytest.mark.parametrize("W,H", SIZES + SMALL)
def test_luminance_moments(rt, tracer, cornell, W, H):
    color, g, _, _ = frame(rt, tracer, cornell, W, H) if (W, H) in SIZES else crop(rt, tracer, cornell, W, H)
    for albedo, emission in itertools.product((True, False), repeat=2):
        gg = pick(g, albedo, emission)
        want = rt.luminance_moments_host(gg, color)
        same(tracer.luminance_moments(gg, color), want, (W, H, albedo, emission))
        ok = R.classify(color, g["normal"], g["point"], g["emission"] if emission else None)
        assert (want[~ok] == 0).all() and (want[..., 2:] == 0).all()
        if W * H > 8:
            assert (want[ok][:, 0] > 0).mean() > 0.5   # (not vacuous: most filterable texels of an 8 spp frame are lit)
    buf = color.copy()
    assert tracer.luminance_moments(g, buf, out=buf) is buf
    same(buf, rt.luminance_moments_host(g, color), (W, H, "out is color"))


@pytest.mark.parametrize("W,H", SMALL)
def test_small_frames(rt, tracer, cornell, W, H):
    color, g, moments, history = crop(rt, tracer, cornell, W, H)
    if W * H > 1:
        ok = R.classify(color, g["normal"], g["point"], g["emission"])
        assert ok.any() and not ok.all(), (W, H)
    for n in (1, 2, 5):
        for emission, mom in itertools.product((True, False), repeat=2):
            gg = pick(g, True, emission)
            kw = dict(moments=moments, history=history) if mom else {}
            same(tracer.denoise_variance(gg, color, n, *SIGMAS, out_variance=True, **kw),
                 rt.denoise_variance_host(gg, color, n, *SIGMAS, out_variance=True, **kw), (W, H, n, emission, mom))


def test_synthetic_frame(rt, tracer):
    """The 24x16 frame of the CPU tests, built to meet every rule (NaN, infinity, tiny and negative albedo; histories and
    moments that do not serve)."""
    c, _ = R.synthetic_case()
    g = {k: c[k] for k in CHANNELS}
    for n in range(1, 6):
        for kw in ({}, dict(moments=c["moments"], history=c["history"])):
            same(tracer.denoise_variance(g, c["color"], n, *SIGMAS, out_variance=True, **kw),
                 rt.denoise_variance_host(g, c["color"], n, *SIGMAS, out_variance=True, **kw), (n, bool(kw)))
    same(tracer.luminance_moments(g, c["color"]), rt.luminance_moments_host(g, c["color"]), "moments")


def test_interleaved_with_denoise(rt, tracer, cornell):
    """The two filters share the handle's scratch: interleaved, at two sizes, each gives its own host result."""
    want = {}
    for _ in range(2):
        for W, H in ((130, 70), (67, 45)):
            color, g, moments, history = frame(rt, tracer, cornell, W, H)
            kw = dict(moments=moments, history=history)
            if (W, H) not in want:
                want[(W, H)] = (rt.denoise_host(g, color, 3, *SIGMAS), rt.denoise_variance_host(g, color, 3, *SIGMAS, out_variance=True, **kw),
                                rt.denoise_variance_host(g, color, 4, *SIGMAS, out_variance=True))
            a, b, c = want[(W, H)]
            same(tracer.denoise_variance(g, color, 3, *SIGMAS, out_variance=True, **kw), b, (W, H, "variance"))
            same(tracer.denoise(g, color, 3, *SIGMAS), a, (W, H, "denoise after variance"))
            same(tracer.denoise_variance(g, color, 4, *SIGMAS, out_variance=True), c, (W, H, "variance after denoise"))
            same(tracer.denoise(g, color, 3, *SIGMAS), a, (W, H, "denoise again"))


def test_no_side_effects(rt, tracer, cornell):
    """A render sequence with calls of both entry points between its frames: the image, rt_get_stats and the launch words
    as without."""
    color, g, moments, history = frame(rt, tracer, cornell, 67, 45)

    def run(denoise, frame_ahead):
        tracer.set_option("frame_ahead", frame_ahead)
        tracer.load_scene(cornell)
        tracer.reset_timing()
        for f in range(12):
            tracer.render(rt.make_params(64, 48, 3, 2, skybox=1, frames=f))
            if denoise:
                tracer.luminance_moments(g, color)
                tracer.denoise_variance(g, color, 1 + f % 3, moments=moments if f % 2 else None, history=history if f % 2 else None)
            else:
                tracer.synchronize()   # (a host-path call returns when its data is on the host: the other sequence waits too)
        img = tracer.read_image(64, 48)
        s = tracer.stats()
        return img, (s.segments, s.paths, s.node_tests, s.triangle_tests, s.frames, s.segments_reused, s.frames_speculative), \
            tuple(tracer.last_launch().values())[:-2]

    try:
        for fa in (-1, 8):
            a, sa, la = run(False, fa)
            b, sb, lb = run(True, fa)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), fa
            # (the automatic policy renders ahead by what it finds on the stream: only the frames asked for are schedule-free)
            assert (sa == sb) if fa > 0 else (sa[4] == sb[4]), (fa, sa, sb)
            if fa > 0:
                assert la == lb, (la, lb)
    finally:
        tracer.set_option("frame_ahead", -1)


def _raw(t, planes, W, H, flags=A.VDENOISE_HOST_MEMORY, fn="rt_denoise_variance", **over):
    d = A.VDenoiseDesc(struct_bytes=C.sizeof(A.VDenoiseDesc), width=W, height=H, iterations=2, sigma_luminance=4.0, sigma_normal=0.3,
                       sigma_point=1.0, min_history=4.0)
    for k, v in planes.items():
        setattr(d, k, v.ctypes.data)
    for k, v in over.items():
        setattr(d, k, v)
    return getattr(t._L, fn)(t._h, C.byref(d), flags)


def _planes(W, H):
    rng = np.random.default_rng(7)
    p = {"color": rng.uniform(0, 2, (H, W, 4)), "normal": np.tile([0.0, 0.0, 1.0], (H, W, 1)), "point": rng.uniform(0, 1, (H, W, 3)),
         "albedo": rng.uniform(0.2, 1, (H, W, 4)), "emission": np.zeros((H, W, 4)), "moments": rng.uniform(1, 2, (H, W, 4)),
         "history": rng.integers(1, 9, (H, W))}
    p = {k: np.ascontiguousarray(v, F32) for k, v in p.items()}
    p["out"] = np.full((H, W, 4), F32(-7.25))
    p["out_variance"] = np.full((H, W), F32(-7.25))
    return p


def _host_of(rt, p, n=2):
    return rt.denoise_variance_host({k: p[k] for k in CHANNELS}, p["color"], n, *SIGMAS, moments=p["moments"], history=p["history"],
                                    out_variance=True)


def test_scratch_is_shared_counted_and_capped(rt):
    """rt_denoise's 64 bytes per texel, held after the first call of either filter (rt_last_launch out[4]) and not twice;
    a cap that has no room for them: RT_ERR_OUT_OF_MEMORY, the outputs untouched; rt_luminance_moments needs none; no
    scene is needed."""
    t = rt.RayTracer(device=0, max_width=16, max_height=16)
    try:
        W, H = 512, 256
        p = _planes(W, H)
        before = t.last_launch()["device_mb_held"]
        t.set_option("max_device_mb", before + 4)    # the scratch alone is 8 MiB
        assert _raw(t, p, W, H) == -8 and b"max_device_mb" in t._L.rt_last_error(t._h)
        assert np.all(p["out"] == F32(-7.25)) and np.all(p["out_variance"] == F32(-7.25))
        assert t.last_launch()["device_mb_held"] == before
        t.set_option("max_device_mb", 0)
        assert _raw(t, p, W, H, fn="rt_luminance_moments") == 0
        assert t.last_launch()["device_mb_held"] == before    # (no scratch for the moments)
        same(p["out"], rt.luminance_moments_host({k: p[k] for k in CHANNELS}, p["color"]), "moments 512x256")
        assert _raw(t, p, W, H) == 0
        same((p["out"], p["out_variance"]), _host_of(rt, p), "512x256")
        assert t.last_launch()["device_mb_held"] == before + 8
        dn = A.DenoiseDesc(struct_bytes=C.sizeof(A.DenoiseDesc), width=W, height=H, iterations=2, sigma_color=4.0, sigma_normal=0.3,
                           sigma_point=1.0)
        for k in A.DENOISE_PLANES:
            setattr(dn, k, p[k].ctypes.data)
        assert t._L.rt_denoise(t._h, C.byref(dn), A.DENOISE_HOST_MEMORY) == 0
        assert t.last_launch()["device_mb_held"] == before + 8    # (one scratch for both)
        same(p["out"], rt.denoise_host({k: p[k] for k in CHANNELS}, p["color"], 2, *SIGMAS), "rt_denoise in the same scratch")
        small = _planes(8, 8)                          # a smaller frame reuses the scratch
        assert _raw(t, small, 8, 8) == 0
        assert t.last_launch()["device_mb_held"] == before + 8
        t.set_option("max_device_mb", before + 8)     # the scratch is held already, but the staging planes need room too
        assert _raw(t, p, W, H) == -8 and b"max_device_mb" in t._L.rt_last_error(t._h)
        assert _raw(t, p, W, H, fn="rt_luminance_moments") == -8 and b"max_device_mb" in t._L.rt_last_error(t._h)
    finally:
        t.close()


def test_errors(rt):
    """The argument errors on the device entry points, the device-only ones included; the outputs stay as they were."""
    t = rt.RayTracer(device=0, max_width=16, max_height=16)
    L, h = t._L, t._h
    W, H = 8, 6

    def err():
        return L.rt_last_error(h).decode()

    try:
        p = _planes(W, H)
        d = A.VDenoiseDesc(struct_bytes=C.sizeof(A.VDenoiseDesc))
        for fn in ("rt_denoise_variance", "rt_luminance_moments"):
            assert getattr(L, fn)(None, C.byref(d), 1) == -1
            assert getattr(L, fn)(h, None, 1) == -1 and "null" in err()
            assert _raw(t, p, W, H, flags=3, fn=fn) == -1 and "flags" in err()
            assert _raw(t, p, W, H, flags=-2, fn=fn) == -1 and "flags" in err()
            for over, text in ((dict(struct_bytes=88), "struct_bytes"), (dict(_p0=1), "_p0"), (dict(_p1=1), "_p1"), (dict(width=0), "zero"),
                               (dict(height=0), "zero"), (dict(normal=None), "null"), (dict(point=None), "null"), (dict(out=None), "null")):
                for flags in (0, 1):
                    assert _raw(t, p, W, H, flags=flags, fn=fn, **over) == -1 and text in err(), (fn, over, flags, err())
            assert _raw(t, p, W, H, flags=1, fn=fn, color=None) == -1 and "color" in err()
            assert _raw(t, p, 1 << 16, 1 << 15, fn=fn) == -2 and "2^31" in err()
            assert _raw(t, p, 17, 16, flags=0, fn=fn, color=None) == -2 and "image" in err()
        for over, text in ((dict(iterations=0), "iterations"), (dict(iterations=9), "iterations"), (dict(sigma_luminance=0.0), "sigma"),
                           (dict(sigma_luminance=float("inf")), "finite"), (dict(sigma_normal=float("nan")), "sigma"),
                           (dict(sigma_normal=float("inf")), "finite"), (dict(sigma_point=float("inf")), "finite"),
                           (dict(sigma_point=-1.0), "sigma"), (dict(min_history=0.5), "min_history"),
                           (dict(min_history=float("nan")), "min_history"), (dict(min_history=float("inf")), "min_history"),
                           (dict(moments=None), "go together"), (dict(history=None), "go together")):
            for flags in (0, 1):
                assert _raw(t, p, W, H, flags=flags, **over) == -1 and text in err(), (over, flags, err())
        # device planes (host arrays' addresses stand in for device pointers: the checks come before any use)
        assert all(v.ctypes.data % 16 == 0 for v in p.values())
        need = {"color": 16, "normal": 4, "point": 4, "albedo": 16, "emission": 16, "moments": 16, "history": 4, "out": 16, "out_variance": 4}
        for c, a in need.items():
            for off in (1, 2, 4, 8):
                if off % a:
                    assert _raw(t, p, W, H, flags=0, **{c: p[c].ctypes.data + off}) == -1 and f"plane {c} " in err() and "aligned" in err(), (c, off)
        assert np.all(p["out"] == F32(-7.25)) and np.all(p["out_variance"] == F32(-7.25))
        # what rt_luminance_moments does not examine may hold anything
        assert _raw(t, p, W, H, fn="rt_luminance_moments", iterations=0, sigma_luminance=-1.0, min_history=0.0, history=None) == 0
        assert not np.any(p["out"] == F32(-7.25)) and np.all(p["out_variance"] == F32(-7.25))
        assert _raw(t, p, W, H) == 0 and not np.any(p["out_variance"] == F32(-7.25))
        same((p["out"], p["out_variance"]), _host_of(rt, p), "the call that is right")
    finally:
        t.close()


def test_device_path():
    """Torch tensors on the device (tests/_vdenoise_device_path.py, a process of its own that imports torch first)."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "_vdenoise_device_path.py")],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "device path ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
