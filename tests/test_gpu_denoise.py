"""rt_denoise (include/rt_abi.h; csrc/rt_denoise.hip) against rt_denoise_host, bit for bit, on real planes -- render_gbuffer
plus one render of the Cornell fixture -- through the host path; then the scratch's bookkeeping, side effects and errors.
The device path (torch tensors, a NULL colour for the handle's image) runs in a process of its own:
tests/_denoise_device_path.py."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import _denoise_reference as R
from ray_tracer_2_amd import _abi as A

pytestmark = pytest.mark.gpu

F32 = np.float32
SIGMAS = (4.0, 0.3, 1.0)
# 130x70 is wider than any tile in both axes (tiles are 32x8): every step crosses tile seams, step 16 included
SIZES = [(67, 45), (24, 16), (130, 70)]
SMALL = [(1, 1), (8, 1), (1, 8)]
CHANNELS = ("normal", "point", "albedo", "emission")

_frames = {}


def frame(rt, tracer, cornell, W, H):
    """color (one 8 spp, 4 bounce frame) and the guides of the Cornell fixture at W x H, rendered once per size."""
    if (W, H) not in _frames:
        tracer.load_scene(cornell)
        tracer.render(rt.make_params(W, H, 4, 8, skybox=1, frames=0))
        color = tracer.read_image(W, H).copy()
        g = tracer.render_gbuffer(rt.make_params(W, H, 1, 1), CHANNELS)
        ok = R.classify(color, g["normal"], g["point"], g["emission"])
        assert 0.3 < ok.mean() < 0.9, (W, H, float(ok.mean()))      # filterable texels, and misses or lamps beside them
        assert (g["emission"][..., :3] != 0).any()                    # the lamp is in view
        _frames[(W, H)] = (color, g)
    return _frames[(W, H)]


def crop(rt, tracer, cornell, W, H):
    """A W x H window of the 67x45 frame that straddles the edge of the lamp: filterable and emissive texels."""
    color, g = frame(rt, tracer, cornell, 67, 45)
    lamp = np.argwhere((g["emission"][..., :3] != 0).any(-1))
    y0, x0 = (int(v) for v in lamp.min(0))
    y0, x0 = max(0, y0 - H // 2), max(0, x0 - W // 2)
    s = (slice(y0, y0 + H), slice(x0, x0 + W))
    return np.ascontiguousarray(color[s]), {k: np.ascontiguousarray(v[s]) for k, v in g.items()}


def pick(g, albedo, emission):
    return {k: v for k, v in g.items() if k in ("normal", "point") or (k == "albedo" and albedo) or (k == "emission" and emission)}


def same(got, want, what):
    bad = ~R.same_bits(got, want)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist())


@pytest.mark.parametrize("W,H", SIZES)
def test_device_equals_host(rt, tracer, cornell, W, H):
    """Iterations 1 .. 5 with every optional plane on and off."""
    color, g = frame(rt, tracer, cornell, W, H)
    for n in range(1, 6):
        for albedo, emission in itertools.product((True, False), repeat=2):
            gg = pick(g, albedo, emission)
            want = rt.denoise_host(gg, color, n, *SIGMAS)
            same(tracer.denoise(gg, color, n, *SIGMAS), want, (W, H, n, albedo, emission))
            if n == 3 and albedo and emission:
                ok = R.classify(color, g["normal"], g["point"], g["emission"])
                assert (~R.same_bits(want[ok][:, :3], color[ok][:, :3])).mean() > 0.9   # (the filter did something)
                same(want[~ok], color[~ok], "copied through")
    # eight passes (steps up to 128, beyond the frame), an infinite sigma_color, and out = color
    same(tracer.denoise(g, color, 8, *SIGMAS), rt.denoise_host(g, color, 8, *SIGMAS), (W, H, 8))
    inf = (np.inf, 0.3, 1.0)
    same(tracer.denoise(g, color, 3, *inf), rt.denoise_host(g, color, 3, *inf), (W, H, "sigma_color = inf"))
    buf = color.copy()
    assert tracer.denoise(g, buf, 3, *SIGMAS, out=buf) is buf
    same(buf, rt.denoise_host(g, color, 3, *SIGMAS), (W, H, "out is color"))


@pytest.mark.parametrize("W,H", SMALL)
def test_small_frames(rt, tracer, cornell, W, H):
    color, g = crop(rt, tracer, cornell, W, H)
    if W * H > 1:
        ok = R.classify(color, g["normal"], g["point"], g["emission"])
        assert ok.any() and not ok.all(), (W, H)
    for n in (1, 2, 5):
        for emission in (True, False):
            gg = pick(g, True, emission)
            same(tracer.denoise(gg, color, n, *SIGMAS), rt.denoise_host(gg, color, n, *SIGMAS), (W, H, n, emission))


def test_synthetic_frame(rt, tracer):
    """The 24x16 frame of the CPU tests, built to meet every rule (NaN, infinity, tiny and negative albedo)."""
    c = R.synthetic_case()
    g = {k: c[k] for k in CHANNELS}
    for n in range(1, 6):
        same(tracer.denoise(g, c["color"], n, *SIGMAS), rt.denoise_host(g, c["color"], n, *SIGMAS), n)


def test_no_side_effects(rt, tracer, cornell):
    """A render sequence with denoise calls between its frames: the image, rt_get_stats and the launch words as without."""
    color, g = frame(rt, tracer, cornell, 67, 45)

    def run(denoise, frame_ahead):
        tracer.set_option("frame_ahead", frame_ahead)
        tracer.load_scene(cornell)
        tracer.reset_timing()
        for f in range(12):
            tracer.render(rt.make_params(64, 48, 3, 2, skybox=1, frames=f))
            if denoise:
                tracer.denoise(g, color, 1 + f % 3)
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


def _raw(t, planes, W, H, flags=A.DENOISE_HOST_MEMORY, **over):
    d = A.DenoiseDesc(struct_bytes=C.sizeof(A.DenoiseDesc), width=W, height=H, iterations=2, sigma_color=4.0, sigma_normal=0.3,
                      sigma_point=1.0)
    for k, v in planes.items():
        setattr(d, k, v.ctypes.data)
    for k, v in over.items():
        setattr(d, k, v)
    return t._L.rt_denoise(t._h, C.byref(d), flags)


def _planes(W, H):
    rng = np.random.default_rng(7)
    p = {"color": rng.uniform(0, 2, (H, W, 4)), "normal": np.tile([0.0, 0.0, 1.0], (H, W, 1)), "point": rng.uniform(0, 1, (H, W, 3)),
         "albedo": rng.uniform(0.2, 1, (H, W, 4)), "emission": np.zeros((H, W, 4))}
    p = {k: np.ascontiguousarray(v, F32) for k, v in p.items()}
    p["out"] = np.full((H, W, 4), F32(-7.25))
    return p


def test_scratch_is_counted_and_capped(rt):
    """64 bytes per texel held after the first call (rt_last_launch out[4]); a cap that has no room for them:
    RT_ERR_OUT_OF_MEMORY, `out` untouched; no scene is needed."""
    t = rt.RayTracer(device=0, max_width=16, max_height=16)
    try:
        W, H = 512, 256
        p = _planes(W, H)
        before = t.last_launch()["device_mb_held"]
        t.set_option("max_device_mb", before + 4)    # the scratch alone is 8 MiB
        assert _raw(t, p, W, H) == -8 and b"max_device_mb" in t._L.rt_last_error(t._h)
        assert np.all(p["out"] == F32(-7.25))
        assert t.last_launch()["device_mb_held"] == before
        t.set_option("max_device_mb", 0)
        assert _raw(t, p, W, H) == 0
        want = rt.denoise_host({k: p[k] for k in CHANNELS}, p["color"], 2, *SIGMAS)
        same(p["out"], want, "512x256")
        assert t.last_launch()["device_mb_held"] == before + 8
        small = _planes(8, 8)                          # a smaller frame reuses the scratch
        assert _raw(t, small, 8, 8) == 0
        assert t.last_launch()["device_mb_held"] == before + 8
        t.set_option("max_device_mb", before + 8)     # the scratch is held already, but the staging planes need room too
        assert _raw(t, p, W, H) == -8 and b"max_device_mb" in t._L.rt_last_error(t._h)
    finally:
        t.close()


def test_errors(rt):
    """The argument errors on the device entry point, the device-only ones included; `out` stays as it was."""
    t = rt.RayTracer(device=0, max_width=16, max_height=16)
    L, h = t._L, t._h
    W, H = 8, 6

    def err():
        return L.rt_last_error(h).decode()

    try:
        p = _planes(W, H)
        d = A.DenoiseDesc(struct_bytes=C.sizeof(A.DenoiseDesc))
        assert L.rt_denoise(None, C.byref(d), 1) == -1
        assert L.rt_denoise(h, None, 1) == -1 and "null" in err()
        assert _raw(t, p, W, H, flags=3) == -1 and "flags" in err()
        assert _raw(t, p, W, H, flags=-2) == -1 and "flags" in err()
        for over, text in ((dict(struct_bytes=72), "struct_bytes"), (dict(_p0=1), "_p0"), (dict(width=0), "zero"), (dict(height=0), "zero"),
                           (dict(iterations=0), "iterations"), (dict(iterations=9), "iterations"), (dict(sigma_color=0.0), "sigma"),
                           (dict(sigma_normal=float("nan")), "sigma"), (dict(sigma_normal=float("inf")), "finite"),
                           (dict(sigma_point=float("inf")), "finite"), (dict(sigma_point=-1.0), "sigma"), (dict(normal=None), "null"),
                           (dict(point=None), "null"), (dict(out=None), "null")):
            for flags in (0, 1):
                assert _raw(t, p, W, H, flags=flags, **over) == -1 and text in err(), (over, flags, err())
        # a NULL colour with the host flag (without it, it names the image: tests/_denoise_device_path.py)
        assert _raw(t, p, W, H, flags=1, color=None) == -1 and "color" in err()
        assert _raw(t, p, 1 << 16, 1 << 15) == -2 and "2^31" in err()
        # device planes (host arrays' addresses stand in for device pointers: the checks come before any use)
        assert all(v.ctypes.data % 16 == 0 for v in p.values())
        need = {"color": 16, "normal": 4, "point": 4, "albedo": 16, "emission": 16, "out": 16}
        for c, a in need.items():
            for off in (1, 2, 4, 8):
                if off % a:
                    assert _raw(t, p, W, H, flags=0, **{c: p[c].ctypes.data + off}) == -1 and f"plane {c} " in err() and "aligned" in err(), (c, off)
        # a NULL colour names the image: 16 x 16 texels here
        assert _raw(t, p, 17, 16, flags=0, color=None) == -2 and "image" in err()
        assert _raw(t, p, 256, 2, flags=0, color=None) == -2 and "image" in err()
        assert np.all(p["out"] == F32(-7.25))
        assert _raw(t, p, W, H) == 0 and not np.any(p["out"] == F32(-7.25))
    finally:
        t.close()


def test_device_path():
    """Torch tensors on the device (tests/_denoise_device_path.py, a process of its own that imports torch first)."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "_denoise_device_path.py")],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "device path ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
