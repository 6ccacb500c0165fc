"""rt_upsample (include/rt_abi.h; csrc/rt_upsample.hip) against rt_upsample_host, bit for bit, on planes the handle rendered
-- rt_render at the low size, render_gbuffer at both -- and on the CPU tests' synthetic pairs, through the host-memory path;
the header's two consequences; then side effects, the staging buffer's cap and the errors.  The device path (torch tensors, a
NULL lo_color for the handle's image) runs in a process of its own: tests/_upsample_device_path.py."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import _upsample_reference as R
from ray_tracer_2_amd import _abi as A

pytestmark = pytest.mark.gpu

F32 = np.float32
# 66x36 -> 130x70 is wider than any tile in both axes (tiles are 32x8 high texels): the tiles' low footprints meet at seams;
# 67x45 -> 34x23 reaches further than a workgroup stages, 24x16 -> 24x16 is the ratio at which it stages the most
SIZES = [(34, 23, 67, 45), (24, 16, 61, 37), (66, 36, 130, 70), (67, 45, 34, 23), (24, 16, 24, 16)]
SMALL = [(1, 1, 8, 8), (8, 1, 1, 8)]
CHANNELS = ("depth", "point", "normal", "object", "albedo", "emission")
MARK = F32(-7.25)

_frames = {}


def gbuffer(rt, tracer, cornell, W, H):
    if ("g", W, H) not in _frames:
        tracer.load_scene(cornell)
        g = tracer.render_gbuffer(rt.make_params(W, H, 1, 1), CHANNELS)
        hit = (g["normal"] != 0).any(-1)
        assert 0.3 < hit.mean() < 1.0 and np.array_equal(hit, g["object"] != A.MISS), (W, H)
        _frames[("g", W, H)] = g
    return _frames[("g", W, H)]


def frames(rt, tracer, cornell, w, h, W, H):
    """One 8 spp / 4 bounce frame at w x h and the guides of both sizes, rendered once per size."""
    if ("c", w, h) not in _frames:
        tracer.load_scene(cornell)
        tracer.render(rt.make_params(w, h, 4, 8, skybox=1, frames=0))
        _frames[("c", w, h)] = tracer.read_image(w, h).copy()
    lo = R.without(gbuffer(rt, tracer, cornell, w, h), "depth", "emission")
    return dict(lo, color=_frames[("c", w, h)]), gbuffer(rt, tracer, cornell, W, H)


def variants(lo, hi):
    """The optional planes on and off."""
    yield "all", lo, hi
    yield "no emission", lo, R.without(hi, "emission")
    yield "no albedo", R.without(lo, "albedo"), R.without(hi, "albedo")
    yield "neither", R.without(lo, "albedo"), R.without(hi, "albedo", "emission")


def both(rt, tracer, lo, hi, what="", **kw):
    """The device (host-memory path) against the host, with and without `coverage`; returns the device's (out, coverage)."""
    guides = R.without(lo, "color")
    want = rt.upsample_host(guides, hi, lo["color"], coverage=True, **kw)
    got = tracer.upsample(guides, hi, lo["color"], coverage=True, **kw)
    bad = ~R.same_bits(got[0], want[0])
    assert not bad.any(), (what, "out", int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert got[1].dtype == np.uint8 and np.array_equal(got[1], want[1]), (what, "coverage", np.argwhere(got[1] != want[1])[:4].tolist())
    alone = tracer.upsample(guides, hi, lo["color"], **kw)
    assert isinstance(alone, np.ndarray) and R.same_bits(alone, want[0]).all(), (what, "without coverage")
    return got


@pytest.mark.parametrize("w,h,W,H", SIZES)
def test_device_equals_host(rt, tracer, cornell, w, h, W, H):
    lo, hi = frames(rt, tracer, cornell, w, h, W, H)
    for name, l, hh in variants(lo, hi):
        for tol, ncos in ((0.02, 0.9), (0.002, 0.999)):
            out, cov = both(rt, tracer, l, hh, (w, h, W, H, name, tol), point_tolerance=tol, normal_cos=ncos)
        assert (cov == 2).mean() > 0.5 and out.shape == (H, W, 4)
    if W > w:
        assert (cov < 2).any(), (w, h, W, H)   # (thin silhouettes the low frame missed: ring 2 or holes)


@pytest.mark.parametrize("w,h,W,H", SMALL + [(24, 16, 61, 37), (67, 45, 34, 23)])
def test_procedural_frames(rt, tracer, w, h, W, H):
    """The CPU tests' procedural pairs: frames of one row, one column and one texel among them."""
    lo, hi = R.pair(w, h, W, H)
    for name, l, hh in variants(lo, hi):
        both(rt, tracer, l, hh, (w, h, W, H, name))


def test_synthetic_frames(rt, tracer):
    """The pairs of the CPU tests built to meet every rule (each refusal, ring 2, holes, PLAIN texels, NaN and infinity, the
    albedo floor, both snap thresholds)."""
    lo, hi, _ = R.synthetic_case()
    for name, l, hh in variants(lo, hi):
        out, cov = both(rt, tracer, l, hh, ("synthetic", name))
        assert (cov == 1).any() and (cov == 0).any()
    for name, l, hh in variants(*R.snap_case()):
        both(rt, tracer, l, hh, ("snap", name))


def test_equal_sizes_copy_the_colour(rt, tracer, cornell):
    """Consequence 1 on the handle's own planes: the low planes are the high planes, no albedo planes."""
    W, H = 67, 45
    lo, _ = frames(rt, tracer, cornell, W, H, W, H)
    g = R.without(gbuffer(rt, tracer, cornell, W, H), "albedo")
    color = lo["color"]
    assert np.isfinite(color).all()
    for guides, ncos in itertools.product((g, R.without(g, "emission")), (0.99, 0.9)):
        out, cov = tracer.upsample(R.without(guides, "depth", "emission"), guides, color, normal_cos=ncos, coverage=True)
        assert R.same_bits(out, color).all() and (cov == 2).all(), ncos


def test_even_texels_of_a_doubled_frame_are_the_low_texels(rt, tracer, cornell):
    """Consequence 2 through the host-memory path (with a NULL lo_color, the handle's image: tests/_upsample_device_path.py)."""
    lo, hi = frames(rt, tracer, cornell, 34, 23, 67, 45)
    out, cov = tracer.upsample(R.without(lo, "color", "albedo"), R.without(hi, "albedo"), lo["color"], coverage=True)
    assert np.isfinite(lo["color"]).all()
    assert R.same_bits(out[::2, ::2], lo["color"]).all() and (cov[::2, ::2] == 2).all()


def test_no_side_effects(rt, tracer, cornell):
    """A render sequence with upsample calls between its frames: the image, rt_get_stats and the launch words as without."""
    lo, hi = frames(rt, tracer, cornell, 34, 23, 67, 45)
    guides = R.without(lo, "color")

    def run(upsample, frame_ahead):
        tracer.set_option("frame_ahead", frame_ahead)
        tracer.load_scene(cornell)
        tracer.reset_timing()
        for fr in range(12):
            tracer.render(rt.make_params(64, 48, 3, 2, skybox=1, frames=fr))
            if upsample:
                tracer.upsample(guides, hi, lo["color"], coverage=bool(fr & 1))
            else:
                tracer.synchronize()   # (a host-path call returns when its data is on the host: the other sequence waits too)
        img = tracer.read_image(64, 48)
        s = tracer.stats()
        return img, (s.segments, s.paths, s.node_tests, s.triangle_tests, s.frames, s.segments_reused, s.frames_speculative), \
            tuple(tracer.last_launch().values())

    try:
        for fa in (-1, 8):
            a, sa, la = run(False, fa)
            b, sb, lb = run(True, fa)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), fa
            # (the automatic policy renders ahead by what it finds on the stream: only the frames asked for are schedule-free)
            assert (sa == sb) if fa > 0 else (sa[4] == sb[4]), (fa, sa, sb)
            if fa > 0:
                assert la == lb, (la, lb)   # (device_mb_held included: the call keeps no scratch)
    finally:
        tracer.set_option("frame_ahead", -1)


def _planes(w, h, W, H):
    rng = np.random.default_rng(7)
    f = lambda *s: rng.uniform(0.5, 2, s).astype(F32)   # noqa: E731
    p = dict(lo_color=f(h, w, 4), lo_point=f(h, w, 3), lo_normal=f(h, w, 3), lo_object=np.ones((h, w), np.uint32), lo_albedo=f(h, w, 4),
             depth=f(H, W), point=f(H, W, 3), normal=f(H, W, 3), object=np.ones((H, W), np.uint32), albedo=f(H, W, 4),
             emission=np.zeros((H, W, 4), F32), out=np.full((H, W, 4), MARK), coverage=np.full((H, W), 0xA5, np.uint8))
    p["lo_normal"][:] = p["normal"][:] = (0, 0, -1)
    p["lo_point"][:] = p["point"][:] = (0, 0, 3)
    return p


def _raw(t, p, w, h, W, H, flags=A.UPSAMPLE_HOST_MEMORY, **over):
    d = A.UpsampleDesc(struct_bytes=C.sizeof(A.UpsampleDesc), lo_width=w, lo_height=h, width=W, height=H, point_tolerance=0.02, normal_cos=0.9)
    for k, v in p.items():
        setattr(d, k, v.ctypes.data)
    for k, v in over.items():
        setattr(d, k, v)
    return t._L.rt_upsample(t._h, C.byref(d), flags)


def _untouched(p):
    return bool(np.all(p["out"] == MARK) and np.all(p["coverage"] == 0xA5))


def _host_of(rt, p):
    lo = {k[3:]: p[k] for k in ("lo_point", "lo_normal", "lo_object", "lo_albedo")}
    hi = {k: p[k] for k in ("depth", "point", "normal", "object", "albedo", "emission")}
    return rt.upsample_host(lo, hi, p["lo_color"], coverage=True)


def test_staging_is_capped_and_nothing_is_kept(rt):
    """The host-memory path stages 60 bytes per low texel and 81 per high texel with every plane (12 MiB for 256x128 ->
    512x256): a cap that has no room for them gives RT_ERR_OUT_OF_MEMORY with the outputs untouched; with room the call holds
    nothing afterwards; no scene is needed."""
    t = rt.RayTracer(device=0, max_width=16, max_height=16)
    try:
        w, h, W, H = 256, 128, 512, 256
        p = _planes(w, h, W, H)
        before = t.last_launch()["device_mb_held"]
        t.set_option("max_device_mb", before + 4)
        assert _raw(t, p, w, h, W, H) == -8 and b"max_device_mb" in t._L.rt_last_error(t._h)
        assert _untouched(p)
        assert t.last_launch()["device_mb_held"] == before
        t.set_option("max_device_mb", before + 14)
        assert _raw(t, p, w, h, W, H) == 0
        want = _host_of(rt, p)
        assert R.same_bits(p["out"], want[0]).all() and np.array_equal(p["coverage"], want[1])
        assert t.last_launch()["device_mb_held"] == before
        t.set_option("max_device_mb", 0)
        q = _planes(w, h, W, H)
        assert _raw(t, q, w, h, W, H) == 0 and R.same_bits(q["out"], p["out"]).all()
    finally:
        t.close()


def test_errors(rt):
    """The argument errors on the device entry point, the device-only ones included; the outputs stay as they were."""
    t = rt.RayTracer(device=0, max_width=16, max_height=16)
    L, hd = t._L, t._h
    w, h, W, H = 5, 4, 9, 7

    def err():
        return L.rt_last_error(hd).decode()

    try:
        p = _planes(w, h, W, H)
        d = A.UpsampleDesc(struct_bytes=C.sizeof(A.UpsampleDesc))
        assert L.rt_upsample(None, C.byref(d), 1) == -1
        assert L.rt_upsample(hd, None, 1) == -1 and "null" in err()
        assert _raw(t, p, w, h, W, H, flags=3) == -1 and "flags" in err()
        assert _raw(t, p, w, h, W, H, flags=-2) == -1 and "flags" in err()
        nan, inf = float("nan"), float("inf")
        for over, text in ((dict(struct_bytes=128), "struct_bytes"), (dict(_p0=1), "_p0"), (dict(lo_width=0), "zero"), (dict(lo_height=0), "zero"),
                           (dict(width=0), "zero"), (dict(height=0), "zero"),
                           (dict(point_tolerance=0.0), "point_tolerance"), (dict(point_tolerance=nan), "point_tolerance"),
                           (dict(point_tolerance=inf), "point_tolerance"), (dict(point_tolerance=-1.0), "point_tolerance"),
                           (dict(normal_cos=nan), "normal_cos"), (dict(normal_cos=1.5), "normal_cos"), (dict(normal_cos=-1.5), "normal_cos"),
                           (dict(lo_point=None), "null"), (dict(lo_normal=None), "null"), (dict(lo_object=None), "null"),
                           (dict(depth=None), "null"), (dict(point=None), "null"), (dict(normal=None), "null"), (dict(object=None), "null"),
                           (dict(out=None), "null"), (dict(albedo=None), "albedo"), (dict(lo_albedo=None), "albedo")):
            for flags in (0, 1):
                assert _raw(t, p, w, h, W, H, flags=flags, **over) == -1 and text in err(), (over, flags, err())
        # a NULL lo_color with the host flag (without it, it names the image: tests/_upsample_device_path.py)
        assert _raw(t, p, w, h, W, H, flags=1, lo_color=None) == -1 and "lo_color" in err()
        assert _raw(t, p, 1 << 16, 1 << 15, W, H) == -2 and "2^31" in err()
        assert _raw(t, p, w, h, 1 << 16, 1 << 15) == -2 and "2^31" in err()
        # device planes (host arrays' addresses stand in for device pointers: the checks come before any use)
        assert all(v.ctypes.data % 16 == 0 for v in p.values())
        need = {"lo_color": 16, "lo_point": 4, "lo_normal": 4, "lo_object": 4, "lo_albedo": 16, "depth": 4, "point": 4, "normal": 4,
                "object": 4, "albedo": 16, "emission": 16, "out": 16, "coverage": 1}
        assert list(need) == list(A.UPSAMPLE_PLANES)
        for c, a in need.items():
            for off in (1, 2, 4, 8):
                if off % a:
                    assert _raw(t, p, w, h, W, H, flags=0, **{c: p[c].ctypes.data + off}) == -1 and f"plane {c} " in err() and "aligned" in err(), (c, off)
        # a NULL lo_color names the image: 16 x 16 texels here
        assert _raw(t, p, 17, 16, W, H, flags=0, lo_color=None) == -2 and "image" in err()
        assert _raw(t, p, 256, 2, W, H, flags=0, lo_color=None) == -2 and "image" in err()
        assert _untouched(p)
        assert _raw(t, p, w, h, W, H) == 0 and not np.any(p["out"] == MARK) and not np.any(p["coverage"] == 0xA5)
        want = _host_of(rt, p)
        assert R.same_bits(p["out"], want[0]).all() and np.array_equal(p["coverage"], want[1])
    finally:
        t.close()


def test_device_path():
    """Torch tensors on the device (tests/_upsample_device_path.py, a process of its own that imports torch first)."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "_upsample_device_path.py")],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "device path ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
