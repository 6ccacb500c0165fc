"""rt_temporal_rectify (include/rt_abi.h; csrc/rt_rectify.hip) against rt_temporal_rectify_host, bit for bit, on planes the
handle rendered and on the CPU tests' synthetic and small frames, through the host-memory path; the header's consequences 1
and 2 on the device; then side effects, the staging buffer's cap and the errors.  The device path (torch tensors, a NULL
colour for the handle's image, outputs in place) runs in a process of its own: tests/_rectify_device_path.py."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import _rectify_reference as R
import _temporal_deform_reference as TD
import _temporal_motion_reference as TM
import _temporal_reference as T
from ray_tracer_2_amd import _abi as A

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = float("inf")
# both are wider than a tile of 32 x 8 in both axes, with partial tiles at both seams: the halo crosses tile seams
SIZES = [(67, 45), (66, 36)]
# 33 x 9: one texel past a tile in each axis
SMALL = [(1, 1), (8, 1), (1, 8), (33, 9)]
CHANNELS = ("point", "normal", "object", "albedo")
MARK = F32(-7.25)
OUTPUTS = ("out", "out_history", "out_moments", "out_clipped")

_frames = {}


def frames(rt, tracer, cornell, W, H):
    """Two 8 spp / 4 bounce frames of different seeds (the history and the new frame), a history length per texel, the object
    plane and the luminance moments of both frames, rendered once per size."""
    if (W, H) not in _frames:
        tracer.load_scene(cornell)
        g = tracer.render_gbuffer(rt.make_params(W, H, 1, 1), CHANNELS)
        hit = (g["normal"] != 0).any(-1)
        assert 0.3 < hit.mean() < 1.0 and np.array_equal(hit, g["object"] != A.MISS), (W, H)
        img = []
        for fr in (0, -1):
            tracer.render(rt.make_params(W, H, 4, 8, skybox=1, frames=fr))
            img.append(tracer.read_image(W, H).copy())
        length = np.random.default_rng(W).integers(1, 9, (H, W)).astype(F32)
        _frames[(W, H)] = dict(color=img[1], history=img[0], history_length=length, object=g["object"],
                               moments=tracer.luminance_moments(g, img[1]), history_moments=tracer.luminance_moments(g, img[0]))
    return _frames[(W, H)]


def both(rt, tracer, kw, what="", **par):
    """The device (host-memory path) against the host, with and without out_clipped; returns the device's outputs as (out,
    out_history, out_moments or None, out_clipped)."""
    want = rt.temporal_rectify_host(**kw, **par, clipped=True)
    got = tracer.temporal_rectify(**kw, **par, clipped=True)
    assert len(got) == len(want) == (4 if "moments" in kw else 3), what
    for a, b, name in zip(got[:-1], want[:-1], OUTPUTS):
        bad = ~R.same_bits(a, b)
        assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert got[-1].dtype == np.uint8 and np.array_equal(got[-1], want[-1]), (what, "out_clipped", np.argwhere(got[-1] != want[-1])[:4].tolist())
    alone = tracer.temporal_rectify(**kw, **par)
    assert len(alone) == len(want) - 1 and all(R.same_bits(a, b).all() for a, b in zip(alone, want)), (what, "without out_clipped")
    return (got[0], got[1], got[2] if "moments" in kw else None, got[-1])


@pytest.mark.parametrize("W,H", SIZES)
def test_device_equals_host(rt, tracer, cornell, W, H):
    planes = frames(rt, tracer, cornell, W, H)
    for (name, kw), radius in itertools.product(R.variants(planes), (1, 2, 3)):
        for sigma, keep in ((1.0, 4.0), (0.25, 1.0)):
            out, hist, _, clip = both(rt, tracer, kw, (W, H, name, radius, sigma), radius=radius, clip_sigma=sigma, clip_history=keep)
        assert (clip == R.CLIPPED).mean() > 0.05 and (clip == R.KEPT).any() and out.shape == (H, W, 4), (W, H, name, radius)
    # in place: the outputs are the history planes
    kw = dict(R.variants(planes))["all"]
    want = rt.temporal_rectify_host(**kw)
    bufs = [planes[k].copy() for k in ("history", "history_length", "history_moments")]
    got = tracer.temporal_rectify(**dict(kw, history=bufs[0], history_length=bufs[1], history_moments=bufs[2]), out=bufs[0],
                                  out_history=bufs[1], out_moments=bufs[2])
    assert all(a is b for a, b in zip(got, bufs)) and all(R.same_bits(a, b).all() for a, b in zip(got, want)), (W, H, "in place")


def test_synthetic_frame(rt, tracer):
    """The 40x20 frame of the CPU tests, built to meet every rule, at every radius and the three kinds of clip_sigma."""
    planes, _ = R.synthetic_case()
    for (name, kw), radius, sigma in itertools.product(R.variants(planes), (1, 2, 3), (0.0, 1.0, INF)):
        both(rt, tracer, kw, ("synthetic", name, radius, sigma), radius=radius, clip_sigma=sigma, clip_history=4.0)
    kw = dict(R.variants(planes))["all"]
    for keep in (1.0, INF):
        both(rt, tracer, kw, ("synthetic", keep), clip_history=keep)


@pytest.mark.parametrize("W,H", SMALL)
def test_small_frames(rt, tracer, W, H):
    planes = R.small_case(W, H)
    for (name, kw), radius in itertools.product(R.variants(planes), (1, 2, 3)):
        both(rt, tracer, kw, (W, H, name, radius), radius=radius, clip_sigma=0.5, clip_history=2.0)


def _cases():
    planes, cam, _ = T.synthetic_case()
    split = lambda p: ({k: p[k] for k in ("point", "normal", "object")}, {k[5:]: p[k] for k in ("prev_point", "prev_normal", "prev_object")})  # noqa: E731
    yield "plain", planes, (*split(planes), cam), {}
    planes, cam, motions, _ = TM.synthetic_case()
    yield "moving", planes, (*split(planes), cam), dict(motions=motions)
    planes, cam, motions, tris, _ = TD.synthetic_case()
    yield "deforming", planes, (*TD.split(planes), cam), dict(motions=motions, prev_triangles=tris, tri_first=TD.TRI_FIRST)


def test_infinite_sigma_is_temporal_accumulation(rt, tracer):
    """Consequence 1 on the device, for the three forms, each with a camera move: temporal_reproject then temporal_rectify at
    clip_sigma = +INF against temporal_accumulate itself; and the reprojection against the host's."""
    for what, planes, guides, kw in _cases():
        args = (*guides, planes["prev_color"], planes["prev_history"])
        for cap in (4.0, INF):
            want = tracer.temporal_accumulate(*args, planes["color"], cap, **kw)
            h, n = tracer.temporal_reproject(*args, cap, **kw)
            hh, hn = rt.temporal_reproject_host(*args, cap, **kw)
            assert R.same_bits(h, hh).all() and R.same_bits(n, hn).all(), (what, "reprojection")
            assert np.isnan(h).all(-1).any() and (n > 1).any() and (~np.isfinite(planes["color"])).any(), what
            for radius, obj in ((3, planes["object"]), (1, None)):
                got = tracer.temporal_rectify(planes["color"], h, n, object=obj, radius=radius, clip_sigma=INF, clip_history=1.0)
                for a, b, name in zip(got, want, OUTPUTS):
                    bad = ~R.same_bits(a, b)
                    assert not bad.any(), (what, cap, radius, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def test_unmoved_camera_is_rt_renders_accumulation(rt, tracer, cornell):
    """Consequence 2: frames = 0 .. 3 on one handle; on a second one the raw samples of frames = -k through temporal_reproject
    and temporal_rectify (clip_sigma = +INF) under the same camera and G-buffer: the first handle's image, bit for bit, on
    every hit texel.  With the default clip_sigma the texels that were not clipped hold those bits too (consequence 4)."""
    W, H = 67, 45
    cam = cornell.uniform.camera
    tracer.load_scene(cornell)
    other = rt.RayTracer(device=0, max_width=W, max_height=H)
    try:
        other.load_scene(cornell)
        g = other.render_gbuffer(rt.make_params(W, H, 1, 1), ("point", "normal", "object"))
        hit = (g["normal"] != 0).any(-1)
        assert 0.5 < hit.mean() < 1.0
        tracer.render(rt.make_params(W, H, 4, 8, skybox=1, frames=0))
        mine, length = tracer.read_image(W, H).copy(), np.ones((H, W), F32)
        for k in range(1, 4):
            tracer.render(rt.make_params(W, H, 4, 8, skybox=1, frames=k))
            acc = tracer.read_image(W, H).copy()
            other.render(rt.make_params(W, H, 4, 8, skybox=1, frames=-k))
            raw = other.read_image(W, H).copy()
            h, n = other.temporal_reproject(g, g, cam, mine, length)
            out, hist, clip = other.temporal_rectify(raw, h, n, object=g["object"], clipped=True)
            kept = hit & (clip == R.KEPT)
            assert kept.any() and (hit & (clip == R.CLIPPED)).any() and R.same_bits(out[kept], acc[kept]).all(), k
            mine, length = other.temporal_rectify(raw, h, n, object=g["object"], clip_sigma=INF)
            assert R.same_bits(mine[hit], acc[hit]).all() and (length[hit] == k + 1).all(), k
            assert R.same_bits(mine[~hit], raw[~hit]).all() and (length[~hit] == 1).all(), k
    finally:
        other.close()


def test_no_side_effects(rt, tracer, cornell):
    """A render sequence with temporal_rectify calls between its frames: the image, rt_get_stats and the launch words as
    without."""
    planes = frames(rt, tracer, cornell, 67, 45)
    kw = dict(R.variants(planes))["all"]

    def run(rectify, frame_ahead):
        tracer.set_option("frame_ahead", frame_ahead)
        tracer.load_scene(cornell)
        tracer.reset_timing()
        for fr in range(12):
            tracer.render(rt.make_params(64, 48, 3, 2, skybox=1, frames=fr))
            if rectify:
                tracer.temporal_rectify(**kw, radius=1 + fr % 3, clipped=bool(fr & 1))
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


def _planes(W, H):
    rng = np.random.default_rng(7)
    f = lambda *s: rng.uniform(0.5, 2, s).astype(F32)   # noqa: E731
    return dict(color=f(H, W, 4), history=f(H, W, 4), history_length=np.full((H, W), 3, F32), object=np.ones((H, W), np.uint32),
                moments=f(H, W, 4), history_moments=f(H, W, 4), out=np.full((H, W, 4), MARK), out_history=np.full((H, W), MARK),
                out_moments=np.full((H, W, 4), MARK), out_clipped=np.full((H, W), 0xA5, np.uint8))


def _raw(t, p, W, H, flags=A.RECTIFY_HOST_MEMORY, **over):
    d = A.RectifyDesc(struct_bytes=C.sizeof(A.RectifyDesc), width=W, height=H, radius=3, clip_sigma=1.0, clip_history=4.0)
    for k, v in p.items():
        setattr(d, k, v.ctypes.data)
    for k, v in over.items():
        setattr(d, k, v)
    return t._L.rt_temporal_rectify(t._h, C.byref(d), flags)


def _untouched(p):
    return bool(all(np.all(p[k] == MARK) for k in OUTPUTS[:3]) and np.all(p["out_clipped"] == 0xA5))


def _same_as_host(rt, p):
    want = rt.temporal_rectify_host(p["color"], p["history"], p["history_length"], p["object"], moments=p["moments"],
                                    history_moments=p["history_moments"], clipped=True)
    return all(R.same_bits(p[k], w).all() for k, w in zip(OUTPUTS[:3], want)) and np.array_equal(p["out_clipped"], want[3])


def test_staging_is_capped_and_nothing_is_kept(rt):
    """The host-memory path stages 73 bytes per texel with every plane (9.2 MiB for 512x256): a cap that has no room for them
    gives RT_ERR_OUT_OF_MEMORY with the outputs untouched; with room the call holds nothing afterwards; no scene is needed."""
    t = rt.RayTracer(device=0, max_width=16, max_height=16)
    try:
        W, H = 512, 256
        p = _planes(W, H)
        before = t.last_launch()["device_mb_held"]
        t.set_option("max_device_mb", before + 4)
        assert _raw(t, p, W, H) == -8 and b"max_device_mb" in t._L.rt_last_error(t._h)
        assert _untouched(p)
        assert t.last_launch()["device_mb_held"] == before
        t.set_option("max_device_mb", before + 11)
        assert _raw(t, p, W, H) == 0
        assert _same_as_host(rt, p)
        assert t.last_launch()["device_mb_held"] == before
        t.set_option("max_device_mb", 0)
        q = _planes(W, H)
        assert _raw(t, q, W, H) == 0 and R.same_bits(q["out"], p["out"]).all()
    finally:
        t.close()


def test_errors(rt):
    """The argument errors on the device entry point, the device-only ones included; the outputs stay as they were."""
    t = rt.RayTracer(device=0, max_width=16, max_height=16)
    L, hd = t._L, t._h
    W, H = 9, 7

    def err():
        return L.rt_last_error(hd).decode()

    try:
        p = _planes(W, H)
        d = A.RectifyDesc(struct_bytes=C.sizeof(A.RectifyDesc))
        assert L.rt_temporal_rectify(None, C.byref(d), 1) == -1
        assert L.rt_temporal_rectify(hd, None, 1) == -1 and "null" in err()
        assert _raw(t, p, W, H, flags=3) == -1 and "flags" in err()
        assert _raw(t, p, W, H, flags=-2) == -1 and "flags" in err()
        nan = float("nan")
        for over, text in ((dict(struct_bytes=104), "struct_bytes"), (dict(_p0=1), "_p0"), (dict(_p1=1), "_p1"), (dict(width=0), "zero"),
                           (dict(height=0), "zero"), (dict(radius=0), "radius"), (dict(radius=4), "radius"),
                           (dict(clip_sigma=-1.0), "clip_sigma"), (dict(clip_sigma=nan), "clip_sigma"),
                           (dict(clip_history=0.5), "clip_history"), (dict(clip_history=nan), "clip_history"),
                           (dict(history=None), "null"), (dict(history_length=None), "null"), (dict(out=None), "null"),
                           (dict(out_history=None), "null"), (dict(moments=None), "moments"), (dict(history_moments=None), "moments"),
                           (dict(out_moments=None), "moments"), (dict(out=p["color"].ctypes.data), "overlaps"),
                           (dict(out=p["color"].ctypes.data + 16 * (W * H - 1)), "overlaps")):
            for flags in (0, 1):
                assert _raw(t, p, W, H, flags=flags, **over) == -1 and text in err(), (over, flags, err())
        # a NULL color with the host flag (without it, it names the image: tests/_rectify_device_path.py)
        assert _raw(t, p, W, H, flags=1, color=None) == -1 and "color" in err()
        assert _raw(t, p, 1 << 16, 1 << 15) == -2 and "2^31" in err()
        # device planes (host arrays' addresses stand in for device pointers: the checks come before any use)
        assert all(v.ctypes.data % 16 == 0 for v in p.values())
        need = {"color": 16, "history": 16, "history_length": 4, "object": 4, "moments": 16, "history_moments": 16, "out": 16,
                "out_history": 4, "out_moments": 16, "out_clipped": 1}
        assert list(need) == list(A.RECTIFY_PLANES)
        for c, a in need.items():
            for off in (1, 2, 4, 8):
                if off % a:
                    assert _raw(t, p, W, H, flags=0, **{c: p[c].ctypes.data + off}) == -1 and f"plane {c} " in err() and "aligned" in err(), (c, off)
        # a NULL color names the image: 16 x 16 texels here; an `out` inside the texels it reads is refused
        assert _raw(t, p, 17, 16, flags=0, color=None) == -2 and "image" in err()
        assert _raw(t, p, 256, 2, flags=0, color=None) == -2 and "image" in err()
        image = L.rt_device_image(hd)
        for off in (0, 16 * (W * H - 1)):
            assert _raw(t, p, W, H, flags=0, color=None, out=image + off) == -1 and "overlaps the image" in err(), off
        assert _untouched(p)
        assert _raw(t, p, W, H) == 0 and not any(np.any(p[k] == MARK) for k in OUTPUTS[:3]) and not np.any(p["out_clipped"] == 0xA5)
        assert _same_as_host(rt, p)
    finally:
        t.close()


def test_device_path():
    """Torch tensors on the device (tests/_rectify_device_path.py, a process of its own that imports torch first)."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "_rectify_device_path.py")],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "device path ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
