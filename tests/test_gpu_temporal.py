"""rt_temporal_accumulate (include/rt_abi.h; csrc/rt_temporal.hip) against rt_temporal_accumulate_host, bit for bit, on real
planes -- render_gbuffer plus a render of the Cornell fixture under two cameras -- through the host-memory path; the
unmoved camera against rt_render's own accumulation; then side effects, the staging buffer's cap and the errors.  The device
path (torch tensors, a NULL colour for the handle's image) runs in a process of its own: tests/_temporal_device_path.py."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import _temporal_reference as R
from ray_tracer_2_amd import _abi as A

pytestmark = pytest.mark.gpu

F32 = np.float32
# 130x70 is wider than any tile in both axes (tiles are 32x8): the gather crosses tile seams
SIZES = [(67, 45), (24, 16), (130, 70)]
SMALL = [(1, 1), (8, 1), (1, 8)]
CHANNELS = ("point", "normal", "object")
# the camera's moves, in world units along its own axes: a fraction of a texel at 67x45, and several texels
MOVES = {"small": dict(right=0.03, up=0.01), "large": dict(right=0.5, up=-0.12, forward=0.1)}
MARK = F32(-7.25)

_frames = {}


def frames(rt, tracer, cornell, W, H):
    """Per camera (the fixture's, and the two moved ones): one 8 spp / 4 bounce frame and its guides, rendered once per
    size; and a history length per texel."""
    if (W, H) not in _frames:
        tracer.load_scene(cornell)
        base = cornell.uniform.camera
        cams = {"base": base, **{k: R.moved_camera(base, **v) for k, v in MOVES.items()}}
        out = {}
        try:
            for name, cam in cams.items():
                tracer.set_camera(cam)
                tracer.render(rt.make_params(W, H, 4, 8, skybox=1, frames=0))
                color = tracer.read_image(W, H).copy()
                g = tracer.render_gbuffer(rt.make_params(W, H, 1, 1), CHANNELS)
                hit = (g["normal"] != 0).any(-1)
                assert 0.3 < hit.mean() < 1.0 and np.array_equal(hit, g["object"] != A.MISS), (W, H, name)
                out[name] = (cam, color, g)
        finally:
            tracer.set_camera(base)
        history = np.random.default_rng(W).integers(1, 7, (H, W)).astype(F32)
        _frames[(W, H)] = (out, history)
    return _frames[(W, H)]


def both(rt, tracer, g, pg, cam, prev_color, history, color, objects=True, what="", **kw):
    """The device (host-memory path) against the host; returns the device's outputs."""
    if not objects:
        g, pg = ({k: v for k, v in d.items() if k != "object"} for d in (g, pg))
    want = rt.temporal_accumulate_host(g, pg, cam, prev_color, history, color, **kw)
    got = tracer.temporal_accumulate(g, pg, cam, prev_color, history, color, **kw)
    assert len(got) == len(want)
    for a, b, name in zip(got, want, ("out", "out_history", "motion")):
        bad = ~R.same_bits(a, b)
        assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    return got


@pytest.mark.parametrize("W,H", SIZES)
def test_device_equals_host(rt, tracer, cornell, W, H):
    """Both moves; the object planes and motion on and off; the cap active and not; out = color."""
    f, history = frames(rt, tracer, cornell, W, H)
    pcam, prev_color, pg = f["base"]
    for move in MOVES:
        _, color, g = f[move]
        for objects, motion, cap in itertools.product((True, False), (True, False), (3.0, np.inf)):
            got = both(rt, tracer, g, pg, pcam, prev_color, history, color, objects, (W, H, move, objects, motion, cap),
                       max_history=cap, motion=motion)
            hit = (g["normal"] != 0).any(-1)
            assert (got[1][hit] > 1).mean() > 0.5 and (got[1][hit] == 1).any(), (W, H, move)   # history found, and restarts
            if cap == 3.0:
                assert got[1].max() == 4 and (history > 3).any()
            if motion:
                size = np.linalg.norm(got[2][got[1] > 1], axis=-1).mean()
                assert (size < 1.5) if move == "small" and (W, H) == (67, 45) else (size > 0.01), (W, H, move, size)
        want = rt.temporal_accumulate_host(g, pg, pcam, prev_color, history, color, 3.0)
        buf, hist = color.copy(), np.zeros((H, W), F32)
        got = tracer.temporal_accumulate(g, pg, pcam, prev_color, history, buf, 3.0, out=buf, out_history=hist)
        assert got[0] is buf and got[1] is hist
        assert R.same_bits(buf, want[0]).all() and R.same_bits(hist, want[1]).all(), (W, H, move, "out is color")


@pytest.mark.parametrize("W,H", SMALL)
def test_small_frames(rt, tracer, cornell, W, H):
    """A window of the 67x45 frames that lies on one object in both of them (a flat wall or the floor: taken as a W x H frame
    its texels still find history on that plane), and the CPU tests' wall of that size."""
    f, history = frames(rt, tracer, cornell, 67, 45)
    pcam, prev_color, pg = f["base"]
    _, color, g = f["small"]
    one = [(y, x) for y in range(45 - H + 1) for x in range(67 - W + 1)
           if g["object"][y, x] != A.MISS and (g["object"][y:y + H, x:x + W] == g["object"][y, x]).all()
           and (pg["object"][y:y + H, x:x + W] == g["object"][y, x]).all()
           and (g["normal"][y:y + H, x:x + W] == g["normal"][y, x]).all() and (pg["normal"][y:y + H, x:x + W] == g["normal"][y, x]).all()]
    assert one, (W, H)
    y, x = one[len(one) // 2]
    s = (slice(y, y + H), slice(x, x + W))
    crop = lambda d: {k: np.ascontiguousarray(v[s]) for k, v in d.items()}   # noqa: E731
    for objects, motion in itertools.product((True, False), repeat=2):
        got = both(rt, tracer, crop(g), crop(pg), pcam, np.ascontiguousarray(prev_color[s]), np.ascontiguousarray(history[s]),
                   np.ascontiguousarray(color[s]), objects, (W, H, objects, motion), max_history=3.0, motion=motion)
        assert (got[1] > 1).any(), (W, H)
    planes, cam = R.small_case(W, H)
    g = {k: planes[k] for k in CHANNELS}
    pg = {k: planes["prev_" + k] for k in CHANNELS}
    got = both(rt, tracer, g, pg, cam, planes["prev_color"], planes["prev_history"], planes["color"], True, (W, H, "wall"), motion=True)
    assert (got[1] > 1).all()


def test_synthetic_frame(rt, tracer):
    """The 24x16 pair of frames of the CPU tests, built to meet every rule (NaN, infinity, misses, edges, off screen)."""
    planes, cam, _ = R.synthetic_case()
    g = {k: planes[k] for k in CHANNELS}
    pg = {k: planes["prev_" + k] for k in CHANNELS}
    for objects, cap in itertools.product((True, False), (4.0, np.inf)):
        both(rt, tracer, g, pg, cam, planes["prev_color"], planes["prev_history"], planes["color"], objects, (objects, cap),
             max_history=cap, motion=True)


def test_unmoved_camera_is_rt_renders_accumulation(rt, tracer, cornell):
    """frames = 0 .. 3 on one handle; on a second one the raw samples of frames = -k, fed through temporal_accumulate with
    prev_history = k under the same camera and G-buffer: the first handle's image, bit for bit, on every hit texel."""
    W, H = 67, 45
    cam = cornell.uniform.camera
    tracer.load_scene(cornell)
    other = rt.RayTracer(device=0, max_width=W, max_height=H)
    try:
        other.load_scene(cornell)
        g = other.render_gbuffer(rt.make_params(W, H, 1, 1), CHANNELS)
        hit = (g["normal"] != 0).any(-1)
        assert 0.5 < hit.mean() < 1.0
        tracer.render(rt.make_params(W, H, 4, 8, skybox=1, frames=0))
        mine = tracer.read_image(W, H).copy()
        for k in range(1, 4):
            tracer.render(rt.make_params(W, H, 4, 8, skybox=1, frames=k))
            acc = tracer.read_image(W, H).copy()
            other.render(rt.make_params(W, H, 4, 8, skybox=1, frames=-k))
            raw = other.read_image(W, H).copy()
            mine, hist, motion = other.temporal_accumulate(g, g, cam, mine, np.full((H, W), k, F32), raw, motion=True)
            assert R.same_bits(mine[hit], acc[hit]).all(), k
            assert (~R.same_bits(mine[hit][:, :3], raw[hit][:, :3])).mean() > 0.9, k
            assert np.array_equal(motion[hit], np.zeros_like(motion[hit])) and (hist[hit] == k + 1).all(), k
            assert R.same_bits(mine[~hit], raw[~hit]).all() and (hist[~hit] == 1).all(), k
    finally:
        other.close()


def test_no_side_effects(rt, tracer, cornell):
    """A render sequence with temporal_accumulate calls between its frames: the image, rt_get_stats and the launch words as
    without."""
    f, history = frames(rt, tracer, cornell, 67, 45)
    pcam, prev_color, pg = f["base"]
    _, color, g = f["large"]

    def run(accumulate, frame_ahead):
        tracer.set_option("frame_ahead", frame_ahead)
        tracer.load_scene(cornell)
        tracer.reset_timing()
        for fr in range(12):
            tracer.render(rt.make_params(64, 48, 3, 2, skybox=1, frames=fr))
            if accumulate:
                tracer.temporal_accumulate(g, pg, pcam, prev_color, history, color, motion=bool(fr & 1))
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
    p = {}
    for k, (dt, n) in A.TEMPORAL_PLANES.items():
        shape = (H, W, n) if n else (H, W)
        p[k] = np.ones(shape, np.uint32) if dt == "<u4" else rng.uniform(0.5, 2, shape).astype(F32)
    p["normal"][:] = p["prev_normal"][:] = (0, 0, -1)
    p["point"][:] = p["prev_point"][:] = (0, 0, 3)    # in front of the identity camera: every texel finds history
    for k in ("out", "out_history", "motion"):
        p[k][:] = MARK
    return p


def _camera():
    cam = A.CameraUniform()
    for i in range(4):
        cam.cam_to_world[i][i] = 1.0
    cam.view_params[:] = (1.2, 0.8, 1.5)
    return cam


def _raw(t, planes, W, H, flags=A.TEMPORAL_HOST_MEMORY, **over):
    d = A.TemporalDesc(struct_bytes=C.sizeof(A.TemporalDesc), width=W, height=H, prev_camera=_camera(), max_history=8.0,
                       point_tolerance=0.01, normal_cos=0.9)
    for k, v in planes.items():
        setattr(d, k, v.ctypes.data)
    for k, v in over.items():
        setattr(d, k, v)
    return t._L.rt_temporal_accumulate(t._h, C.byref(d), flags)


def _untouched(p):
    return all(np.all(p[k] == MARK) for k in ("out", "out_history", "motion"))


def _host_of(rt, p):
    g = {k: p[k] for k in CHANNELS}
    pg = {k: p["prev_" + k] for k in CHANNELS}
    return rt.temporal_accumulate_host(g, pg, _camera(), p["prev_color"], p["prev_history"], p["color"], 8.0, motion=True)


def test_staging_is_capped_and_nothing_is_kept(rt):
    """The host-memory path stages 104 bytes per texel with every plane (13 MiB at 512x256): a cap that has no room for them
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
        t.set_option("max_device_mb", before + 14)
        assert _raw(t, p, W, H) == 0
        for a, b in zip((p["out"], p["out_history"], p["motion"]), _host_of(rt, p)):
            assert R.same_bits(a, b).all()
        assert t.last_launch()["device_mb_held"] == before
        t.set_option("max_device_mb", 0)
        q = _planes(W, H)
        assert _raw(t, q, W, H) == 0 and R.same_bits(q["out"], p["out"]).all()
    finally:
        t.close()


def test_errors(rt):
    """The argument errors on the device entry point, the device-only ones included; the outputs stay as they were."""
    t = rt.RayTracer(device=0, max_width=16, max_height=16)
    L, h = t._L, t._h
    W, H = 8, 6

    def err():
        return L.rt_last_error(h).decode()

    try:
        p = _planes(W, H)
        d = A.TemporalDesc(struct_bytes=C.sizeof(A.TemporalDesc))
        assert L.rt_temporal_accumulate(None, C.byref(d), 1) == -1
        assert L.rt_temporal_accumulate(h, None, 1) == -1 and "null" in err()
        assert _raw(t, p, W, H, flags=3) == -1 and "flags" in err()
        assert _raw(t, p, W, H, flags=-2) == -1 and "flags" in err()
        nan, inf = float("nan"), float("inf")
        for over, text in ((dict(struct_bytes=200), "struct_bytes"), (dict(_p0=1), "_p0"), (dict(width=0), "zero"), (dict(height=0), "zero"),
                           (dict(max_history=0.5), "max_history"), (dict(max_history=nan), "max_history"),
                           (dict(point_tolerance=0.0), "point_tolerance"), (dict(point_tolerance=nan), "point_tolerance"),
                           (dict(point_tolerance=inf), "point_tolerance"), (dict(point_tolerance=-1.0), "point_tolerance"),
                           (dict(normal_cos=nan), "normal_cos"), (dict(normal_cos=1.5), "normal_cos"), (dict(normal_cos=-1.5), "normal_cos"),
                           (dict(point=None), "null"), (dict(normal=None), "null"), (dict(prev_color=None), "null"),
                           (dict(prev_history=None), "null"), (dict(prev_point=None), "null"), (dict(prev_normal=None), "null"),
                           (dict(out=None), "null"), (dict(out_history=None), "null")):
            for flags in (0, 1):
                assert _raw(t, p, W, H, flags=flags, **over) == -1 and text in err(), (over, flags, err())
        # a NULL colour with the host flag (without it, it names the image: tests/_temporal_device_path.py)
        assert _raw(t, p, W, H, flags=1, color=None) == -1 and "color" in err()
        assert _raw(t, p, 1 << 16, 1 << 15) == -2 and "2^31" in err()
        # device planes (host arrays' addresses stand in for device pointers: the checks come before any use)
        assert all(v.ctypes.data % 16 == 0 for v in p.values())
        need = {"color": 16, "point": 4, "normal": 4, "object": 4, "prev_color": 16, "prev_history": 4, "prev_point": 4,
                "prev_normal": 4, "prev_object": 4, "out": 16, "out_history": 4, "motion": 8}
        assert list(need) == list(A.TEMPORAL_PLANES)
        for c, a in need.items():
            for off in (1, 2, 4, 8):
                if off % a:
                    assert _raw(t, p, W, H, flags=0, **{c: p[c].ctypes.data + off}) == -1 and f"plane {c} " in err() and "aligned" in err(), (c, off)
        # a NULL colour names the image: 16 x 16 texels here
        assert _raw(t, p, 17, 16, flags=0, color=None) == -2 and "image" in err()
        assert _raw(t, p, 256, 2, flags=0, color=None) == -2 and "image" in err()
        assert _untouched(p)
        assert _raw(t, p, W, H) == 0 and not any(np.any(p[k] == MARK) for k in ("out", "out_history", "motion"))
        for a, b in zip((p["out"], p["out_history"], p["motion"]), _host_of(rt, p)):
            assert R.same_bits(a, b).all()
    finally:
        t.close()


def test_device_path():
    """Torch tensors on the device (tests/_temporal_device_path.py, a process of its own that imports torch first)."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "_temporal_device_path.py")],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "device path ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
