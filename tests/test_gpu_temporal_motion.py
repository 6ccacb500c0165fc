"""rt_temporal_accumulate_moving (include/rt_abi.h; csrc/rt_temporal.hip) against rt_temporal_accumulate_moving_host, bit for
bit, on real planes -- render_gbuffer plus a render of the Cornell fixture before and after update_instances moved its two
boxes and the camera moved too -- through the host-memory path; an all-static table against the call without one; then side
effects, the staging buffer's cap with the table counted, and the errors.  The device path (torch tensors, a device-resident
table, a NULL colour for the handle's image) runs in a process of its own: tests/_temporal_motion_device_path.py."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import _temporal_motion_reference as M
import _temporal_reference as R
from ray_tracer_2_amd import _abi as A

pytestmark = pytest.mark.gpu

F32 = np.float32
# 130x70 is wider than any tile in both axes (tiles are 32x8): the gather crosses tile seams
SIZES = [(67, 45), (24, 16), (130, 70)]
SMALL = [(1, 1), (8, 1), (1, 8)]
CHANNELS = ("point", "normal", "object")
MOVES = {"small": dict(right=0.03, up=0.01), "large": dict(right=0.5, up=-0.12, forward=0.1)}
MARK = F32(-7.25)

_frames = {}


def moved_scene(cornell):
    return M.moved_mesh(cornell, {5: M.rigid((0.06, 0.0, 0.02), 0.05, M.centroid(cornell, 5)),
                                  6: M.rigid((-0.04, 0.0, 0.03), -0.08, M.centroid(cornell, 6))})


def frames(rt, tracer, cornell, W, H, render=True):
    """The previous frame (the fixture as it is, under its own camera) and, per camera move, the current one after
    update_instances moved meshes 5 and 6: (camera, colour, guides) each -- the colour one 8 spp / 4 bounce frame, or noise
    with render=False --, a history length per texel and the motion table.  Rendered once per size."""
    if (W, H) not in _frames:
        tracer.load_scene(cornell)
        base = cornell.uniform.camera
        moved = moved_scene(cornell)
        rng = np.random.default_rng(W + H)

        def frame(cam):
            tracer.set_camera(cam)
            if render:
                tracer.render(rt.make_params(W, H, 4, 8, skybox=1, frames=0))
                color = tracer.read_image(W, H).copy()
            else:
                color = rng.uniform(0, 2, (H, W, 4)).astype(F32)
            return cam, color, tracer.render_gbuffer(rt.make_params(W, H, 1, 1), CHANNELS)

        out = {}
        try:
            out["base"] = frame(base)
            tracer.update_instances(moved)
            for name, mv in MOVES.items():
                out[name] = frame(R.moved_camera(base, **mv))
        finally:
            tracer.update_instances(cornell)
            tracer.set_camera(base)
        history = rng.integers(1, 7, (H, W)).astype(F32)
        _frames[(W, H)] = (out, history, rt.object_motions(cornell, moved))
    return _frames[(W, H)]


def both(rt, tracer, g, pg, cam, prev_color, history, color, motions, objects=True, what="", **kw):
    """The device (host-memory path) against the host; returns the device's outputs."""
    if not objects:
        pg = {k: v for k, v in pg.items() if k != "object"}
    want = rt.temporal_accumulate_host(g, pg, cam, prev_color, history, color, motions=motions, **kw)
    got = tracer.temporal_accumulate(g, pg, cam, prev_color, history, color, motions=motions, **kw)
    assert len(got) == len(want)
    for a, b, name in zip(got, want, ("out", "out_history", "motion")):
        bad = ~R.same_bits(a, b)
        assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    return got


@pytest.mark.parametrize("W,H", SIZES)
def test_device_equals_host(rt, tracer, cornell, W, H):
    """Both camera moves with both boxes moved; prev_object and motion on and off; the cap active and not; out = color."""
    f, history, motions = frames(rt, tracer, cornell, W, H)
    assert motions["moved"].nonzero()[0].tolist() == [5, 6]
    pcam, prev_color, pg = f["base"]
    for move in MOVES:
        _, color, g = f[move]
        boxes = (g["object"] == 5) | (g["object"] == 6)
        assert boxes.sum() >= 8, (W, H, move)
        for objects, motion, cap in itertools.product((True, False), (True, False), (3.0, np.inf)):
            got = both(rt, tracer, g, pg, pcam, prev_color, history, color, motions, objects, (W, H, move, objects, motion, cap),
                       max_history=cap, motion=motion)
            assert (got[1][boxes] > 1).mean() > 0.5, (W, H, move)            # the moved boxes keep their history
            hit = g["object"] != A.MISS
            assert (got[1][hit] > 1).mean() > 0.5 and (got[1][hit] == 1).any(), (W, H, move)
        want = rt.temporal_accumulate_host(g, pg, pcam, prev_color, history, color, 3.0, motions=motions)
        buf, hist = color.copy(), np.zeros((H, W), F32)
        got = tracer.temporal_accumulate(g, pg, pcam, prev_color, history, buf, 3.0, out=buf, out_history=hist, motions=motions)
        assert got[0] is buf and got[1] is hist
        assert R.same_bits(buf, want[0]).all() and R.same_bits(hist, want[1]).all(), (W, H, move, "out is color")


@pytest.mark.parametrize("W,H", SMALL)
def test_small_frames(rt, tracer, cornell, W, H):
    """Frames of one texel, one row and one column: the fixture's guides at that size (noise for the colour) with the boxes and
    the camera moved, and the CPU tests' wall of that size with its one object moved."""
    f, history, motions = frames(rt, tracer, cornell, W, H, render=False)
    pcam, prev_color, pg = f["base"]
    for move in MOVES:
        _, color, g = f[move]
        for objects, motion in itertools.product((True, False), repeat=2):
            both(rt, tracer, g, pg, pcam, prev_color, history, color, motions, objects, (W, H, move, objects, motion), max_history=3.0,
                 motion=motion)
    planes, cam, table = M.small_case(W, H)
    g = {k: planes[k] for k in CHANNELS}
    pg = {k: planes["prev_" + k] for k in CHANNELS}
    for objects, motion in itertools.product((True, False), repeat=2):
        got = both(rt, tracer, g, pg, cam, planes["prev_color"], planes["prev_history"], planes["color"], table, objects,
                   (W, H, "wall", objects, motion), motion=motion)
        assert (got[1] > 1).all()


def test_synthetic_frame(rt, tracer):
    """The 24x16 pair of frames of the CPU tests with a record for every new rule (a word past the table, a point sent to
    infinity, an annihilated normal, moved objects off screen and behind the camera)."""
    planes, cam, motions, notes = M.synthetic_case()
    g = {k: planes[k] for k in CHANNELS}
    pg = {k: planes["prev_" + k] for k in CHANNELS}
    for objects, cap in itertools.product((True, False), (4.0, np.inf)):
        got = both(rt, tracer, g, pg, cam, planes["prev_color"], planes["prev_history"], planes["color"], motions, objects,
                   (objects, cap), max_history=cap, motion=True)
        for k in ("outside_table", "to_infinity", "no_normal", "moved_off_screen", "moved_behind"):
            assert got[1][notes[k]] == 1 and np.isnan(got[2][notes[k]]).all(), k
        assert got[1][notes["sphere"]] > 1


def test_an_all_static_table_changes_nothing(rt, tracer, cornell):
    """Every record with moved == 0: the device's planes are those of temporal_accumulate without a table, bit for bit, under
    both camera moves; a still record's matrices are not read (NaNs in them change nothing)."""
    W, H = 67, 45
    f, history, _ = frames(rt, tracer, cornell, W, H)
    pcam, prev_color, pg = f["base"]
    still = rt.object_motions(cornell, cornell)
    assert not still["moved"].any()
    poisoned = still.copy()
    poisoned["d"][:], poisoned["nt"][:] = np.nan, np.nan
    for move, objects, cap in itertools.product(MOVES, (True, False), (3.0, np.inf)):
        _, color, g = f[move]
        p = pg if objects else {k: v for k, v in pg.items() if k != "object"}
        want = tracer.temporal_accumulate(g, p, pcam, prev_color, history, color, cap, motion=True)
        for t in (still, poisoned):
            got = tracer.temporal_accumulate(g, p, pcam, prev_color, history, color, cap, motion=True, motions=t)
            for a, b, name in zip(got, want, ("out", "out_history", "motion")):
                assert R.same_bits(a, b).all(), (move, objects, cap, name)
        assert (want[1] > 1).mean() > 0.3


def test_no_side_effects(rt, tracer, cornell):
    """A render sequence with temporal_accumulate(motions=) calls between its frames: the image, rt_get_stats and the launch
    words as without."""
    f, history, motions = frames(rt, tracer, cornell, 67, 45)
    pcam, prev_color, pg = f["base"]
    _, color, g = f["large"]

    def run(accumulate, frame_ahead):
        tracer.set_option("frame_ahead", frame_ahead)
        tracer.load_scene(cornell)
        tracer.reset_timing()
        for fr in range(12):
            tracer.render(rt.make_params(64, 48, 3, 2, skybox=1, frames=fr))
            if accumulate:
                tracer.temporal_accumulate(g, pg, pcam, prev_color, history, color, motion=bool(fr & 1), motions=motions)
            else:
                tracer.synchronize()
        img = tracer.read_image(64, 48)
        s = tracer.stats()
        return img, (s.segments, s.paths, s.node_tests, s.triangle_tests, s.frames, s.segments_reused, s.frames_speculative), \
            tuple(tracer.last_launch().values())

    try:
        for fa in (-1, 8):
            a, sa, la = run(False, fa)
            b, sb, lb = run(True, fa)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), fa
            assert (sa == sb) if fa > 0 else (sa[4] == sb[4]), (fa, sa, sb)
            if fa > 0:
                assert la == lb, (la, lb)   # (device_mb_held included: the call keeps no scratch)
    finally:
        tracer.set_option("frame_ahead", -1)


def _planes(W, H, n_objects=2):
    rng = np.random.default_rng(7)
    p = {}
    for k, (dt, n) in A.TEMPORAL_PLANES.items():
        shape = (H, W, n) if n else (H, W)
        p[k] = np.ones(shape, np.uint32) if dt == "<u4" else rng.uniform(0.5, 2, shape).astype(F32)
    p["normal"][:] = p["prev_normal"][:] = (0, 0, -1)
    p["point"][:] = (0.25, 0, 3)
    p["prev_point"][:] = (0, 0, 3)    # record 1 carries the current points onto the previous ones: every texel finds history
    for k in ("out", "out_history", "motion"):
        p[k][:] = MARK
    t = M.table(n_objects)
    M.record(t, 1, translation=(-0.25, 0, 0))
    p["motions"] = t
    return p


def _camera():
    cam = A.CameraUniform()
    for i in range(4):
        cam.cam_to_world[i][i] = 1.0
    cam.view_params[:] = (1.2, 0.8, 1.5)
    return cam


def _raw(t, planes, W, H, flags=A.TEMPORAL_HOST_MEMORY, **over):
    d = A.TemporalMotionDesc(struct_bytes=C.sizeof(A.TemporalMotionDesc), width=W, height=H, prev_camera=_camera(), max_history=8.0,
                             point_tolerance=0.01, normal_cos=0.9, n_objects=len(planes["motions"]))
    for k, v in planes.items():
        setattr(d, k, v.ctypes.data)
    for k, v in over.items():
        setattr(d, k, v)
    return t._L.rt_temporal_accumulate_moving(t._h, C.byref(d), flags)


def _untouched(p):
    return all(np.all(p[k] == MARK) for k in ("out", "out_history", "motion"))


def _host_of(rt, p):
    g = {k: p[k] for k in CHANNELS}
    pg = {k: p["prev_" + k] for k in CHANNELS}
    return rt.temporal_accumulate_host(g, pg, _camera(), p["prev_color"], p["prev_history"], p["color"], 8.0, motion=True, motions=p["motions"])


def test_staging_counts_the_table_and_nothing_is_kept(rt):
    """The host-memory path stages 104 bytes per texel with every plane (13 MiB at 512x256) and the motion table: with a table
    of 32768 records (3 MiB) a cap that has room for the planes alone gives RT_ERR_OUT_OF_MEMORY with the outputs untouched;
    with room for both the call holds nothing afterwards."""
    t = rt.RayTracer(device=0, max_width=16, max_height=16)
    try:
        W, H = 512, 256
        p = _planes(W, H, 32768)
        assert p["motions"].nbytes == 3 << 20
        before = t.last_launch()["device_mb_held"]
        small = dict(p, motions=p["motions"][:2])
        t.set_option("max_device_mb", before + 4)
        assert _raw(t, small, W, H) == -8 and b"max_device_mb" in t._L.rt_last_error(t._h)
        t.set_option("max_device_mb", before + 14)
        assert _raw(t, p, W, H) == -8 and b"max_device_mb" in t._L.rt_last_error(t._h)      # the planes would fit: the table is counted
        assert _untouched(p)
        assert t.last_launch()["device_mb_held"] == before
        assert _raw(t, small, W, H) == 0                                                      # (they do fit, with a table of two records)
        for k in ("out", "out_history", "motion"):
            small[k][:] = MARK
        t.set_option("max_device_mb", before + 17)
        assert _raw(t, p, W, H) == 0
        for a, b in zip((p["out"], p["out_history"], p["motion"]), _host_of(rt, p)):
            assert R.same_bits(a, b).all()
        assert (p["out_history"] > 1).all()
        assert t.last_launch()["device_mb_held"] == before
        t.set_option("max_device_mb", 0)
        q = _planes(W, H, 32768)
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
        d = A.TemporalMotionDesc(struct_bytes=C.sizeof(A.TemporalMotionDesc))
        assert L.rt_temporal_accumulate_moving(None, C.byref(d), 1) == -1
        assert L.rt_temporal_accumulate_moving(h, None, 1) == -1 and "null" in err()
        assert _raw(t, p, W, H, flags=3) == -1 and "flags" in err()
        assert _raw(t, p, W, H, flags=-2) == -1 and "flags" in err()
        nan, inf = float("nan"), float("inf")
        for over, text in ((dict(struct_bytes=208), "struct_bytes"), (dict(_p0=1), "_p0"), (dict(_p1=1), "_p1"), (dict(width=0), "zero"),
                           (dict(height=0), "zero"), (dict(max_history=0.5), "max_history"), (dict(max_history=nan), "max_history"),
                           (dict(point_tolerance=0.0), "point_tolerance"), (dict(point_tolerance=inf), "point_tolerance"),
                           (dict(normal_cos=nan), "normal_cos"), (dict(normal_cos=1.5), "normal_cos"),
                           (dict(point=None), "null"), (dict(normal=None), "null"), (dict(object=None), "object"),
                           (dict(prev_color=None), "null"), (dict(prev_history=None), "null"), (dict(prev_point=None), "null"),
                           (dict(prev_normal=None), "null"), (dict(out=None), "null"), (dict(out_history=None), "null"),
                           (dict(motions=None), "motions"), (dict(n_objects=0), "n_objects")):
            for flags in (0, 1):
                assert _raw(t, p, W, H, flags=flags, **over) == -1 and text in err(), (over, flags, err())
        assert _raw(t, p, W, H, flags=1, color=None) == -1 and "color" in err()
        assert _raw(t, p, 1 << 16, 1 << 15) == -2 and "2^31" in err()
        # device planes (host arrays' addresses stand in for device pointers: the checks come before any use)
        aligned = np.zeros(p["motions"].nbytes + 16, np.uint8)
        off = (-aligned.ctypes.data) % 16
        table = aligned[off:off + p["motions"].nbytes]
        table[:] = p["motions"].view(np.uint8)
        p["motions"] = table.view(A.OBJECT_MOTION_DTYPE)
        assert all(v.ctypes.data % 16 == 0 for v in p.values())
        need = {"color": 16, "point": 4, "normal": 4, "object": 4, "prev_color": 16, "prev_history": 4, "prev_point": 4,
                "prev_normal": 4, "prev_object": 4, "out": 16, "out_history": 4, "motion": 8, "motions": 16}
        assert list(need) == list(A.TEMPORAL_MOTION_PLANES)
        for c, a in need.items():
            for off in (1, 2, 4, 8):
                if off % a:
                    name = f"plane {c} "
                    assert _raw(t, p, W, H, flags=0, **{c: p[c].ctypes.data + off}) == -1 and name in err() and "aligned" in err(), (c, off, err())
        # a NULL colour names the image: 16 x 16 texels here
        assert _raw(t, p, 17, 16, flags=0, color=None) == -2 and "image" in err()
        assert _untouched(p)
        assert _raw(t, p, W, H) == 0 and not any(np.any(p[k] == MARK) for k in ("out", "out_history", "motion"))
        for a, b in zip((p["out"], p["out_history"], p["motion"]), _host_of(rt, p)):
            assert R.same_bits(a, b).all()
    finally:
        t.close()


def test_device_path():
    """Torch tensors on the device (tests/_temporal_motion_device_path.py, a process of its own that imports torch first)."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "_temporal_motion_device_path.py")],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "device path ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
