"""rt_display and rt_auto_exposure (include/rt_abi.h; csrc/rt_display.hip) against rt_display_host and rt_auto_exposure_host,
bit for bit, through the host-memory path: a synthetic frame that holds every threshold with both neighbours and the special
values, and a rendered Cornell frame over thirteen stops of exposure, at sizes narrower and wider than a wave's row and
larger than one workgroup's chunk; the meter on a rendered frame, a frame that hits every bin and a frame in one bin; the
chain; then side effects, the staging buffer's cap, the errors, and the display snapshot pair.  The device path (torch
tensors, a NULL color for the handle's image) runs in a process of its own: tests/_display_device_path.py."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import _display_reference as R
from ray_tracer_2_amd import _abi as A

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
# 130 x 70 = 9100 texels: nine workgroups' chunks of 1024 in the display kernel, five of 2048 in the count kernel, with a tail
SIZES = [(1, 1), (7, 3), (33, 9), (130, 70), (257, 5)]
TONES = [("clamp", 1.0), ("reinhard", 0.5), ("reinhard", 4.0), ("reinhard", np.inf)]
MARK = 0xA5

_frames = {}


def cornell_frame(rt, tracer, cornell, W=64, H=36):
    """One 8 spp / 4 bounce Cornell frame, rendered once."""
    if (W, H) not in _frames:
        tracer.load_scene(cornell)
        tracer.render(rt.make_params(W, H, 4, 8, skybox=1, frames=0))
        _frames[(W, H)] = tracer.read_image(W, H).copy()
        assert np.isfinite(_frames[(W, H)]).all() and (_frames[(W, H)][..., :3] > 1).any()   # (the lamp clips at exposure 1)
    return _frames[(W, H)]


def both(rt, tracer, color, what, **kw):
    want = rt.display_host(color, **kw)
    got = tracer.display(color, **kw)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == want.shape, what
    bad = (got != want).any(-1)
    assert not bad.any(), (what, kw, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    return got


@pytest.mark.parametrize("W,H", SIZES)
def test_device_equals_host_on_the_threshold_frame(rt, tracer, W, H):
    """Every T[k] with both neighbours and the special values in every channel (at the larger sizes: the small ones hold the
    head of the list), every tone x transfer x layout."""
    color = R.threshold_frame(W, H)
    for (tone, white), transfer, layout in itertools.product(TONES, ("srgb", "linear"), range(4)):
        got = both(rt, tracer, color, (W, H), tone=tone, white=white, transfer=transfer, bgra=bool(layout & 1), top_first=bool(layout & 2))
    if W * H >= 400:   # (twice the list: alpha takes every fourth float of the first round)
        plain = both(rt, tracer, color, (W, H))
        assert len(np.unique(plain[..., :3])) == 256 and np.array_equal(plain, R.display(color))
    assert got.shape == (H, W, 4)


def test_device_equals_host_on_a_rendered_frame(rt, tracer, cornell):
    color = cornell_frame(rt, tracer, cornell)
    seen = set()
    for stop in range(-6, 7):
        for (tone, white), transfer in itertools.product(TONES[:1] + TONES[2:3], ("srgb", "linear")):
            got = both(rt, tracer, color, stop, exposure=2.0 ** stop, tone=tone, white=white, transfer=transfer, bgra=True)
        seen.add(got.tobytes())
    assert len(seen) == 13
    for layout in range(4):
        both(rt, tracer, color, layout, bgra=bool(layout & 1), top_first=bool(layout & 2), exposure_scale=np.array([0.37], F32))
    # the window: what the restatement in numpy gives too
    assert np.array_equal(both(rt, tracer, color, "window", bgra=True), R.display(color, layout=R.BGRA))


def meter_both(rt, tracer, color, what, **kw):
    ws, wh = rt.auto_exposure_host(color, histogram=True, **kw)
    gs, gh = tracer.auto_exposure(color, histogram=True, **kw)
    assert gh.dtype == U32 and np.array_equal(gh, wh), (what, kw, np.argwhere(gh != wh)[:4].tolist())
    assert gs.dtype == F32 and gs.shape == (1,) and gs.view(U32)[0] == ws.view(U32)[0], (what, kw, gs, ws)
    alone = tracer.auto_exposure(color, **kw)
    assert isinstance(alone, np.ndarray) and alone.view(U32)[0] == ws.view(U32)[0], (what, "without the histogram")
    return gs, gh


def meter_frames(rt, tracer, cornell):
    return {"rendered": cornell_frame(rt, tracer, cornell, 130, 70), "every bin": R.every_bin_frame(130, 70), "one bin": R.one_bin_frame(130, 70)}


@pytest.mark.parametrize("name", ["rendered", "every bin", "one bin"])
def test_auto_exposure_device_equals_host(rt, tracer, cornell, name):
    color = meter_frames(rt, tracer, cornell)[name]
    wide = dict(min_scale=2.0 ** -40, max_scale=2.0 ** 40)
    for lo, hi in ((100, 950), (0, 1000), (0, 1), (999, 1000), (250, 750)):
        s, h = meter_both(rt, tracer, color, name, low_permille=lo, high_permille=hi, **wide)
        assert np.array_equal(h, R.histogram(color)) and s.view(U32)[0] == np.array([R.meter(h, lo, hi, **wide)], F32).view(U32)[0]
    meter_both(rt, tracer, color, name)
    for prev in (3.0, np.nan, 0.0):
        meter_both(rt, tracer, color, name, prev_scale=prev, rate=0.25)
    if name == "every bin":
        assert (h > 0).all()
    if name == "one bin":
        assert np.count_nonzero(h) == 1 and h.sum() == 130 * 70
    # the same call twice gives the same bits (integer atomics: no arrival order in the result)
    a, b = (tracer.auto_exposure(color, histogram=True) for _ in range(2))
    assert a[0].view(U32)[0] == b[0].view(U32)[0] and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("W,H", [(1, 1), (7, 3), (257, 5)])
def test_auto_exposure_small_sizes(rt, tracer, W, H):
    meter_both(rt, tracer, R.hdr_frame(W, H), (W, H), low_permille=0, high_permille=1000)
    meter_both(rt, tracer, np.zeros((H, W, 4), F32), (W, H, "black"))


def test_the_chain_on_host_memory_equals_the_host_chain(rt, tracer, cornell):
    color = cornell_frame(rt, tracer, cornell, 130, 70)
    want_scale = rt.auto_exposure_host(color)
    assert want_scale[0] != 1 and 2.0 ** -10 < want_scale[0] < 2.0 ** 10
    want = rt.display_host(color, tone="reinhard", white=4.0, bgra=True, exposure_scale=want_scale)
    scale = tracer.auto_exposure(color)
    got = tracer.display(color, tone="reinhard", white=4.0, bgra=True, exposure_scale=scale)
    assert scale.view(U32)[0] == want_scale.view(U32)[0] and np.array_equal(got, want)
    assert not np.array_equal(got, tracer.display(color, tone="reinhard", white=4.0, bgra=True))
    assert np.array_equal(got, tracer.display(color, tone="reinhard", white=4.0, bgra=True, exposure_scale=scale))   # twice: the same bits


def test_no_side_effects(rt, tracer, cornell):
    """A render sequence with display and auto_exposure calls between its frames: the image, rt_get_stats and the launch words
    as without (device_mb_held too, once the meter's 1 KiB of bins -- which round up into the same MiB -- are held)."""
    color = cornell_frame(rt, tracer, cornell)
    tracer.auto_exposure(color)

    def run(calls, frame_ahead):
        tracer.set_option("frame_ahead", frame_ahead)
        tracer.load_scene(cornell)
        tracer.reset_timing()
        for fr in range(12):
            tracer.render(rt.make_params(64, 48, 3, 2, skybox=1, frames=fr))
            if calls:
                s = tracer.auto_exposure(color, histogram=bool(fr & 1))
                tracer.display(color, bgra=bool(fr & 1), exposure_scale=s[0] if fr & 1 else s)
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
            assert np.array_equal(a.view(U32), b.view(U32)), fa
            # (the automatic policy renders ahead by what it finds on the stream: only the frames asked for are schedule-free)
            assert (sa == sb) if fa > 0 else (sa[4] == sb[4]), (fa, sa, sb)
            if fa > 0:
                assert la == lb, (la, lb)
    finally:
        tracer.set_option("frame_ahead", -1)


def _display_raw(t, color_plane, out_plane, W, H, flags=A.DISPLAY_HOST_MEMORY, **over):
    d = A.DisplayDesc(struct_bytes=C.sizeof(A.DisplayDesc), width=W, height=H, exposure=1.0, white=1.0)
    for k, v in dict(dict(color=color_plane.ctypes.data, out=out_plane.ctypes.data), **over).items():
        setattr(d, k, v)
    return t._L.rt_display(t._h, C.byref(d), flags)


def _meter_planes(W, H):
    return dict(color=np.ones((H, W, 4), F32), prev_scale=np.array([2.0], F32), histogram=np.full(256, 0xA5A5A5A5, U32), scale=np.array([-7.25], F32))


def _meter_raw(t, p, W, H, flags=A.AUTO_EXPOSURE_HOST_MEMORY, **over):
    d = A.AutoExposureDesc(struct_bytes=C.sizeof(A.AutoExposureDesc), width=W, height=H, low_permille=100, high_permille=900, key=0.18,
                           min_scale=0.01, max_scale=100.0, rate=1.0)
    for k, v in dict({k: v.ctypes.data for k, v in p.items()}, **over).items():
        setattr(d, k, v)
    return t._L.rt_auto_exposure(t._h, C.byref(d), flags)


def _meter_untouched(p):
    return bool(p["scale"][0] == F32(-7.25) and np.all(p["histogram"] == 0xA5A5A5A5))


def test_staging_is_capped_and_only_the_bins_are_kept(rt):
    """The host-memory paths stage 20 (display) and 16 (meter) bytes per texel: 10 and 8 MiB for 1024 x 512.  A cap that has no
    room for them gives RT_ERR_OUT_OF_MEMORY with the outputs untouched; with room the calls hold nothing afterwards but
    the meter's 1 KiB; no scene is needed."""
    t = rt.RayTracer(device=0, max_width=16, max_height=16)
    try:
        W, H = 1024, 512
        color = np.random.default_rng(5).random((H, W, 4), F32)
        out = np.full((H, W, 4), MARK, np.uint8)
        before = t.last_launch()["device_mb_held"]
        t.set_option("max_device_mb", before + 6)
        assert _display_raw(t, color, out, W, H) == -8 and b"max_device_mb" in t._L.rt_last_error(t._h)
        p = dict(_meter_planes(W, H), color=color)
        assert _meter_raw(t, p, W, H) == -8 and b"max_device_mb" in t._L.rt_last_error(t._h)
        assert np.all(out == MARK) and _meter_untouched(p)
        assert t.last_launch()["device_mb_held"] == before
        t.set_option("max_device_mb", before + 12)
        assert _display_raw(t, color, out, W, H) == 0 and np.array_equal(out, rt.display_host(color))
        assert _meter_raw(t, p, W, H) == 0
        ws, wh = rt.auto_exposure_host(color, low_permille=100, high_permille=900, min_scale=0.01, max_scale=100.0, prev_scale=2.0, histogram=True)
        assert p["scale"].view(U32)[0] == ws.view(U32)[0] and np.array_equal(p["histogram"], wh)
        assert t.last_launch()["device_mb_held"] <= before + 1   # (the bins: 1 KiB)
        t.set_option("max_device_mb", 0)
        out2 = np.full((H, W, 4), MARK, np.uint8)
        assert _display_raw(t, color, out2, W, H) == 0 and np.array_equal(out2, out)
    finally:
        t.close()


def test_errors(rt):
    """The argument errors on the device entry points, the device-only ones included; the outputs stay as they were."""
    t = rt.RayTracer(device=0, max_width=16, max_height=16)
    L, hd = t._L, t._h
    W, H = 9, 7
    nan, inf = float("nan"), float("inf")

    def err():
        return L.rt_last_error(hd).decode()

    try:
        color, out = np.ones((H, W, 4), F32), np.full((H, W, 4), MARK, np.uint8)
        d = A.DisplayDesc(struct_bytes=C.sizeof(A.DisplayDesc))
        assert L.rt_display(None, C.byref(d), 1) == -1
        assert L.rt_display(hd, None, 1) == -1 and "null" in err()
        assert _display_raw(t, color, out, W, H, flags=3) == -1 and "flags" in err()
        assert _display_raw(t, color, out, W, H, flags=-2) == -1 and "flags" in err()
        for over, text in ((dict(struct_bytes=56), "struct_bytes"), (dict(_p0=1), "_p0"), (dict(_p1=1), "_p1"), (dict(width=0), "zero"),
                           (dict(height=0), "zero"), (dict(tone=2), "tone"), (dict(transfer=2), "transfer"), (dict(layout=4), "layout"),
                           (dict(exposure=0.0), "exposure"), (dict(exposure=nan), "exposure"), (dict(exposure=inf), "exposure"),
                           (dict(exposure=-1.0), "exposure"), (dict(tone=1, white=0.0), "white"), (dict(tone=1, white=nan), "white"),
                           (dict(out=None), "out")):
            for flags in (0, 1):
                assert _display_raw(t, color, out, W, H, flags=flags, **over) == -1 and text in err(), (over, flags, err())
        assert _display_raw(t, color, out, W, H, flags=1, color=None) == -1 and "color" in err()
        assert _display_raw(t, color, out, 1 << 16, 1 << 15) == -2 and "2^31" in err()
        # device planes (host arrays' addresses stand in for device pointers: the checks come before any use)
        scale = np.ones(4, F32)
        assert color.ctypes.data % 16 == 0 and out.ctypes.data % 16 == 0 and scale.ctypes.data % 16 == 0
        for name, base, a in (("color", color, 16), ("out", out, 4), ("exposure_scale", scale, 4)):
            for off in (1, 2, 4, 8):
                if off % a:
                    rc = _display_raw(t, color, out, W, H, flags=0, **dict(dict(exposure_scale=scale.ctypes.data), **{name: base.ctypes.data + off}))
                    assert rc == -1 and f"plane {name} " in err() and "aligned" in err(), (name, off)
        # a NULL color names the image: 16 x 16 texels here
        assert _display_raw(t, color, out, 17, 16, flags=0, color=None) == -2 and "image" in err()
        assert np.all(out == MARK)
        assert _display_raw(t, color, out, W, H) == 0 and np.all(out == 255)

        p = _meter_planes(W, H)
        m = A.AutoExposureDesc(struct_bytes=C.sizeof(A.AutoExposureDesc))
        assert L.rt_auto_exposure(None, C.byref(m), 1) == -1
        assert L.rt_auto_exposure(hd, None, 1) == -1 and "null" in err()
        assert _meter_raw(t, p, W, H, flags=2) == -1 and "flags" in err()
        for over, text in ((dict(struct_bytes=64), "struct_bytes"), (dict(_p0=1), "_p0"), (dict(width=0), "zero"), (dict(height=0), "zero"),
                           (dict(low_permille=500, high_permille=500), "permille"), (dict(high_permille=1001), "permille"),
                           (dict(key=0.0), "key"), (dict(key=nan), "key"), (dict(key=inf), "key"), (dict(min_scale=0.0), "min_scale"),
                           (dict(max_scale=inf), "max_scale"), (dict(min_scale=2.0, max_scale=1.0), "min_scale"), (dict(rate=0.0), "rate"),
                           (dict(rate=1.5), "rate"), (dict(rate=nan), "rate"), (dict(scale=None), "scale")):
            for flags in (0, 1):
                assert _meter_raw(t, p, W, H, flags=flags, **over) == -1 and text in err(), (over, flags, err())
        assert _meter_raw(t, p, W, H, flags=1, color=None) == -1 and "color" in err()
        assert _meter_raw(t, p, 1 << 16, 1 << 15) == -2 and "2^31" in err()
        big = {k: np.zeros(v.size + 8, v.dtype) for k, v in p.items()}
        assert all(v.ctypes.data % 16 == 0 for v in big.values())
        for name, a in (("color", 16), ("prev_scale", 4), ("histogram", 4), ("scale", 4)):
            for off in (1, 2, 4, 8):
                if off % a:
                    assert _meter_raw(t, big, W, H, flags=0, **{name: big[name].ctypes.data + off}) == -1 and f"plane {name} " in err(), (name, off)
        assert _meter_raw(t, p, 17, 16, flags=0, color=None) == -2 and "image" in err()
        assert _meter_untouched(p)
        assert _meter_raw(t, p, W, H) == 0 and not _meter_untouched(p) and p["histogram"].sum() == W * H
    finally:
        t.close()


def test_display_snapshot_is_the_frame_of_its_call_while_later_frames_render(rt, cornell):
    """rt_snapshot_display / rt_read_display_snapshot: the picture taken behind frame k is display_host of frame k although
    frame k + 1 was queued before it was read; a float snapshot taken in between is frame k too; the buffer is counted
    from its first use on, and a cap that has no room for it refuses the snapshot."""
    w, h, n = 320, 180, 5
    kw = dict(tone="reinhard", white=4.0, bgra=True, top_first=True, exposure=0.75)
    t = rt.RayTracer(0, w, h)
    try:
        with pytest.raises(rt.RtError):
            t.read_display_snapshot(w, h)                           # nothing taken yet
        t.load_scene(cornell)
        with pytest.raises(rt.RtError) as e:
            t.snapshot_display(w + 1, h)                            # larger than the image
        assert e.value.code == -2
        d = A.DisplayDesc(struct_bytes=C.sizeof(A.DisplayDesc), width=w, height=h, exposure=1.0, white=1.0)
        junk = np.zeros(16, F32)
        for over in (dict(color=junk.ctypes.data), dict(out=junk.ctypes.data), dict(tone=2), dict(exposure=0.0)):
            bad = A.DisplayDesc.from_buffer_copy(d)
            for k, v in over.items():
                setattr(bad, k, v)
            assert t._L.rt_snapshot_display(t._h, C.byref(bad)) == -1, over
        t.set_option("frame_ahead", 0)
        t.set_option("pipeline", 0)
        want = []
        for f in range(n):
            t.render(rt.make_params(w, h, 4, 3, skybox=1, frames=f))
            want.append(t.read_image(w, h).copy())
        held = t.last_launch()["device_mb_held"]
        # a lowered cap refuses the first display snapshot (225 KiB that round into one more MiB or not: the cap is below what is held)
        t.set_option("max_device_mb", 1)
        with pytest.raises(rt.RtError) as e:
            t.snapshot_display(w, h, **kw)
        assert e.value.code == -8 and "max_device_mb" in str(e.value)
        t.set_option("max_device_mb", 0)
        assert t.last_launch()["device_mb_held"] == held            # unchanged before the first use
        for ahead, pipe in ((0, 0), (0, 4), (-1, 1)):
            t.set_option("frame_ahead", ahead)
            t.set_option("pipeline", pipe)
            t.write_image(np.zeros((h, w, 4), F32))
            got, floats = [], []
            t.render(rt.make_params(w, h, 4, 3, skybox=1, frames=0))
            t.snapshot_display(w, h, **kw)
            for f in range(1, n):
                t.snapshot_image(w, h)                              # the float pair in between: frame f - 1 too
                t.render(rt.make_params(w, h, 4, 3, skybox=1, frames=f))   # queued before frame f - 1 is read
                got.append(t.read_display_snapshot(w, h))
                floats.append(t.read_snapshot(w, h))
                if f == 2:
                    assert np.array_equal(t.read_display_snapshot(w, h), got[-1])                    # twice
                    assert np.array_equal(t.read_display_snapshot(w, h // 2), got[-1][: h // 2])      # in part
                t.snapshot_display(w, h, **kw)
            got.append(t.read_display_snapshot(w, h))
            for f in range(n):
                assert np.array_equal(got[f], rt.display_host(want[f], **kw)), (ahead, pipe, f)
            for f in range(n - 1):
                assert np.array_equal(floats[f].view(U32), want[f].view(U32)), (ahead, pipe, f)
            assert np.array_equal(t.read_image(w, h).view(U32), want[-1].view(U32))
        # out[4] counts the buffer from its first use on: w * h * 4 bytes more, in whole MiB
        t2 = rt.RayTracer(0, 1024, 1024)
        try:
            t2.write_image(np.zeros((1024, 1024, 4), F32))
            a = t2.last_launch()["device_mb_held"]
            t2.snapshot_display(1024, 1024)
            assert t2.last_launch()["device_mb_held"] == a + 4     # 4 MiB exactly
            assert not t2.read_display_snapshot(1024, 1024)[..., :3].any()
        finally:
            t2.close()
    finally:
        t.close()


def test_device_path():
    """Torch tensors on the device (tests/_display_device_path.py, a process of its own that imports torch first)."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "_display_device_path.py")],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "device path ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
