"""rt_adaptive_plan and rt_adaptive_merge (include/rt_abi.h; csrc/rt_adaptive.hip) against their host forms, bit for bit, on
the synthetic planes of the CPU tests and on sizes that reach every level of the plan's scans -- through the host-memory
path --; then the loop end to end on the Cornell fixture, the tail of the ray list, the scratch's bookkeeping, side effects and
errors.  The device path (torch tensors, a NULL colour for the handle's image, adaptive_samples without a host
synchronisation) runs in a process of its own: tests/_adaptive_device_path.py.

The scans work on blocks of 1024 texels and one workgroup scans the block sums 1024 at a time: 24x16 ... 1x8 stay inside one
block, 41x25 = 1025 texels (one more than a block) and 130x70 reach several blocks and the block scan's first round, and
1025x1031 = 1033 blocks reaches its second round, the carry -- the last level there is."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _adaptive_reference as R
from _adaptive_reference import ORIGIN, SIZES, assert_plan_equal, merge_inputs, plan_cases
from ray_tracer_2_amd import _abi as A

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
GPU_SIZES = SIZES + [(130, 70), (41, 25)]


@pytest.mark.parametrize("W,H", GPU_SIZES)
def test_plan_device_equals_host(rt, tracer, W, H):
    d = R.dir_plane(W, H)
    for name, v, budget, mn, mx, ff in plan_cases(W, H):
        want = rt.adaptive_plan_host(v, d, ORIGIN, budget, mn, mx, ff)
        assert_plan_equal(tracer.adaptive_plan(v, d, ORIGIN, budget, mn, mx, ff), want, (W, H, name))


def test_plan_over_every_level_of_the_scans(rt, tracer):
    """1025 x 1031: 1033 blocks, the second round of the one-workgroup scans.  Plan only."""
    W, H = 1025, 1031
    T = W * H
    v, d = R.variance_plane(W, H), R.dir_plane(W, H)
    spike = np.full((H, W), F32(1e-6))
    spike.ravel()[::5] = F32(4.0)
    for name, vv, budget, mn, mx, ff in (("no clamp", v, 3 * T, 1, 65535, 5), ("clamped, a long tail", spike, 3 * T + 5000, 0, 6, 0)):
        want = rt.adaptive_plan_host(vv, d, ORIGIN, budget, mn, mx, ff)
        assert int(want[3][0]) > 1024 * 1024 and (name == "no clamp") == (int(want[3][0]) == budget)
        assert_plan_equal(tracer.adaptive_plan(vv, d, ORIGIN, budget, mn, mx, ff), want, name)


@pytest.mark.parametrize("W,H", GPU_SIZES)
def test_merge_device_equals_host(rt, tracer, W, H):
    counts, offsets, p, _ = merge_inputs(W, H)
    for albedo, moments in ((True, True), (False, True), (False, False)):
        for max_history in (np.inf, 4.0):
            kw = dict(albedo=p["albedo"] if albedo else None, moments=p["moments"] if moments else None)
            want = rt.adaptive_merge_host(p["radiance"], counts, offsets, p["color"], p["history"], max_history, **kw)
            got = tracer.adaptive_merge(p["radiance"], counts, offsets, p["color"], p["history"], max_history, **kw)
            assert len(got) == len(want)
            for g, w, name in zip(got, want, ("out", "out_history", "out_moments")):
                assert R.same_bits(g, w).all(), (W, H, albedo, moments, max_history, name)
    color, hist, mom = p["color"].copy(), p["history"].copy(), p["moments"].copy()
    want = rt.adaptive_merge_host(p["radiance"], counts, offsets, p["color"], p["history"], 6.0, p["albedo"], p["moments"])
    got = tracer.adaptive_merge(p["radiance"], counts, offsets, color, hist, 6.0, p["albedo"], mom, out=color, out_history=hist, out_moments=mom)
    assert got[0] is color and got[1] is hist and got[2] is mom
    for g, w in zip(got, want):
        assert R.same_bits(g, w).all(), (W, H, "the outputs are the inputs")
    # counts and offsets that point past the list: nothing is read beyond it
    short = p["radiance"][:max(1, p["radiance"].shape[0] // 2)]
    want = rt.adaptive_merge_host(short, counts, offsets, p["color"], p["history"])
    for g, w in zip(tracer.adaptive_merge(short, counts, offsets, p["color"], p["history"]), want):
        assert R.same_bits(g, w).all(), (W, H, "a list shorter than the plan")


W, H = 67, 45


def _cornell(rt, tracer, cornell):
    tracer.load_scene(cornell)
    cam = cornell.uniform.camera
    g = tracer.render_gbuffer(rt.make_params(W, H, 1, 1), ("dir", "normal", "point", "albedo", "emission"))
    return g, np.asarray(cam.cam_to_world, F32)[3, :3].copy()


def test_uniform_plan_is_rt_render(rt, tracer, cornell):
    """min = max = N = 3, budget = N W H, history 0: plan -> rt_radiance_rays -> merge leaves what rt_render leaves after
    frames 0 .. 2, bit for bit, alpha included."""
    g, origin = _cornell(rt, tracer, cornell)
    for f in range(3):
        tracer.render(rt.make_params(W, H, 4, 8, skybox=1, frames=f))
    want = tracer.read_image(W, H).copy()
    out, hist, counts, totals = tracer.adaptive_samples(g, np.ones((H, W), F32), np.zeros((H, W, 4), F32), np.zeros((H, W), F32),
                                                        3 * W * H, 4, 8, origin, min_samples=3, max_samples=3)
    assert (counts == 3).all() and totals[0] == 3 * W * H and (hist == 3).all()
    assert R.same_bits(out, want).all()


def test_adaptive_samples_equals_the_host_pipeline(rt, tracer, cornell):
    """A pilot of 4 frames, its variance, 4 more rays per texel on average: adaptive_samples against plan_host -> the same
    radiance -> merge_host.  max_samples clamps some texels, so the list has a tail, which traces to zeros; then budgets one
    record and more than a block beyond the plan's total."""
    g, origin = _cornell(rt, tracer, cornell)
    for f in range(4):
        tracer.render(rt.make_params(W, H, 4, 8, skybox=1, frames=f))
    color = tracer.read_image(W, H).copy()
    hist = np.full((H, W), 4, F32)
    variance = tracer.denoise_variance(g, color, out_variance=True)[1]
    assert (variance > 0).mean() > 0.15
    moments = tracer.luminance_moments(g, color)
    budget = 4 * W * H
    counts, offsets, rays, totals = rt.adaptive_plan_host(variance, g["dir"], origin, budget, 1, 16, 4)
    total = int(totals[0])
    assert totals[2] > 0 and total < budget and counts.max() == 16 and counts.min() == 1
    radiance = tracer.radiance(rays["origin"], rays["dir"], rays["seed"], 4, 8)
    assert radiance.shape == (budget, 4) and not radiance[total:].view(U32).any(), "the tail traces to zeros"
    assert (radiance[:total, 3] != 0).any()
    want = rt.adaptive_merge_host(radiance, counts, offsets, color, hist, np.inf, g["albedo"], moments)
    got = tracer.adaptive_samples(g, variance, color, hist, budget, 4, 8, origin, first_frame=4, moments=moments)
    assert len(got) == 5
    for a, b, name in zip(got[:3], want, ("out", "out_history", "out_moments")):
        assert R.same_bits(a, b).all(), name
    assert np.array_equal(got[3], counts) and np.array_equal(got[4], totals) and np.array_equal(got[1], hist + counts)
    # budgets past the plan's total by one record and by more than a block: min = max leaves R unspent
    for extra in (1, 1500):
        budget = 2 * W * H + extra
        want = rt.adaptive_plan_host(np.zeros((H, W), F32), g["dir"], origin, budget, 2, 2, 0)
        got = tracer.adaptive_plan(np.zeros((H, W), F32), g["dir"], origin, budget, 2, 2, 0)
        assert_plan_equal(got, want, ("tail", extra))
        assert int(got[3][0]) == budget - extra and not got[2][budget - extra:].view(np.uint8).any()
        rad = tracer.radiance(got[2]["origin"], got[2]["dir"], got[2]["seed"], 2, 1)
        assert not rad[budget - extra:].view(U32).any() and (rad[:budget - extra, 3] != 0).any()


def _plan_raw(t, p, flags=A.ADAPTIVE_HOST_MEMORY, **over):
    d = A.AdaptivePlanDesc(struct_bytes=C.sizeof(A.AdaptivePlanDesc), width=p["variance"].shape[1], height=p["variance"].shape[0],
                           budget=p["rays"].shape[0], min_samples=1, max_samples=16)
    for k, v in p.items():
        setattr(d, k, v.ctypes.data)
    for k, v in over.items():
        setattr(d, k, v)
    return t._L.rt_adaptive_plan(t._h, C.byref(d), flags)


def _plan_planes(Wp, Hp, per_texel=3):
    rng = np.random.default_rng(9)
    return {"variance": rng.uniform(0, 2, (Hp, Wp)).astype(F32), "dir": rng.normal(0, 1, (Hp, Wp, 3)).astype(F32),
            "counts": np.full((Hp, Wp), 0xA5A5A5A5, U32), "offsets": np.full((Hp, Wp), 0xA5A5A5A5, U32),
            "rays": np.full((per_texel * Wp * Hp, 8), 0xA5A5A5A5, U32), "totals": np.full(4, 0xA5A5A5A5, U32)}


def _untouched(p):
    return all((p[k] == 0xA5A5A5A5).all() for k in ("counts", "offsets", "rays", "totals"))


def test_staging_is_capped_and_no_scene_is_needed(rt):
    """The host-memory path stages every plane through a temporary buffer that option max_device_mb bounds: without room,
    RT_ERR_OUT_OF_MEMORY and the outputs untouched; with room the host's bits, on a handle that never saw a scene.  (The
    scratch itself -- 32 bytes per 1024 texels -- shows in whole MiB only for a frame of 32 M texels:
    tests/_adaptive_device_path.py counts and caps it there, on device planes.)"""
    t = rt.RayTracer(device=0, max_width=16, max_height=16)
    try:
        before = t.last_launch()["device_mb_held"]
        p = _plan_planes(512, 256)                      # 12.6 MB of ray records alone
        t.set_option("max_device_mb", before + 4)
        assert _plan_raw(t, p) == -8 and b"max_device_mb" in t._L.rt_last_error(t._h) and _untouched(p)
        counts, offsets, m, _ = merge_inputs(512, 256)
        out = np.full((256, 512, 4), F32(-7.25))
        with pytest.raises(rt.RtError) as e:
            t.adaptive_merge(m["radiance"], counts, offsets, m["color"], m["history"], out=out)
        assert e.value.code == -8 and (out == F32(-7.25)).all()
        t.set_option("max_device_mb", 0)
        assert _plan_raw(t, p) == 0 and not _untouched(p)
        want = rt.adaptive_plan_host(p["variance"], p["dir"], (0, 0, 0), p["rays"].shape[0])
        assert np.array_equal(p["counts"], want[0]) and np.array_equal(p["offsets"], want[1]) and np.array_equal(p["totals"], want[3])
        assert np.array_equal(p["rays"].view(np.uint8).ravel(), want[2].view(np.uint8).ravel())
        assert t.last_launch()["device_mb_held"] <= before + 1     # (4.3 KB of scratch: at most the rounding moves)
        got = t.adaptive_merge(m["radiance"], counts, offsets, m["color"], m["history"], out=out)
        assert R.same_bits(got[0], rt.adaptive_merge_host(m["radiance"], counts, offsets, m["color"], m["history"])[0]).all()
    finally:
        t.close()


def test_no_side_effects(rt, tracer, cornell):
    """A render sequence with both calls between its frames: the image, rt_get_stats and the launch words as without."""
    p = _plan_planes(64, 48)
    counts, offsets, m, _ = merge_inputs(24, 16)

    def run(adaptive):
        tracer.set_option("frame_ahead", 8)
        tracer.load_scene(cornell)
        tracer.reset_timing()
        for f in range(8):
            tracer.render(rt.make_params(64, 48, 3, 2, skybox=1, frames=f))
            if adaptive:
                assert _plan_raw(tracer, p) == 0
                tracer.adaptive_merge(m["radiance"], counts, offsets, m["color"], m["history"], moments=m["moments"])
            else:
                tracer.synchronize()
        img = tracer.read_image(64, 48)
        s = tracer.stats()
        return img, (s.segments, s.paths, s.node_tests, s.triangle_tests, s.frames, s.segments_reused, s.frames_speculative), \
            tuple(tracer.last_launch().values())[:-2]

    try:
        a, sa, la = run(False)
        b, sb, lb = run(True)
        assert np.array_equal(a.view(U32), b.view(U32)) and sa == sb and la == lb, (sa, sb, la, lb)
    finally:
        tracer.set_option("frame_ahead", -1)


def test_errors(rt):
    """The argument errors on the device entry points, the device-only ones included; the outputs stay as they were."""
    t = rt.RayTracer(device=0, max_width=16, max_height=16)
    L, h = t._L, t._h

    def err():
        return L.rt_last_error(h).decode()

    try:
        p = _plan_planes(8, 6)
        assert L.rt_adaptive_plan(None, None, 1) == -1 and L.rt_adaptive_merge(None, None, 1) == -1
        assert L.rt_adaptive_plan(h, None, 1) == -1 and "null" in err()
        assert L.rt_adaptive_merge(h, None, 1) == -1 and "null" in err()
        for flags in (2, 3, -2):
            assert _plan_raw(t, p, flags=flags) == -1 and "flags" in err()
        for over, code, text in ((dict(struct_bytes=88), -1, "struct_bytes"), (dict(_p0=1), -1, "_p0"), (dict(_p1=1), -1, "_p1"),
                                 (dict(width=0), -1, "zero"), (dict(budget=0), -1, "budget"), (dict(max_samples=0), -1, "max_samples"),
                                 (dict(max_samples=65536), -1, "max_samples"), (dict(min_samples=17), -1, "min_samples"),
                                 (dict(min_samples=4), -1, "budget"), (dict(variance=None), -1, "null"), (dict(rays=None), -1, "null"),
                                 (dict(width=1 << 16, height=1 << 15, min_samples=0), -2, "2^31")):
            for flags in (0, 1):
                assert _plan_raw(t, p, flags=flags, **over) == code and text in err(), (over, flags, err())
        # device planes (host arrays' addresses stand in for device pointers: the checks come before any use)
        need = {"variance": 4, "dir": 4, "counts": 4, "offsets": 4, "rays": 16, "totals": 4}
        for c, a in need.items():
            for off in (1, 2, 4, 8):
                if off % a:
                    assert _plan_raw(t, p, flags=0, **{c: p[c].ctypes.data + off}) == -1 and f"plane {c} " in err() and "aligned" in err(), (c, off)
        assert _untouched(p)
        # the merge
        counts, offsets, m, _ = merge_inputs(8, 1)
        out, oh = np.full((1, 8, 4), F32(-7.25)), np.full((1, 8), F32(-7.25))

        def merge_raw(flags=1, **over):
            d = A.AdaptiveMergeDesc(struct_bytes=C.sizeof(A.AdaptiveMergeDesc), width=8, height=1, budget=m["radiance"].shape[0], max_history=4.0)
            for k, v in dict(radiance=m["radiance"], counts=counts, offsets=offsets, color=m["color"], history=m["history"], out=out,
                             out_history=oh).items():
                setattr(d, k, v.ctypes.data)
            for k, v in over.items():
                setattr(d, k, v)
            return L.rt_adaptive_merge(h, C.byref(d), flags)

        for over, code, text in ((dict(struct_bytes=96), -1, "struct_bytes"), (dict(_p0=1), -1, "_p0"), (dict(height=0), -1, "zero"),
                                 (dict(budget=0), -1, "budget"), (dict(max_history=0.5), -1, "max_history"),
                                 (dict(max_history=float("nan")), -1, "max_history"), (dict(radiance=None), -1, "null"),
                                 (dict(out=None), -1, "null"), (dict(moments=m["moments"].ctypes.data), -1, "go together"),
                                 (dict(out_moments=m["moments"].ctypes.data), -1, "go together"),
                                 (dict(width=1 << 16, height=1 << 15), -2, "2^31")):
            for flags in (0, 1):
                assert merge_raw(flags, **over) == code and text in err(), (over, flags, err())
        assert merge_raw(3) == -1 and "flags" in err()
        assert merge_raw(1, color=None) == -1 and "color" in err()
        assert merge_raw(0, color=None, width=17, height=16) == -2 and "image" in err()
        for c, a in (("radiance", 16), ("counts", 4), ("offsets", 4), ("color", 16), ("history", 4), ("out", 16), ("out_history", 4)):
            base = dict(radiance=m["radiance"], counts=counts, offsets=offsets, color=m["color"], history=m["history"], out=out, out_history=oh)[c]
            for off in (2, 4, 8):
                if off % a:
                    assert merge_raw(0, **{c: base.ctypes.data + off}) == -1 and f"plane {c} " in err() and "aligned" in err(), (c, off)
        assert (out == F32(-7.25)).all() and (oh == F32(-7.25)).all()
        assert merge_raw(1) == 0 and not (out == F32(-7.25)).any()
        want = rt.adaptive_merge_host(m["radiance"], counts, offsets, m["color"], m["history"], 4.0)
        assert R.same_bits(out, want[0]).all() and R.same_bits(oh, want[1]).all()
    finally:
        t.close()


def test_device_path():
    """Torch tensors on the device (tests/_adaptive_device_path.py, a process of its own that imports torch first)."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "_adaptive_device_path.py")],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "device path ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
