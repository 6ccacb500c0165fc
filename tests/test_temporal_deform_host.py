"""rt_temporal_accumulate_deforming_host and rt_object_motions_deforming (include/rt_abi.h; csrc/host/temporal.cpp over
csrc/rt_temporal.h, csrc/host/object_motions.cpp) against their independent numpy restatements (tests/
_temporal_deform_reference.py), bit for bit; a table without a deformed record against rt_temporal_accumulate_moving_host;
the stand-alone sanitizer driver (tests/cpp/temporal_deform_driver.cpp).  No device."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import _temporal_deform_reference as D
import _temporal_motion_reference as M
import _temporal_reference as R
from conftest import ROOT

F32 = np.float32
DEFAULTS = (0.01, 0.9)
NAMES = ("out", "out_history", "motion")


def _host(rt, planes, cam, motions, tris, first=D.TRI_FIRST, cap=np.inf, motion=True, **kw):
    g, pg = D.split(planes)
    return rt.temporal_accumulate_host(g, pg, cam, planes["prev_color"], planes["prev_history"], planes["color"], cap, *DEFAULTS,
                                       motion=motion, motions=motions, prev_triangles=tris, tri_first=first, **kw)


def _same(got, want, what):
    assert len(got) == len(want), what
    for a, b, name in zip(got, want, NAMES):
        bad = ~R.same_bits(a, b)
        assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def test_synthetic_case_meets_every_rule():
    """By the reference's own account, on the 37x19 frames: all four kinds of record find history; primitive words below and
    past the range, NaN and infinite barycentrics, the degenerate triangle, zero and NaN normals, words past the table and
    0xffffffff all give "no history"; both backface states are carried and find history; taps fall off every edge."""
    planes, cam, motions, tris, notes = D.synthetic_case()
    H, W = planes["object"].shape
    assert (W, H) == (37, 19) and len(tris) == 5 and motions["moved"].tolist() == [0, 1, 2, 2]
    st = {}
    out, hist, motion = D.reference(planes, cam, motions, tris, D.TRI_FIRST, 4.0, *DEFAULTS, stats=st)
    obj = planes["object"]
    for k in range(4):
        on = (obj == k) & st["reprojectable" if k < 2 else "deformed"]
        assert on.sum() > 100 and (st["have"] & on).mean() > 0.4 * on.mean(), k
        assert (hist[on] > 1).sum() > 60, k
    assert (st["table_still"] & (obj == 0)).sum() > 100 and (st["table_moved"] & (obj == 1)).sum() > 100
    assert not (st["table_moved"] & (obj >= 2)).any() and np.array_equal(st["deformed"], st["carried"] | st["deform_lost"])
    for face in ("backface", "frontface"):
        assert (st[face] & st["carried"] & st["have"]).sum() > 40, face
    for k, rule in (("below_range", "below_range"), ("past_range", "past_range"), ("degenerate", "zero_normal_length"),
                    ("nan_bary", "bary_bad"), ("inf_bary", "bary_bad")):
        y, x = notes[k]
        assert st[rule][y, x] and st["deform_lost"][y, x], k
        assert hist[y, x] == 1 and R.same_bits(out[y, x], planes["color"][y, x]).all() and np.isnan(motion[y, x]).all(), k
    assert st["past_range"].sum() >= 2 and st["bary_bad"].sum() == 4 and st["deform_normal_bad"].sum() >= 2
    for k in ("zero_normal", "nan_normal", "no_object"):
        y, x = notes[k]
        assert not st["reprojectable"][y, x] and not st["deformed"][y, x] and hist[y, x] == 1 and np.isnan(motion[y, x]).all(), k
    y, x = notes["past_table"]
    assert st["outside_table"][y, x] and st["outside_table"].sum() == 2 and hist[y, x] == 1
    for k in ("left_edge", "right_edge", "bottom_edge", "top_edge"):
        y, x = notes[k]
        assert st["carried"][y, x] and st["on_screen"][y, x] and st["outside"][y, x], k
    y, x = notes["off_left"]
    assert st["carried"][y, x] and st["left"][y, x] and np.isnan(motion[y, x]).all()
    y, x = notes["one_tap"]
    assert st["carried"][y, x] and st["valid_taps"][y, x] == 1 and st["snap_x_down"][y, x] and st["snap_y_down"][y, x]
    for k in ("prev_miss", "prev_nan", "history_low", "object", "dropped_sample", "capped", "plane", "normal"):
        assert st[k].any(), k
    # the G-buffer's own point and normal of a deformed texel are not what finds the history: without the triangle side
    # (the deformed records read as rigid ones, as rt_temporal_accumulate_moving reads them) far fewer do
    rigid = {}
    M.reference(planes, cam, motions, 4.0, *DEFAULTS, stats=rigid)
    assert (rigid["have"] & st["deformed"]).sum() < 0.5 * (st["have"] & st["deformed"]).sum()


@pytest.mark.parametrize("objects,motion,cap", list(itertools.product((True, False), (True, False), (4.0, np.inf))))
def test_synthetic_frame_equals_the_reference(rt, objects, motion, cap):
    planes, cam, motions, tris, _ = D.synthetic_case()
    if not objects:
        planes = {k: v for k, v in planes.items() if k != "prev_object"}
    want = D.reference(planes, cam, motions, tris, D.TRI_FIRST, cap, *DEFAULTS)
    got = _host(rt, planes, cam, motions, tris, cap=cap, motion=motion)
    assert len(got) == (3 if motion else 2)
    _same(got, want[:len(got)], (objects, motion, cap))


@pytest.mark.parametrize("W,H", [(70, 21), (1, 1), (5, 1)])
def test_other_sizes_equal_the_reference(rt, W, H):
    planes, cam, motions, tris, _ = D.synthetic_case(W, H) if (W, H) == (70, 21) else _tiny(W, H)
    want = D.reference(planes, cam, motions, tris, D.TRI_FIRST, 6.0, *DEFAULTS)
    _same(_host(rt, planes, cam, motions, tris, cap=6.0), want, (W, H))


def _tiny(W, H):
    """A W x H cut of the 37x19 case's deformed band (the frame's size enters the projection: only equality is asked)."""
    planes, cam, motions, tris, notes = D.synthetic_case()
    x2 = notes["below_range"][1]
    cut = {k: np.ascontiguousarray(v[2:2 + H, x2:x2 + W]) for k, v in planes.items()}
    return cut, cam, motions, tris, notes


def test_without_a_deformed_record_it_is_the_moving_call(rt):
    """Consequence (a): no record of moved == 2 -- the deformed ones turned into rigid ones of moved 1 and 3 -- and every
    output plane is rt_temporal_accumulate_moving_host's bit for bit, whatever primitive, bary, flags and the triangles hold."""
    planes, cam, motions, tris, _ = D.synthetic_case()
    g, pg = D.split(planes)
    t = motions.copy()
    t["moved"][2], t["moved"][3] = 1, 3
    rng = np.random.default_rng(3)
    junk = tris.copy()
    junk.view(np.uint32)[:] = rng.integers(0, 1 << 32, junk.view(np.uint32).shape, dtype=np.uint64).astype(np.uint32)
    poisoned = dict(planes, primitive=rng.integers(0, 1 << 32, planes["primitive"].shape, dtype=np.uint64).astype(np.uint32),
                    bary=np.full(planes["bary"].shape, np.nan, F32), flags=rng.integers(0, 256, planes["flags"].shape).astype(np.uint8))
    for cap, objects in itertools.product((3.0, np.inf), (True, False)):
        drop = (lambda p: p) if objects else (lambda p: {k: v for k, v in p.items() if k != "prev_object"})
        gg, pgg = D.split(drop(planes))
        want = rt.temporal_accumulate_host({k: gg[k] for k in ("point", "normal", "object")}, pgg, cam, planes["prev_color"],
                                           planes["prev_history"], planes["color"], cap, *DEFAULTS, motion=True, motions=t)
        for p, tr in ((planes, tris), (poisoned, junk)):
            _same(_host(rt, drop(p), cam, t, tr, cap=cap), want, (cap, objects))
    assert (want[1] > 1).mean() > 0.3
    # ... and the moving call still reads a 2 as "moved": the new call's results differ from it on the deformed texels
    there = _host(rt, planes, cam, motions, tris)
    moving = rt.temporal_accumulate_host({k: g[k] for k in ("point", "normal", "object")}, pg, cam, planes["prev_color"],
                                         planes["prev_history"], planes["color"], np.inf, *DEFAULTS, motion=True, motions=motions)
    deformed = planes["object"] >= 2
    assert not R.same_bits(there[1], moving[1])[deformed].all() and R.same_bits(there[1], moving[1])[~deformed].all()


def test_out_may_be_color(rt):
    planes, cam, motions, tris, _ = D.synthetic_case()
    want = _host(rt, planes, cam, motions, tris, cap=4.0)
    buf = planes["color"].copy()
    hist = np.zeros(buf.shape[:2], F32)
    got = _host(rt, dict(planes, color=buf), cam, motions, tris, cap=4.0, out=buf, out_history=hist)
    assert got[0] is buf and got[1] is hist
    _same(got, want, "out is color")


def test_object_motions_deforming_equals_its_restatement(rt, cornell):
    """The Cornell arrays with two boxes moved, meshes 2 and 5 marked deformed (5 moved as well: its record holds the PREVIOUS
    model_to_world); indices and a boolean array name the same table; no mark is rt_object_motions byte for byte."""
    moved = M.moved_mesh(cornell, {5: M.rigid((0.06, 0.0, 0.02), 0.05, M.centroid(cornell, 5)), 6: M.rigid((-0.04, 0.0, 0.03), -0.08, M.centroid(cornell, 6))})
    nm = len(cornell.meshes)
    marks = np.zeros(nm, bool)
    marks[[2, 5]] = True
    want = D.object_motions(cornell.meshes, moved.meshes, cornell.spheres, moved.spheres, marks)
    for deformed in ([2, 5], (5, 2), marks, np.array([2, 5], np.uint32)):
        got = rt.object_motions(cornell, moved, deformed=deformed)
        assert got.dtype == want.dtype and got.shape == want.shape == (nm + len(cornell.spheres),)
        assert got.tobytes() == want.tobytes()
    assert got["moved"].tolist()[:7] == [0, 0, 2, 0, 0, 2, 1]
    for k in (2, 5):
        assert np.array_equal(got["d"][k], cornell.meshes["model_to_world"][k][:, :3])
        assert np.array_equal(got["nt"][k], cornell.meshes["model_to_world"][k][:3, :3]) and not got["_p"][k].any()
    plain = rt.object_motions(cornell, moved)
    for deformed in ([], np.zeros(nm, bool)):
        assert rt.object_motions(cornell, moved, deformed=deformed).tobytes() == plain.tobytes()
    rest = np.ones(len(got), bool)
    rest[[2, 5]] = False
    assert got[rest].tobytes() == plain[rest].tobytes()
    for bad in ([nm], [-1], np.zeros(nm + 1, bool)):
        with pytest.raises(ValueError):
            rt.object_motions(cornell, moved, deformed=bad)
    # spheres only: nothing to mark
    none = cornell.meshes[:0]
    s = np.zeros(2, cornell.spheres.dtype)
    s["radius"] = 1
    scene = type(cornell)(cornell.uniform, s, none, cornell.triangles, cornell.nodes)
    assert rt.object_motions(scene, scene, deformed=[]).tobytes() == rt.object_motions(scene, scene).tobytes()


def test_sanitizer_driver(rt, tmp_path):
    """tests/cpp/temporal_deform_driver.cpp with host/temporal.cpp under AddressSanitizer and UndefinedBehaviorSanitizer, a
    program of its own: the 37x19 case from a file of this test's planes, exactly sized heap buffers, and a 1x1 frame; its
    outputs are the wrapper's bit for bit."""
    csrc = os.path.join(ROOT, "ray_tracer_2_amd", "csrc")
    exe = tmp_path / "temporal_deform_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "temporal_deform_driver.cpp"),
                    os.path.join(csrc, "host", "temporal.cpp"), "-o", str(exe)], check=True)
    from ray_tracer_2_amd import _abi as A
    planes, cam, motions, tris, _ = D.synthetic_case()
    H, W = planes["object"].shape
    order = [k for k in A.TEMPORAL_DEFORM_PLANES if k in planes]
    assert order == ["color", "point", "normal", "object", "prev_color", "prev_history", "prev_point", "prev_normal", "prev_object",
                     "primitive", "bary", "flags"]
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        f.write(np.array([W, H, len(motions), len(tris), D.TRI_FIRST], np.uint32).tobytes())
        f.write(bytes(cam))
        f.write(np.array([4.0, *DEFAULTS], F32).tobytes())
        for k in order:
            f.write(np.ascontiguousarray(planes[k]).tobytes())
        f.write(motions.tobytes())
        f.write(tris.tobytes())
    res = tmp_path / "out.bin"
    run = subprocess.run([str(exe), str(path), str(res)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout, run.stderr)
    assert "37x19 ok" in run.stdout and "1x1 ok" in run.stdout, run.stdout
    raw = np.fromfile(res, F32)
    n = W * H
    got = raw[:4 * n].reshape(H, W, 4), raw[4 * n:5 * n].reshape(H, W), raw[5 * n:7 * n].reshape(H, W, 2)
    assert raw.size == 7 * n
    _same(got, _host(rt, planes, cam, motions, tris, cap=4.0), "driver")
