"""rt_temporal_deform_desc of include/rt_abi.h against the ctypes struct of ray_tracer_2_amd._abi, as the host compiler lays
it out; the bindings; every argument error that needs no device, on rt_temporal_accumulate_deforming_host and
rt_object_motions_deforming, with the outputs left as they were and a reason in rt_last_error."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

MOTION_FIELDS = ["struct_bytes", "_p0", "width", "height", "prev_camera", "max_history", "point_tolerance", "normal_cos", "color",
                 "point", "normal", "object", "prev_color", "prev_history", "prev_point", "prev_normal", "prev_object", "out",
                 "out_history", "motion", "motions", "n_objects", "_p1"]
SIDE = ["primitive", "bary", "flags", "prev_triangles", "tri_first", "n_prev_triangles"]
FIELDS = MOTION_FIELDS + SIDE
INVALID, CAPACITY = -1, -2
MARK = np.float32(-7.25)


def test_header_layout_matches_the_ctypes_struct(rt, tmp_path):
    from ray_tracer_2_amd import _abi as A
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_abi.h"', "int main(void) {",
             '    printf("size %zu %zu %zu\\n", sizeof(rt_temporal_deform_desc), sizeof(rt_temporal_motion_desc), sizeof(rt_packed_triangle));']
    for f in FIELDS:
        lines.append(f'    printf("{f} %zu %zu\\n", offsetof(rt_temporal_deform_desc, {f}), sizeof(((rt_temporal_deform_desc*)0)->{f}));')
    for f in MOTION_FIELDS:
        lines.append(f'    printf("head.{f} %zu %zu\\n", offsetof(rt_temporal_motion_desc, {f}), sizeof(((rt_temporal_motion_desc*)0)->{f}));')
    lines += ["    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c11", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in out if l}
    assert got["size"] == [C.sizeof(A.TemporalDeformDesc), C.sizeof(A.TemporalMotionDesc), A.TRI_DTYPE.itemsize] == [264, 224, 96]
    assert [n for n, _ in A.TemporalDeformDesc._fields_] == FIELDS
    for f in FIELDS:
        d = getattr(A.TemporalDeformDesc, f)
        assert got[f] == [d.offset, d.size], f
    for f in MOTION_FIELDS:   # rt_temporal_motion_desc's fields in their order, at their offsets
        assert got[f] == got["head." + f], f
    assert got["primitive"][0] == 224 and got["tri_first"] == [256, 4] and got["n_prev_triangles"] == [260, 4]
    assert list(A.TEMPORAL_DEFORM_PLANES) == list(A.TEMPORAL_MOTION_PLANES) + SIDE[:4]
    assert A.TEMPORAL_DEFORM_PLANES["flags"] == ("u1", 0) and A.TEMPORAL_DEFORM_PLANES["prev_triangles"][0] == A.TRI_DTYPE
    assert A.OBJECT_DEFORMED == 2


def test_the_calls_are_declared_and_bound(rt):
    from ray_tracer_2_amd.lib import EXPORTS
    L = rt.load()
    header = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    for name, nargs in (("rt_temporal_accumulate_deforming", 3), ("rt_temporal_accumulate_deforming_host", 1), ("rt_object_motions_deforming", 8)):
        assert name in EXPORTS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == nargs and getattr(L, name).restype is C.c_int
        assert f"int {name}(" in header
    for fn in (rt.temporal_accumulate_host, rt.RayTracer.temporal_accumulate):
        p = inspect.signature(fn).parameters
        assert p["prev_triangles"].default is None and p["tri_first"].default == 0
    assert inspect.signature(rt.object_motions).parameters["deformed"].default is None


W, H = 6, 4
FIRST = 3


def _planes():
    """Every texel a deformed one that finds its history: the triangle lies in the previous points' plane."""
    from ray_tracer_2_amd import _abi as A
    rng = np.random.default_rng(5)
    p = {}
    for k, (dt, n) in A.TEMPORAL_PLANES.items():
        shape = (H, W, n) if n else (H, W)
        p[k] = np.ones(shape, np.uint32) if dt == "<u4" else rng.uniform(0.5, 2, shape).astype(np.float32)
    p["normal"][:] = (0, 1, 0)            # (the G-buffer's own normal and point of a deformed texel are not used)
    p["point"][:] = (5, 5, 5)
    p["prev_normal"][:] = (0, 0, -1)
    p["prev_point"][:] = (0, 0, 3)
    for k in ("out", "out_history", "motion"):
        p[k][:] = MARK
    t = np.zeros(2, A.OBJECT_MOTION_DTYPE)
    t["d"][:, :3] = np.eye(3, dtype=np.float32)
    t["nt"][:] = np.eye(3, dtype=np.float32)
    t["moved"][1] = 2
    p["motions"] = t
    p["primitive"] = np.full((H, W), FIRST + 1, np.uint32)
    p["bary"] = np.zeros((H, W, 2), np.float32)
    p["bary"][:] = (0.25, 0.5)
    p["flags"] = np.ones((H, W), np.uint8)
    tri = np.zeros(2, A.TRI_DTYPE)
    tri["v1"], tri["v2"], tri["v3"] = (-1, -2, 3), (4, 0, 3), (-1.5, 1, 3)      # (u, v) = (0.25, 0.5) is (0, 0, 3)
    tri["n1"] = tri["n2"] = tri["n3"] = (0, 0, -1)
    p["prev_triangles"] = tri
    return p


def _desc(A, p, **over):
    cam = A.CameraUniform()
    for i in range(4):
        cam.cam_to_world[i][i] = 1.0
    cam.view_params[:] = (1.2, 0.8, 1.5)
    d = A.TemporalDeformDesc(struct_bytes=C.sizeof(A.TemporalDeformDesc), width=W, height=H, prev_camera=cam, max_history=8.0,
                             point_tolerance=0.01, normal_cos=0.9, n_objects=len(p["motions"]), tri_first=FIRST,
                             n_prev_triangles=len(p["prev_triangles"]))
    for k, v in p.items():
        setattr(d, k, v.ctypes.data)
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _untouched(p):
    return all(np.all(p[k] == MARK) for k in ("out", "out_history", "motion"))


CASES = [
    ("struct_bytes of rt_temporal_motion_desc", dict(struct_bytes=224), INVALID, "struct_bytes"),
    ("struct_bytes of rt_temporal_desc", dict(struct_bytes=208), INVALID, "struct_bytes"),
    ("struct_bytes zero", dict(struct_bytes=0), INVALID, "struct_bytes"),
    ("struct_bytes too large", dict(struct_bytes=272), INVALID, "struct_bytes"),
    ("_p0", dict(_p0=1), INVALID, "_p0"),
    ("_p1", dict(_p1=1), INVALID, "_p1"),
    ("zero width", dict(width=0), INVALID, "zero"),
    ("zero height", dict(height=0), INVALID, "zero"),
    ("max_history below 1", dict(max_history=0.5), INVALID, "max_history"),
    ("max_history NaN", dict(max_history=float("nan")), INVALID, "max_history"),
    ("point_tolerance zero", dict(point_tolerance=0.0), INVALID, "point_tolerance"),
    ("point_tolerance NaN", dict(point_tolerance=float("nan")), INVALID, "point_tolerance"),
    ("point_tolerance infinite", dict(point_tolerance=float("inf")), INVALID, "point_tolerance"),
    ("normal_cos NaN", dict(normal_cos=float("nan")), INVALID, "normal_cos"),
    ("normal_cos above 1", dict(normal_cos=1.5), INVALID, "normal_cos"),
    ("normal_cos below -1", dict(normal_cos=-1.5), INVALID, "normal_cos"),
    ("null color", dict(color=None), INVALID, "color"),
    ("null point", dict(point=None), INVALID, "null"),
    ("null normal", dict(normal=None), INVALID, "null"),
    ("null object", dict(object=None), INVALID, "object"),
    ("null prev_color", dict(prev_color=None), INVALID, "null"),
    ("null prev_history", dict(prev_history=None), INVALID, "null"),
    ("null prev_point", dict(prev_point=None), INVALID, "null"),
    ("null prev_normal", dict(prev_normal=None), INVALID, "null"),
    ("null out", dict(out=None), INVALID, "null"),
    ("null out_history", dict(out_history=None), INVALID, "null"),
    ("null motions", dict(motions=None), INVALID, "motions"),
    ("no objects", dict(n_objects=0), INVALID, "n_objects"),
    ("null primitive", dict(primitive=None), INVALID, "primitive"),
    ("null bary", dict(bary=None), INVALID, "bary"),
    ("null flags", dict(flags=None), INVALID, "flags"),
    ("null prev_triangles", dict(prev_triangles=None), INVALID, "prev_triangles"),
    ("no previous triangles", dict(n_prev_triangles=0), INVALID, "n_prev_triangles"),
    ("triangle range past 2^32", dict(tri_first=0xFFFFFFFF, n_prev_triangles=2), INVALID, "2^32"),
    ("triangle range far past 2^32", dict(tri_first=0xFFFFFFFF, n_prev_triangles=0xFFFFFFFF), INVALID, "2^32"),
    ("2^31 texels", dict(width=1 << 16, height=1 << 15), CAPACITY, "2^31"),
]


@pytest.mark.parametrize("what,over,code,text", CASES, ids=[c[0] for c in CASES])
def test_errors_leave_the_outputs_untouched(rt, what, over, code, text):
    from ray_tracer_2_amd import _abi as A
    L = rt.load()
    p = _planes()
    assert L.rt_temporal_accumulate_deforming_host(C.byref(_desc(A, p, **over))) == code, what
    reason = L.rt_last_error(None).decode()
    assert reason and text in reason, (what, reason)
    assert _untouched(p), what


def test_null_desc_and_the_call_that_is_right(rt):
    from ray_tracer_2_amd import _abi as A
    L = rt.load()
    assert L.rt_temporal_accumulate_deforming_host(None) == INVALID and "null" in L.rt_last_error(None).decode()
    p = _planes()
    assert L.rt_temporal_accumulate_deforming_host(C.byref(_desc(A, p))) == 0
    assert not any(np.any(p[k] == MARK) for k in ("out", "out_history", "motion"))
    assert np.all(p["out_history"] > 1)
    # the range may end exactly at 2^32 (the words of this frame are then outside it: no history anywhere)
    q = _planes()
    assert L.rt_temporal_accumulate_deforming_host(C.byref(_desc(A, q, tri_first=0xFFFFFFFE))) == 0
    assert np.all(q["out_history"] == 1) and np.isnan(q["motion"]).all() and np.array_equal(q["out"], q["color"])
    # a range of one triangle leaves the frame's word outside it
    q = _planes()
    assert L.rt_temporal_accumulate_deforming_host(C.byref(_desc(A, q, n_prev_triangles=1))) == 0
    assert np.all(q["out_history"] == 1) and np.isnan(q["motion"]).all()
    # the optional planes may be NULL; nothing needs an alignment on the host
    for over in (dict(prev_object=None), dict(prev_object=None, motion=None), dict(max_history=float("inf"))):
        q = _planes()
        assert L.rt_temporal_accumulate_deforming_host(C.byref(_desc(A, q, **over))) == 0, over
        assert not np.any(q["out"] == MARK) and np.all(q["out_history"] > 1), over
    q = _planes()
    over = {}
    keep = []
    for k in ("prev_triangles", "primitive", "bary", "motions"):
        raw = np.zeros(q[k].nbytes + 8, np.uint8)
        off = 1 if k == "prev_triangles" else 4
        raw[off:off + q[k].nbytes] = q[k].view(np.uint8).ravel()
        keep.append(raw)
        over[k] = raw.ctypes.data + off
    assert L.rt_temporal_accumulate_deforming_host(C.byref(_desc(A, q, **over))) == 0
    assert np.array_equal(q["out"], p["out"]) and np.array_equal(q["out_history"], p["out_history"])


def test_object_motions_deforming_refuses_null_arrays(rt):
    from ray_tracer_2_amd import _abi as A
    L = rt.load()
    m, s = np.zeros(2, A.MESH_DTYPE), np.zeros(3, A.SPHERE_DTYPE)
    s["radius"] = 1
    marks = np.array([0, 1], np.uint8)
    out = np.full(5 * 24, MARK, np.float32)
    mp, sp, op, kp = m.ctypes.data, s.ctypes.data, out.ctypes.data, marks.ctypes.data
    for args in ((mp, mp, 2, sp, sp, 3, None, op), (None, mp, 2, sp, sp, 3, kp, op), (mp, None, 2, sp, sp, 3, kp, op), (mp, mp, 2, None, sp, 3, kp, op),
                 (mp, mp, 2, sp, None, 3, kp, op), (mp, mp, 2, sp, sp, 3, kp, None), (None, None, 0, sp, sp, 3, None, None)):
        assert L.rt_object_motions_deforming(*args) == INVALID, args
        assert np.all(out == MARK)
    assert L.rt_object_motions_deforming(None, None, 0, None, None, 0, None, None) == 0
    assert L.rt_object_motions_deforming(None, None, 0, sp, sp, 3, None, op) == 0 and np.all(out[:72] != MARK) and np.all(out[72:] == MARK)
    assert L.rt_object_motions_deforming(mp, mp, 2, None, None, 0, kp, op) == 0
    assert out.view(np.uint32)[21] == 0 and out.view(np.uint32)[24 + 21] == 2


def test_wrappers_check_their_arguments(rt):
    from ray_tracer_2_amd import _abi as A
    p = _planes()
    cam = _desc(A, p).prev_camera
    g = {k: p[k] for k in ("point", "normal", "object", "primitive", "bary", "flags")}
    pg = {k[5:]: p[k] for k in ("prev_point", "prev_normal", "prev_object")}
    t, tri = p["motions"], p["prev_triangles"]
    args = (pg, cam, p["prev_color"], p["prev_history"], p["color"])
    out, hist, motion = rt.temporal_accumulate_host(g, *args, motion=True, motions=t, prev_triangles=tri, tri_first=FIRST)
    assert out.shape == (H, W, 4) and out.dtype == np.float32 and np.all(hist > 1) and motion.shape == (H, W, 2)
    # every texel is carried exactly onto prev_point: the call without a table on those points and normals, bit for bit
    there = rt.temporal_accumulate_host(dict(g, point=p["prev_point"], normal=p["prev_normal"]), *args, motion=True)
    for a, b in zip((out, hist, motion), there):
        assert np.array_equal(a, b)
    # tri_first defaults to 0: the frame's word 4 is then outside the two triangles
    assert np.all(rt.temporal_accumulate_host(g, *args, motions=t, prev_triangles=tri)[1] == 1)
    # a (n, 24) float32 view is not the packed dtype; bytes that are reinterpreted are
    assert np.array_equal(rt.temporal_accumulate_host(g, *args, motions=t, prev_triangles=tri.copy(), tri_first=FIRST)[1], hist)
    for bad in (dict(prev_triangles=tri),                                                      # no table
                dict(motions=t, prev_triangles=tri[:0]), dict(motions=t, prev_triangles=tri.view(np.float32).reshape(-1, 24)),
                dict(motions=t, prev_triangles=tri, tri_first=-1), dict(motions=t, prev_triangles=tri, tri_first=(1 << 32) - 1)):
        with pytest.raises(ValueError):
            rt.temporal_accumulate_host(g, *args, **bad)
    for missing in ("primitive", "bary", "flags", "object"):
        with pytest.raises(ValueError):
            rt.temporal_accumulate_host({k: v for k, v in g.items() if k != missing}, *args, motions=t, prev_triangles=tri, tri_first=FIRST)
    with pytest.raises(ValueError):
        rt.temporal_accumulate_host(g, pg, cam, p["prev_color"], p["prev_history"], None, motions=t, prev_triangles=tri, tri_first=FIRST)
    with pytest.raises(rt.RtError) as e:
        rt.temporal_accumulate_host(g, *args, max_history=0.0, motions=t, prev_triangles=tri, tri_first=FIRST)
    assert e.value.code == INVALID
    tr = rt.RayTracer.__new__(rt.RayTracer)   # (no handle: the checks come before any library call)
    tr._L, tr._h, tr.device = None, None, 0
    with pytest.raises(ValueError):
        tr.temporal_accumulate({k: v for k, v in g.items() if k != "bary"}, *args, motions=t, prev_triangles=tri, tri_first=FIRST)
    with pytest.raises(ValueError):
        tr.temporal_accumulate(g, *args, prev_triangles=tri)
