"""rt_rectify_desc of include/rt_abi.h against the ctypes struct of ray_tracer_2_amd._abi, as the host compiler lays it out;
the bindings; every argument error that needs no device, on rt_temporal_rectify_host, with the outputs left as they were."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

FIELDS = ["struct_bytes", "_p0", "width", "height", "radius", "clip_sigma", "clip_history", "_p1", "color", "history", "history_length",
          "object", "moments", "history_moments", "out", "out_history", "out_moments", "out_clipped"]
INVALID, CAPACITY = -1, -2
MARK = np.float32(-7.25)
W, H = 7, 5
OUTPUTS = ("out", "out_history", "out_moments", "out_clipped")


def test_header_layout_matches_the_ctypes_struct(rt, tmp_path):
    from ray_tracer_2_amd import _abi as A
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_abi.h"', "int main(void) {",
             '    printf("size %zu\\n", sizeof(rt_rectify_desc));']
    for f in FIELDS:
        lines.append(f'    printf("{f} %zu %zu\\n", offsetof(rt_rectify_desc, {f}), sizeof(((rt_rectify_desc*)0)->{f}));')
    lines += ['    printf("flag %d\\n", RT_RECTIFY_HOST_MEMORY);', "    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c11", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in out if l}
    assert got["size"] == [C.sizeof(A.RectifyDesc)] == [112]
    assert [n for n, _ in A.RectifyDesc._fields_] == FIELDS
    for f in FIELDS:
        d = getattr(A.RectifyDesc, f)
        assert got[f] == [d.offset, d.size], f
    assert got["flag"] == [A.RECTIFY_HOST_MEMORY]
    assert list(A.RECTIFY_PLANES) == FIELDS[8:]
    assert (A.RECTIFY_NO_HISTORY, A.RECTIFY_KEPT, A.RECTIFY_CLIPPED) == (0, 1, 2)


def test_the_calls_are_declared_and_bound(rt):
    from ray_tracer_2_amd.lib import EXPORTS
    L = rt.load()
    header = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    for name, nargs in (("rt_temporal_rectify", 3), ("rt_temporal_rectify_host", 1)):
        assert name in EXPORTS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == nargs and getattr(L, name).restype is C.c_int
        assert f"int {name}(" in header
    for f in (rt.temporal_rectify_host, rt.temporal_reproject_host, rt.RayTracer.temporal_rectify, rt.RayTracer.temporal_reproject):
        assert callable(f)


def _planes():
    rng = np.random.default_rng(5)
    f = lambda *s: rng.uniform(0.5, 2, s).astype(np.float32)   # noqa: E731
    return dict(color=f(H, W, 4), history=f(H, W, 4), history_length=np.full((H, W), 3, np.float32), object=np.ones((H, W), np.uint32),
                moments=f(H, W, 4), history_moments=f(H, W, 4), out=np.full((H, W, 4), MARK), out_history=np.full((H, W), MARK),
                out_moments=np.full((H, W, 4), MARK), out_clipped=np.full((H, W), 0xA5, np.uint8))


def _desc(A, p, **over):
    d = A.RectifyDesc(struct_bytes=C.sizeof(A.RectifyDesc), width=W, height=H, radius=3, clip_sigma=1.0, clip_history=4.0)
    for k, v in p.items():
        setattr(d, k, v.ctypes.data)
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _untouched(p):
    return bool(all(np.all(p[k] == MARK) for k in OUTPUTS[:3]) and np.all(p["out_clipped"] == 0xA5))


NAN, INF = float("nan"), float("inf")
CASES = [
    ("struct_bytes too small", dict(struct_bytes=104), INVALID, "struct_bytes"),
    ("struct_bytes zero", dict(struct_bytes=0), INVALID, "struct_bytes"),
    ("struct_bytes too large", dict(struct_bytes=120), INVALID, "struct_bytes"),
    ("_p0", dict(_p0=1), INVALID, "_p0"),
    ("_p1", dict(_p1=1), INVALID, "_p1"),
    ("zero width", dict(width=0), INVALID, "zero"),
    ("zero height", dict(height=0), INVALID, "zero"),
    ("radius 0", dict(radius=0), INVALID, "radius"),
    ("radius 4", dict(radius=4), INVALID, "radius"),
    ("radius -1", dict(radius=0xFFFFFFFF), INVALID, "radius"),
    ("clip_sigma negative", dict(clip_sigma=-0.5), INVALID, "clip_sigma"),
    ("clip_sigma NaN", dict(clip_sigma=NAN), INVALID, "clip_sigma"),
    ("clip_sigma -inf", dict(clip_sigma=-INF), INVALID, "clip_sigma"),
    ("clip_history below 1", dict(clip_history=0.5), INVALID, "clip_history"),
    ("clip_history zero", dict(clip_history=0.0), INVALID, "clip_history"),
    ("clip_history NaN", dict(clip_history=NAN), INVALID, "clip_history"),
    ("null color", dict(color=None), INVALID, "color"),
    ("null history", dict(history=None), INVALID, "null"),
    ("null history_length", dict(history_length=None), INVALID, "null"),
    ("null out", dict(out=None), INVALID, "null"),
    ("null out_history", dict(out_history=None), INVALID, "null"),
    ("no moments", dict(moments=None), INVALID, "moments"),
    ("no history_moments", dict(history_moments=None), INVALID, "moments"),
    ("no out_moments", dict(out_moments=None), INVALID, "moments"),
    ("moments alone", dict(history_moments=None, out_moments=None), INVALID, "moments"),
    ("history_moments alone", dict(moments=None, out_moments=None), INVALID, "moments"),
    ("out_moments alone", dict(moments=None, history_moments=None), INVALID, "moments"),
    ("2^31 texels", dict(width=1 << 16, height=1 << 15), CAPACITY, "2^31"),
    ("more than 2^31 texels", dict(width=0x7fffffff, height=2), CAPACITY, "2^31"),
]


@pytest.mark.parametrize("what,over,code,text", CASES, ids=[c[0] for c in CASES])
def test_errors_leave_the_outputs_untouched(rt, what, over, code, text):
    from ray_tracer_2_amd import _abi as A
    L = rt.load()
    p = _planes()
    assert L.rt_temporal_rectify_host(C.byref(_desc(A, p, **over))) == code, what
    assert text in L.rt_last_error(None).decode(), (what, L.rt_last_error(None))
    assert _untouched(p), what


def test_out_must_not_overlap_color(rt):
    from ray_tracer_2_amd import _abi as A
    L = rt.load()
    p = _planes()
    before = p["color"].copy()
    # out is color; out begins inside color; color begins inside out (the last texel of out is the first of color)
    n = H * W
    two = np.full((2 * n, 4), MARK)
    for over in (dict(out=p["color"].ctypes.data), dict(out=p["color"].ctypes.data + 16 * (n - 1)),
                 dict(out=p["color"].ctypes.data - 16 * (n - 1)), dict(out=two.ctypes.data, color=two.ctypes.data + 16 * (n - 1))):
        assert L.rt_temporal_rectify_host(C.byref(_desc(A, p, **over))) == INVALID, over
        assert "overlaps" in L.rt_last_error(None).decode()
        assert _untouched(p) and np.array_equal(p["color"], before) and np.all(two == MARK)
    # ... and planes that touch without sharing a byte are fine
    two[n:] = before.reshape(-1, 4)
    assert L.rt_temporal_rectify_host(C.byref(_desc(A, p, out=two.ctypes.data, color=two.ctypes.data + 16 * n))) == 0
    q = _planes()
    assert L.rt_temporal_rectify_host(C.byref(_desc(A, q))) == 0
    assert np.array_equal(two[:n].view(np.uint32), q["out"].reshape(-1, 4).view(np.uint32)) and np.array_equal(two[n:], before.reshape(-1, 4))


def test_null_desc_and_the_call_that_is_right(rt):
    from ray_tracer_2_amd import _abi as A
    L = rt.load()
    assert L.rt_temporal_rectify_host(None) == INVALID and "null" in L.rt_last_error(None).decode()
    p = _planes()
    assert L.rt_temporal_rectify_host(C.byref(_desc(A, p))) == 0
    assert not any(np.any(p[k] == MARK) for k in OUTPUTS[:3]) and np.all((p["out_clipped"] == 1) | (p["out_clipped"] == 2))
    # the optional planes may be NULL; clip_sigma may be 0 or +INF, clip_history 1 or +INF; every radius
    none = dict(moments=None, history_moments=None, out_moments=None)
    for over in (dict(object=None), none, dict(out_clipped=None), dict(none, object=None, out_clipped=None), dict(clip_sigma=0.0),
                 dict(clip_sigma=INF), dict(clip_history=1.0), dict(clip_history=INF), dict(radius=1), dict(radius=2)):
        q = _planes()
        assert L.rt_temporal_rectify_host(C.byref(_desc(A, q, **over))) == 0, over
        assert not np.any(q["out"] == MARK) and not np.any(q["out_history"] == MARK), over
        assert np.all(q["out_moments"] == MARK) == ("out_moments" in over), over
        assert np.all(q["out_clipped"] == 0xA5) == ("out_clipped" in over), over


def test_wrappers_check_their_arguments(rt):
    p = _planes()
    c, h, n = p["color"], p["history"], p["history_length"]
    out, hist = rt.temporal_rectify_host(c, h, n)
    assert out.shape == (H, W, 4) and out.dtype == np.float32 and hist.shape == (H, W) and hist.dtype == np.float32
    out, hist, mom, clip = rt.temporal_rectify_host(c, h, n, p["object"], moments=p["moments"], history_moments=p["history_moments"], clipped=True)
    assert mom.shape == (H, W, 4) and clip.shape == (H, W) and clip.dtype == np.uint8
    mine = np.zeros((H, W), np.uint8)
    assert rt.temporal_rectify_host(c, h, n, p["object"], clipped=mine)[2] is mine and np.array_equal(mine, clip)
    for bad in (dict(moments=p["moments"]), dict(history_moments=p["history_moments"]), dict(out_moments=np.zeros((H, W, 4), np.float32)),
                dict(out=np.zeros((H, W, 4), np.float64)), dict(out_history=np.zeros((H, W, 1), np.float32)),
                dict(clipped=np.zeros((H, W), np.float32)), dict(object=p["object"][:-1])):
        with pytest.raises(ValueError):
            rt.temporal_rectify_host(c, h, n, **bad)
    with pytest.raises(ValueError):
        rt.temporal_rectify_host(None, h, n)
    with pytest.raises(ValueError):
        rt.temporal_rectify_host(c[:, :-1], h, n)
    for bad in (dict(radius=0), dict(radius=4), dict(clip_sigma=-1.0), dict(clip_history=0.5), dict(out=c)):
        with pytest.raises(rt.RtError) as e:
            rt.temporal_rectify_host(c, h, n, **bad)
        assert e.value.code == INVALID, bad
    t = rt.RayTracer.__new__(rt.RayTracer)   # (no handle: the checks come before any library call)
    t._L, t._h, t.device = None, None, 0
    with pytest.raises(ValueError):
        t.temporal_rectify(None, h, n)
    with pytest.raises(ValueError):
        t.temporal_rectify(c, h, n, moments=p["moments"])


def test_reproject_is_accumulation_with_a_dropped_sample(rt):
    """temporal_reproject_host: the history fetched and nothing blended in -- out_history is accumulation's minus one where
    there is history, `out` NaN and out_history 1 where there is none."""
    import _temporal_reference as T
    planes, cam, _ = T.synthetic_case()
    g = {k: planes[k] for k in ("point", "normal", "object")}
    pg = {k[5:]: planes[k] for k in ("prev_point", "prev_normal", "prev_object")}
    out, hist, motion = rt.temporal_accumulate_host(g, pg, cam, planes["prev_color"], planes["prev_history"], planes["color"], 4.0, motion=True)
    h, n, m = rt.temporal_reproject_host(g, pg, cam, planes["prev_color"], planes["prev_history"], 4.0, motion=True)
    none = np.isnan(h).all(-1)
    assert none.any() and not none.all() and np.isfinite(h[~none]).all() and (h.view(np.uint32)[none] == 0x7FC00000).all()
    assert (n[none] == 1).all() and T.same_bits(m, motion).all()
    ok = ~none & np.isfinite(planes["color"]).all(-1)
    assert (n[ok] + 1 == hist[ok]).all() and (n[~none] >= 1).all()
