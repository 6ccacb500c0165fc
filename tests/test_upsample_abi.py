"""rt_upsample_desc of include/rt_abi.h against the ctypes struct of ray_tracer_2_amd._abi, as the host compiler lays it
out; the bindings; every argument error that needs no device, on rt_upsample_host, with the outputs left as they were."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

FIELDS = ["struct_bytes", "_p0", "lo_width", "lo_height", "width", "height", "point_tolerance", "normal_cos", "lo_color", "lo_point",
          "lo_normal", "lo_object", "lo_albedo", "depth", "point", "normal", "object", "albedo", "emission", "out", "coverage"]
INVALID, CAPACITY = -1, -2
MARK = np.float32(-7.25)
w, h, W, H = 4, 3, 7, 5


def test_header_layout_matches_the_ctypes_struct(rt, tmp_path):
    from ray_tracer_2_amd import _abi as A
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_abi.h"', "int main(void) {",
             '    printf("size %zu\\n", sizeof(rt_upsample_desc));']
    for f in FIELDS:
        lines.append(f'    printf("{f} %zu %zu\\n", offsetof(rt_upsample_desc, {f}), sizeof(((rt_upsample_desc*)0)->{f}));')
    lines += ['    printf("flag %d\\n", RT_UPSAMPLE_HOST_MEMORY);', "    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c11", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in out if l}
    assert got["size"] == [C.sizeof(A.UpsampleDesc)] == [136]
    assert [n for n, _ in A.UpsampleDesc._fields_] == FIELDS
    for f in FIELDS:
        d = getattr(A.UpsampleDesc, f)
        assert got[f] == [d.offset, d.size], f
    assert got["flag"] == [A.UPSAMPLE_HOST_MEMORY]
    assert list(A.UPSAMPLE_PLANES) == FIELDS[8:] and list(A.UPSAMPLE_LO_COMPONENTS) == FIELDS[8:13]


def test_the_calls_are_declared_and_bound(rt):
    from ray_tracer_2_amd.lib import EXPORTS
    L = rt.load()
    header = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    for name, nargs in (("rt_upsample", 3), ("rt_upsample_host", 1)):
        assert name in EXPORTS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == nargs and getattr(L, name).restype is C.c_int
        assert f"int {name}(" in header
    assert callable(rt.upsample_host) and callable(rt.RayTracer.upsample)


def _planes():
    rng = np.random.default_rng(5)
    f = lambda *s: rng.uniform(0.5, 2, s).astype(np.float32)   # noqa: E731
    p = dict(lo_color=f(h, w, 4), lo_point=f(h, w, 3), lo_normal=f(h, w, 3), lo_object=np.ones((h, w), np.uint32), lo_albedo=f(h, w, 4),
             depth=f(H, W), point=f(H, W, 3), normal=f(H, W, 3), object=np.ones((H, W), np.uint32), albedo=f(H, W, 4),
             emission=np.zeros((H, W, 4), np.float32), out=np.full((H, W, 4), MARK), coverage=np.full((H, W), 0xA5, np.uint8))
    p["lo_normal"][:] = p["normal"][:] = (0, 0, -1)
    p["lo_point"][:] = p["point"][:] = (0, 0, 3)
    return p


def _desc(A, p, **over):
    d = A.UpsampleDesc(struct_bytes=C.sizeof(A.UpsampleDesc), lo_width=w, lo_height=h, width=W, height=H, point_tolerance=0.02, normal_cos=0.9)
    for k, v in p.items():
        setattr(d, k, v.ctypes.data)
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _untouched(p):
    return bool(np.all(p["out"] == MARK) and np.all(p["coverage"] == 0xA5))


CASES = [
    ("struct_bytes too small", dict(struct_bytes=128), INVALID, "struct_bytes"),
    ("struct_bytes zero", dict(struct_bytes=0), INVALID, "struct_bytes"),
    ("struct_bytes too large", dict(struct_bytes=144), INVALID, "struct_bytes"),
    ("_p0", dict(_p0=1), INVALID, "_p0"),
    ("zero lo_width", dict(lo_width=0), INVALID, "zero"),
    ("zero lo_height", dict(lo_height=0), INVALID, "zero"),
    ("zero width", dict(width=0), INVALID, "zero"),
    ("zero height", dict(height=0), INVALID, "zero"),
    ("point_tolerance zero", dict(point_tolerance=0.0), INVALID, "point_tolerance"),
    ("point_tolerance negative", dict(point_tolerance=-0.01), INVALID, "point_tolerance"),
    ("point_tolerance NaN", dict(point_tolerance=float("nan")), INVALID, "point_tolerance"),
    ("point_tolerance infinite", dict(point_tolerance=float("inf")), INVALID, "point_tolerance"),
    ("normal_cos NaN", dict(normal_cos=float("nan")), INVALID, "normal_cos"),
    ("normal_cos above 1", dict(normal_cos=1.5), INVALID, "normal_cos"),
    ("normal_cos below -1", dict(normal_cos=-1.5), INVALID, "normal_cos"),
    ("normal_cos infinite", dict(normal_cos=float("inf")), INVALID, "normal_cos"),
    ("null lo_color", dict(lo_color=None), INVALID, "lo_color"),
    ("null lo_point", dict(lo_point=None), INVALID, "null"),
    ("null lo_normal", dict(lo_normal=None), INVALID, "null"),
    ("null lo_object", dict(lo_object=None), INVALID, "null"),
    ("null depth", dict(depth=None), INVALID, "null"),
    ("null point", dict(point=None), INVALID, "null"),
    ("null normal", dict(normal=None), INVALID, "null"),
    ("null object", dict(object=None), INVALID, "null"),
    ("null out", dict(out=None), INVALID, "null"),
    ("lo_albedo alone", dict(albedo=None), INVALID, "albedo"),
    ("albedo alone", dict(lo_albedo=None), INVALID, "albedo"),
    ("2^31 low texels", dict(lo_width=1 << 16, lo_height=1 << 15), CAPACITY, "2^31"),
    ("2^31 high texels", dict(width=1 << 16, height=1 << 15), CAPACITY, "2^31"),
    ("more than 2^31 high texels", dict(width=0x7fffffff, height=2), CAPACITY, "2^31"),
]


@pytest.mark.parametrize("what,over,code,text", CASES, ids=[c[0] for c in CASES])
def test_errors_leave_the_outputs_untouched(rt, what, over, code, text):
    from ray_tracer_2_amd import _abi as A
    L = rt.load()
    p = _planes()
    assert L.rt_upsample_host(C.byref(_desc(A, p, **over))) == code, what
    assert text in L.rt_last_error(None).decode(), (what, L.rt_last_error(None))
    assert _untouched(p), what


def test_null_desc_and_the_call_that_is_right(rt):
    from ray_tracer_2_amd import _abi as A
    L = rt.load()
    assert L.rt_upsample_host(None) == INVALID and "null" in L.rt_last_error(None).decode()
    p = _planes()
    assert L.rt_upsample_host(C.byref(_desc(A, p))) == 0
    assert not np.any(p["out"] == MARK) and np.all(p["coverage"] == 2)
    # the optional planes may be NULL; normal_cos may be -1 or 1
    for over in (dict(emission=None), dict(albedo=None, lo_albedo=None), dict(coverage=None), dict(normal_cos=-1.0), dict(normal_cos=1.0),
                 dict(albedo=None, lo_albedo=None, emission=None, coverage=None)):
        q = _planes()
        assert L.rt_upsample_host(C.byref(_desc(A, q, **over))) == 0, over
        assert not np.any(q["out"] == MARK), over
        assert np.all(q["coverage"] == 0xA5) == ("coverage" in over), over


def test_wrappers_check_their_arguments(rt):
    p = _planes()
    lo = {k[3:]: p[k] for k in ("lo_point", "lo_normal", "lo_object", "lo_albedo")}
    hi = {k: p[k] for k in ("depth", "point", "normal", "object", "albedo", "emission")}
    out = rt.upsample_host(lo, hi, p["lo_color"])
    assert out.shape == (H, W, 4) and out.dtype == np.float32
    out, cov = rt.upsample_host(lo, hi, p["lo_color"], coverage=True)
    assert cov.shape == (H, W) and cov.dtype == np.uint8
    mine = np.zeros((H, W), np.uint8)
    assert rt.upsample_host(lo, hi, p["lo_color"], coverage=mine)[1] is mine and np.array_equal(mine, cov)
    drop = lambda d, k: {n: v for n, v in d.items() if n != k}   # noqa: E731
    for k in ("point", "normal", "object"):
        with pytest.raises(ValueError):
            rt.upsample_host(drop(lo, k), hi, p["lo_color"])
    for k in ("depth", "point", "normal", "object"):
        with pytest.raises(ValueError):
            rt.upsample_host(lo, drop(hi, k), p["lo_color"])
    with pytest.raises(ValueError):
        rt.upsample_host(drop(lo, "albedo"), hi, p["lo_color"])
    with pytest.raises(ValueError):
        rt.upsample_host(lo, drop(hi, "albedo"), p["lo_color"])
    with pytest.raises(ValueError):
        rt.upsample_host(lo, hi, None)
    with pytest.raises(ValueError):
        rt.upsample_host(lo, hi, p["lo_color"][:, :-1])
    with pytest.raises(ValueError):
        rt.upsample_host(lo, dict(hi, depth=p["depth"][:-1]), p["lo_color"])
    with pytest.raises(ValueError):
        rt.upsample_host(lo, hi, p["lo_color"], out=np.zeros((H, W, 4), np.float64))
    with pytest.raises(ValueError):
        rt.upsample_host(lo, hi, p["lo_color"], coverage=np.zeros((H, W), np.float32))
    with pytest.raises(rt.RtError) as e:
        rt.upsample_host(lo, hi, p["lo_color"], point_tolerance=0.0)
    assert e.value.code == INVALID
    t = rt.RayTracer.__new__(rt.RayTracer)   # (no handle: the checks come before any library call)
    t._L, t._h, t.device = None, None, 0
    with pytest.raises(ValueError):
        t.upsample(drop(lo, "object"), hi, p["lo_color"])
    with pytest.raises(ValueError):
        t.upsample(lo, hi, None)
