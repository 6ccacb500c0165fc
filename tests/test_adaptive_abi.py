"""rt_adaptive_plan_desc and rt_adaptive_merge_desc of include/rt_abi.h against the ctypes structs of ray_tracer_2_amd._abi, as
the host compiler lays them out; the bindings; every argument error that needs no device, on rt_adaptive_plan_host and
rt_adaptive_merge_host, with the outputs left as they were; the wrappers' own checks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

PLAN_FIELDS = ["struct_bytes", "_p0", "width", "height", "budget", "min_samples", "max_samples", "first_frame", "origin", "_p1",
               "variance", "dir", "counts", "offsets", "rays", "totals"]
MERGE_FIELDS = ["struct_bytes", "_p0", "width", "height", "budget", "max_history", "radiance", "counts", "offsets", "color",
                "history", "albedo", "moments", "out", "out_history", "out_moments"]
INVALID, CAPACITY = -1, -2
F32, U32 = np.float32, np.uint32


def test_header_layout_matches_the_ctypes_structs(rt, tmp_path):
    from ray_tracer_2_amd import _abi as A
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_abi.h"', "int main(void) {"]
    for t, fields in (("rt_adaptive_plan_desc", PLAN_FIELDS), ("rt_adaptive_merge_desc", MERGE_FIELDS)):
        lines.append(f'    printf("{t} %zu\\n", sizeof({t}));')
        for f in fields:
            lines.append(f'    printf("{t}.{f} %zu %zu\\n", offsetof({t}, {f}), sizeof((({t}*)0)->{f}));')
    lines += ['    printf("flag %d\\n", RT_ADAPTIVE_HOST_MEMORY);', "    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c11", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in out if l}
    for t, cls, fields in (("rt_adaptive_plan_desc", A.AdaptivePlanDesc, PLAN_FIELDS), ("rt_adaptive_merge_desc", A.AdaptiveMergeDesc, MERGE_FIELDS)):
        assert got[t] == [C.sizeof(cls)]
        assert [n for n, _ in cls._fields_] == fields
        for f in fields:
            d = getattr(cls, f)
            assert got[f"{t}.{f}"] == [d.offset, d.size], (t, f)
    assert got["flag"] == [A.ADAPTIVE_HOST_MEMORY]
    assert set(A.ADAPTIVE_PLAN_PLANES) | {"rays", "totals"} == set(PLAN_FIELDS[10:])
    assert set(A.ADAPTIVE_MERGE_PLANES) | {"radiance"} == set(MERGE_FIELDS[6:])


def test_the_calls_are_declared_and_bound(rt):
    from ray_tracer_2_amd.lib import EXPORTS
    L = rt.load()
    header = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    for name, nargs in (("rt_adaptive_plan", 3), ("rt_adaptive_merge", 3), ("rt_adaptive_plan_host", 1), ("rt_adaptive_merge_host", 1)):
        assert name in EXPORTS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == nargs and getattr(L, name).restype is C.c_int
        assert f"int {name}(" in header
    assert callable(rt.adaptive_plan_host) and callable(rt.adaptive_merge_host)
    for m in ("adaptive_plan", "adaptive_merge", "adaptive_samples"):
        assert callable(getattr(rt.RayTracer, m))


W, H, BUDGET = 6, 4, 60
MARK = 0xA5A5A5A5


def _plan_planes():
    rng = np.random.default_rng(5)
    return {"variance": rng.uniform(0, 2, (H, W)).astype(F32), "dir": rng.normal(0, 1, (H, W, 3)).astype(F32),
            "counts": np.full((H, W), MARK, U32), "offsets": np.full((H, W), MARK, U32), "rays": np.full((BUDGET, 8), MARK, U32),
            "totals": np.full(4, MARK, U32)}


def _plan_desc(A, p, **over):
    d = A.AdaptivePlanDesc(struct_bytes=C.sizeof(A.AdaptivePlanDesc), width=W, height=H, budget=BUDGET, min_samples=1, max_samples=16)
    for k, v in p.items():
        setattr(d, k, v.ctypes.data)
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _plan_untouched(p):
    return all((p[k] == MARK).all() for k in ("counts", "offsets", "rays", "totals"))


PLAN_CASES = [
    ("struct_bytes too small", dict(struct_bytes=88), INVALID, "struct_bytes"),
    ("struct_bytes zero", dict(struct_bytes=0), INVALID, "struct_bytes"),
    ("struct_bytes of the merge", dict(struct_bytes=104), INVALID, "struct_bytes"),
    ("_p0", dict(_p0=1), INVALID, "_p0"),
    ("_p1", dict(_p1=1), INVALID, "_p1"),
    ("zero width", dict(width=0), INVALID, "zero"),
    ("zero height", dict(height=0), INVALID, "zero"),
    ("no budget", dict(budget=0, min_samples=0), INVALID, "budget"),
    ("budget 2^31", dict(budget=1 << 31), INVALID, "budget"),
    ("no max_samples", dict(max_samples=0, min_samples=0), INVALID, "max_samples"),
    ("max_samples 65536", dict(max_samples=65536), INVALID, "max_samples"),
    ("min above max", dict(min_samples=17), INVALID, "min_samples"),
    ("min W H above the budget", dict(min_samples=3), INVALID, "budget"),
    ("min W H one above the budget", dict(min_samples=2, budget=47), INVALID, "budget"),
    ("null variance", dict(variance=None), INVALID, "null"),
    ("null dir", dict(dir=None), INVALID, "null"),
    ("null counts", dict(counts=None), INVALID, "null"),
    ("null offsets", dict(offsets=None), INVALID, "null"),
    ("null rays", dict(rays=None), INVALID, "null"),
    ("null totals", dict(totals=None), INVALID, "null"),
    ("2^31 texels", dict(width=1 << 16, height=1 << 15, min_samples=0), CAPACITY, "2^31"),
    ("more than 2^31 texels, min 1", dict(width=0x7fffffff, height=2), CAPACITY, "2^31"),
]


@pytest.mark.parametrize("what,over,code,text", PLAN_CASES, ids=[c[0] for c in PLAN_CASES])
def test_plan_errors_leave_the_outputs_untouched(rt, what, over, code, text):
    from ray_tracer_2_amd import _abi as A
    L = rt.load()
    p = _plan_planes()
    assert L.rt_adaptive_plan_host(C.byref(_plan_desc(A, p, **over))) == code, what
    assert text in L.rt_last_error(None).decode(), (what, L.rt_last_error(None))
    assert _plan_untouched(p), what


def _merge_planes():
    rng = np.random.default_rng(6)
    counts = np.full((H, W), 2, U32)
    return {"radiance": rng.uniform(0, 2, (BUDGET, 4)).astype(F32), "counts": counts,
            "offsets": (np.arange(W * H, dtype=U32) * 2).reshape(H, W), "color": rng.uniform(0, 2, (H, W, 4)).astype(F32),
            "history": rng.integers(0, 5, (H, W)).astype(F32), "albedo": rng.uniform(0.2, 1, (H, W, 4)).astype(F32),
            "moments": rng.uniform(0, 2, (H, W, 4)).astype(F32), "out": np.full((H, W, 4), F32(-7.25)),
            "out_history": np.full((H, W), F32(-7.25)), "out_moments": np.full((H, W, 4), F32(-7.25))}


def _merge_desc(A, p, **over):
    d = A.AdaptiveMergeDesc(struct_bytes=C.sizeof(A.AdaptiveMergeDesc), width=W, height=H, budget=BUDGET, max_history=float("inf"))
    for k, v in p.items():
        setattr(d, k, v.ctypes.data)
    for k, v in over.items():
        setattr(d, k, v)
    return d


def _merge_untouched(p):
    return all((p[k] == F32(-7.25)).all() for k in ("out", "out_history", "out_moments"))


MERGE_CASES = [
    ("struct_bytes too small", dict(struct_bytes=96), INVALID, "struct_bytes"),
    ("struct_bytes zero", dict(struct_bytes=0), INVALID, "struct_bytes"),
    ("_p0", dict(_p0=1), INVALID, "_p0"),
    ("zero width", dict(width=0), INVALID, "zero"),
    ("zero height", dict(height=0), INVALID, "zero"),
    ("no budget", dict(budget=0), INVALID, "budget"),
    ("budget 2^31", dict(budget=1 << 31), INVALID, "budget"),
    ("max_history below 1", dict(max_history=0.5), INVALID, "max_history"),
    ("max_history NaN", dict(max_history=float("nan")), INVALID, "max_history"),
    ("null radiance", dict(radiance=None), INVALID, "null"),
    ("null counts", dict(counts=None), INVALID, "null"),
    ("null offsets", dict(offsets=None), INVALID, "null"),
    ("null color", dict(color=None), INVALID, "color"),
    ("null history", dict(history=None), INVALID, "null"),
    ("null out", dict(out=None), INVALID, "null"),
    ("null out_history", dict(out_history=None), INVALID, "null"),
    ("moments without out_moments", dict(out_moments=None), INVALID, "go together"),
    ("out_moments without moments", dict(moments=None), INVALID, "go together"),
    ("2^31 texels", dict(width=1 << 16, height=1 << 15), CAPACITY, "2^31"),
]


@pytest.mark.parametrize("what,over,code,text", MERGE_CASES, ids=[c[0] for c in MERGE_CASES])
def test_merge_errors_leave_the_outputs_untouched(rt, what, over, code, text):
    from ray_tracer_2_amd import _abi as A
    L = rt.load()
    p = _merge_planes()
    assert L.rt_adaptive_merge_host(C.byref(_merge_desc(A, p, **over))) == code, what
    assert text in L.rt_last_error(None).decode(), (what, L.rt_last_error(None))
    assert _merge_untouched(p), what


def test_null_desc_and_the_calls_that_are_right(rt):
    from ray_tracer_2_amd import _abi as A
    L = rt.load()
    for fn in (L.rt_adaptive_plan_host, L.rt_adaptive_merge_host):
        assert fn(None) == INVALID and "null" in L.rt_last_error(None).decode()
    p = _plan_planes()
    assert L.rt_adaptive_plan_host(C.byref(_plan_desc(A, p))) == 0
    assert not any((p[k] == MARK).any() for k in ("counts", "offsets", "rays", "totals"))
    assert p["totals"][0] == p["counts"].sum() == BUDGET and p["totals"][3] == 0
    # the edges that are allowed: min = max, budget = min W H exactly, max_samples 65535, budget 2^31 - 1 is not tried (64 GB)
    q = _plan_planes()
    assert L.rt_adaptive_plan_host(C.byref(_plan_desc(A, q, min_samples=2, max_samples=2, budget=48))) == 0 and (q["counts"] == 2).all()
    assert L.rt_adaptive_plan_host(C.byref(_plan_desc(A, q, min_samples=0, max_samples=65535))) == 0
    m = _merge_planes()
    assert L.rt_adaptive_merge_host(C.byref(_merge_desc(A, m))) == 0 and not any((m[k] == F32(-7.25)).any() for k in ("out", "out_history"))
    m = _merge_planes()   # the optional planes may be NULL, max_history may be 1
    assert L.rt_adaptive_merge_host(C.byref(_merge_desc(A, m, albedo=None, moments=None, out_moments=None, max_history=1.0))) == 0
    assert (m["out_moments"] == F32(-7.25)).all() and not (m["out"] == F32(-7.25)).any()


def test_wrappers_check_their_arguments(rt):
    p, m = _plan_planes(), _merge_planes()
    counts, offsets, rays, totals = rt.adaptive_plan_host(p["variance"], p["dir"], (0, 0, 1), BUDGET)
    assert counts.shape == offsets.shape == (H, W) and counts.dtype == offsets.dtype == U32
    assert rays.shape == (BUDGET,) and rays.dtype.itemsize == 32 and totals.shape == (4,)
    out, hist = rt.adaptive_merge_host(m["radiance"], counts, offsets, m["color"], m["history"])
    assert out.shape == (H, W, 4) and hist.shape == (H, W) and out.dtype == hist.dtype == F32
    assert len(rt.adaptive_merge_host(m["radiance"], counts, offsets, m["color"], m["history"], moments=m["moments"])) == 3
    with pytest.raises(ValueError):
        rt.adaptive_plan_host(p["variance"], p["dir"][:, :-1], (0, 0, 1), BUDGET)
    with pytest.raises(ValueError):
        rt.adaptive_plan_host(p["variance"], p["dir"], (0, 0), BUDGET)
    with pytest.raises(ValueError):
        rt.adaptive_plan_host(p["variance"], p["dir"], (0, 0, 1), 0)
    with pytest.raises(ValueError):
        rt.adaptive_plan_host(p["variance"], p["dir"], (0, 0, 1), 1 << 31)
    with pytest.raises(rt.RtError) as e:
        rt.adaptive_plan_host(p["variance"], p["dir"], (0, 0, 1), W * H - 1)
    assert e.value.code == INVALID
    with pytest.raises(rt.RtError) as e:
        rt.adaptive_plan_host(p["variance"], p["dir"], (0, 0, 1), BUDGET, max_samples=70000)
    assert e.value.code == INVALID
    with pytest.raises(ValueError):
        rt.adaptive_merge_host(m["radiance"], counts, offsets, None, m["history"])
    with pytest.raises(ValueError):
        rt.adaptive_merge_host(m["radiance"][:, :3], counts, offsets, m["color"], m["history"])
    with pytest.raises(ValueError):
        rt.adaptive_merge_host(m["radiance"], counts, offsets, m["color"], m["history"][:-1])
    with pytest.raises(ValueError):
        rt.adaptive_merge_host(m["radiance"], counts, offsets, m["color"], m["history"], out_moments=m["out_moments"])
    with pytest.raises(ValueError):
        rt.adaptive_merge_host(m["radiance"], counts, offsets, m["color"], m["history"], out=np.zeros((H, W, 4), np.float64))
    with pytest.raises(rt.RtError) as e:
        rt.adaptive_merge_host(m["radiance"], counts, offsets, m["color"], m["history"], max_history=0.0)
    assert e.value.code == INVALID
    t = rt.RayTracer.__new__(rt.RayTracer)   # (no handle: the checks come before any library call)
    t._L, t._h, t.device = None, None, 0
    with pytest.raises(ValueError):
        t.adaptive_plan(p["variance"], p["dir"], (0, 0, 1), 0)
    with pytest.raises(ValueError):
        t.adaptive_merge(m["radiance"], counts, offsets, None, m["history"])
    with pytest.raises(ValueError):
        t.adaptive_samples({"normal": p["dir"]}, p["variance"], m["color"], m["history"], BUDGET, 4, 1, (0, 0, 1))
    with pytest.raises(ValueError):
        t.adaptive_samples({"dir": p["dir"]}, p["variance"], m["color"], m["history"], BUDGET, -1, 1, (0, 0, 1))
