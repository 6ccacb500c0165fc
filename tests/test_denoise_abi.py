"""rt_denoise_desc of include/rt_abi.h against the ctypes struct of ray_tracer_2_amd._abi, as the host compiler lays it out;
the bindings; every argument error that needs no device, on rt_denoise_host, with `out` left as it was."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

FIELDS = ["struct_bytes", "_p0", "width", "height", "iterations", "sigma_color", "sigma_normal", "sigma_point", "color",
          "normal", "point", "albedo", "emission", "out"]
INVALID, CAPACITY = -1, -2


def test_header_layout_matches_the_ctypes_struct(rt, tmp_path):
    from ray_tracer_2_amd import _abi as A
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_abi.h"', "int main(void) {",
             '    printf("size %zu\\n", sizeof(rt_denoise_desc));']
    for f in FIELDS:
        lines.append(f'    printf("{f} %zu %zu\\n", offsetof(rt_denoise_desc, {f}), sizeof(((rt_denoise_desc*)0)->{f}));')
    lines += ['    printf("flag %d\\n", RT_DENOISE_HOST_MEMORY);', "    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c11", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in out if l}
    assert got["size"] == [C.sizeof(A.DenoiseDesc)]
    assert [n for n, _ in A.DenoiseDesc._fields_] == FIELDS
    for f in FIELDS:
        d = getattr(A.DenoiseDesc, f)
        assert got[f] == [d.offset, d.size], f
    assert got["flag"] == [A.DENOISE_HOST_MEMORY]
    assert list(A.DENOISE_PLANES) == FIELDS[8:]


def test_the_calls_are_declared_and_bound(rt):
    from ray_tracer_2_amd.lib import EXPORTS
    L = rt.load()
    header = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    for name, nargs in (("rt_denoise", 3), ("rt_denoise_host", 1)):
        assert name in EXPORTS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == nargs and getattr(L, name).restype is C.c_int
        assert f"int {name}(" in header


W, H = 6, 4


def _planes():
    rng = np.random.default_rng(5)
    p = {"color": rng.uniform(0, 2, (H, W, 4)), "normal": np.tile([0.0, 0.0, 1.0], (H, W, 1)), "point": rng.uniform(0, 1, (H, W, 3)),
         "albedo": rng.uniform(0.2, 1, (H, W, 4)), "emission": np.zeros((H, W, 4))}
    p = {k: np.ascontiguousarray(v, np.float32) for k, v in p.items()}
    p["out"] = np.full((H, W, 4), np.float32(-7.25))
    return p


def _desc(A, p, **over):
    d = A.DenoiseDesc(struct_bytes=C.sizeof(A.DenoiseDesc), width=W, height=H, iterations=2, sigma_color=4.0, sigma_normal=0.3,
                      sigma_point=1.0)
    for k, v in p.items():
        setattr(d, k, v.ctypes.data)
    for k, v in over.items():
        setattr(d, k, v)
    return d


CASES = [
    ("struct_bytes too small", dict(struct_bytes=72), INVALID, "struct_bytes"),
    ("struct_bytes zero", dict(struct_bytes=0), INVALID, "struct_bytes"),
    ("struct_bytes too large", dict(struct_bytes=88), INVALID, "struct_bytes"),
    ("_p0", dict(_p0=1), INVALID, "_p0"),
    ("zero width", dict(width=0), INVALID, "zero"),
    ("zero height", dict(height=0), INVALID, "zero"),
    ("no iterations", dict(iterations=0), INVALID, "iterations"),
    ("nine iterations", dict(iterations=9), INVALID, "iterations"),
    ("sigma_color zero", dict(sigma_color=0.0), INVALID, "sigma"),
    ("sigma_color negative", dict(sigma_color=-1.0), INVALID, "sigma"),
    ("sigma_color NaN", dict(sigma_color=float("nan")), INVALID, "sigma"),
    ("sigma_normal zero", dict(sigma_normal=0.0), INVALID, "sigma"),
    ("sigma_normal NaN", dict(sigma_normal=float("nan")), INVALID, "sigma"),
    ("sigma_normal infinite", dict(sigma_normal=float("inf")), INVALID, "finite"),
    ("sigma_point negative", dict(sigma_point=-0.5), INVALID, "sigma"),
    ("sigma_point NaN", dict(sigma_point=float("nan")), INVALID, "sigma"),
    ("sigma_point infinite", dict(sigma_point=float("inf")), INVALID, "finite"),
    ("null color", dict(color=None), INVALID, "color"),
    ("null normal", dict(normal=None), INVALID, "null"),
    ("null point", dict(point=None), INVALID, "null"),
    ("null out", dict(out=None), INVALID, "null"),
    ("2^31 texels", dict(width=1 << 16, height=1 << 15), CAPACITY, "2^31"),
    ("more than 2^31 texels", dict(width=0x7fffffff, height=2), CAPACITY, "2^31"),
]


@pytest.mark.parametrize("what,over,code,text", CASES, ids=[c[0] for c in CASES])
def test_errors_leave_out_untouched(rt, what, over, code, text):
    from ray_tracer_2_amd import _abi as A
    L = rt.load()
    p = _planes()
    assert L.rt_denoise_host(C.byref(_desc(A, p, **over))) == code, what
    assert text in L.rt_last_error(None).decode(), (what, L.rt_last_error(None))
    assert np.all(p["out"] == np.float32(-7.25)), what


def test_null_desc_and_the_call_that_is_right(rt):
    from ray_tracer_2_amd import _abi as A
    L = rt.load()
    assert L.rt_denoise_host(None) == INVALID and "null" in L.rt_last_error(None).decode()
    p = _planes()
    assert L.rt_denoise_host(C.byref(_desc(A, p))) == 0
    assert not np.any(p["out"] == np.float32(-7.25))
    q = _planes()   # the optional planes may be NULL, sigma_color may be infinite, 8 iterations are allowed
    assert L.rt_denoise_host(C.byref(_desc(A, q, albedo=None, emission=None, sigma_color=float("inf"), iterations=8))) == 0
    assert not np.any(q["out"] == np.float32(-7.25))


def test_wrappers_check_their_arguments(rt):
    p = _planes()
    g = {k: p[k] for k in ("normal", "point", "albedo", "emission")}
    out = rt.denoise_host(g, p["color"])
    assert out.shape == (H, W, 4) and out.dtype == np.float32
    with pytest.raises(ValueError):
        rt.denoise_host({"normal": p["normal"]}, p["color"])
    with pytest.raises(ValueError):
        rt.denoise_host(g, p["color"][:, :-1])
    with pytest.raises(ValueError):
        rt.denoise_host(g, p["color"], out=np.zeros((H, W, 4), np.float64))
    with pytest.raises(rt.RtError) as e:
        rt.denoise_host(g, p["color"], iterations=0)
    assert e.value.code == INVALID
    t = rt.RayTracer.__new__(rt.RayTracer)   # (no handle: the checks come before any library call)
    t._L, t._h, t.device = None, None, 0
    with pytest.raises(ValueError):
        t.denoise({"point": p["point"]}, p["color"])
    with pytest.raises(ValueError):
        t.denoise(g, None)
