"""rt_vdenoise_desc of include/rt_abi.h against the ctypes struct of ray_tracer_2_amd._abi, as the host compiler lays it out;
the bindings; every argument error that needs no device, on rt_denoise_variance_host and rt_luminance_moments_host, with the
outputs left as they were."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

FIELDS = ["struct_bytes", "_p0", "width", "height", "iterations", "sigma_luminance", "sigma_normal", "sigma_point", "min_history",
          "_p1", "color", "normal", "point", "albedo", "emission", "moments", "history", "out", "out_variance"]
INVALID, CAPACITY = -1, -2


def test_header_layout_matches_the_ctypes_struct(rt, tmp_path):
    from ray_tracer_2_amd import _abi as A
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_abi.h"', "int main(void) {",
             '    printf("size %zu\\n", sizeof(rt_vdenoise_desc));']
    for f in FIELDS:
        lines.append(f'    printf("{f} %zu %zu\\n", offsetof(rt_vdenoise_desc, {f}), sizeof(((rt_vdenoise_desc*)0)->{f}));')
    lines += ['    printf("flag %d\\n", RT_VDENOISE_HOST_MEMORY);', "    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c11", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {l.split()[0]: [int(x) for x in l.split()[1:]] for l in out if l}
    assert got["size"] == [C.sizeof(A.VDenoiseDesc)]
    assert [n for n, _ in A.VDenoiseDesc._fields_] == FIELDS
    for f in FIELDS:
        d = getattr(A.VDenoiseDesc, f)
        assert got[f] == [d.offset, d.size], f
    assert got["flag"] == [A.VDENOISE_HOST_MEMORY]
    assert list(A.VDENOISE_PLANES) == FIELDS[10:]


def test_the_calls_are_declared_and_bound(rt):
    from ray_tracer_2_amd.lib import EXPORTS
    L = rt.load()
    header = open(os.path.join(ROOT, "include", "rt_abi.h")).read()
    for name, nargs in (("rt_denoise_variance", 3), ("rt_luminance_moments", 3), ("rt_denoise_variance_host", 1),
                        ("rt_luminance_moments_host", 1)):
        assert name in EXPORTS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == nargs and getattr(L, name).restype is C.c_int
        assert f"int {name}(" in header
    assert callable(rt.denoise_variance_host) and callable(rt.luminance_moments_host)
    assert callable(rt.RayTracer.denoise_variance) and callable(rt.RayTracer.luminance_moments)


W, H = 6, 4
UNTOUCHED = np.float32(-7.25)


def _planes():
    rng = np.random.default_rng(5)
    p = {"color": rng.uniform(0, 2, (H, W, 4)), "normal": np.tile([0.0, 0.0, 1.0], (H, W, 1)), "point": rng.uniform(0, 1, (H, W, 3)),
         "albedo": rng.uniform(0.2, 1, (H, W, 4)), "emission": np.zeros((H, W, 4)), "moments": rng.uniform(1, 2, (H, W, 4)),
         "history": rng.integers(1, 9, (H, W))}
    p = {k: np.ascontiguousarray(v, np.float32) for k, v in p.items()}
    p["out"] = np.full((H, W, 4), UNTOUCHED)
    p["out_variance"] = np.full((H, W), UNTOUCHED)
    return p


def _desc(A, p, **over):
    d = A.VDenoiseDesc(struct_bytes=C.sizeof(A.VDenoiseDesc), width=W, height=H, iterations=2, sigma_luminance=4.0, sigma_normal=0.3,
                       sigma_point=1.0, min_history=4.0)
    for k, v in p.items():
        setattr(d, k, v.ctypes.data)
    for k, v in over.items():
        setattr(d, k, v)
    return d


# (what, overrides, code, text of the reason, does rt_luminance_moments_host refuse it too)
CASES = [
    ("struct_bytes too small", dict(struct_bytes=104), INVALID, "struct_bytes", True),
    ("struct_bytes zero", dict(struct_bytes=0), INVALID, "struct_bytes", True),
    ("struct_bytes too large", dict(struct_bytes=120), INVALID, "struct_bytes", True),
    ("struct_bytes of rt_denoise_desc", dict(struct_bytes=80), INVALID, "struct_bytes", True),
    ("_p0", dict(_p0=1), INVALID, "_p0", True),
    ("_p1", dict(_p1=1), INVALID, "_p1", True),
    ("zero width", dict(width=0), INVALID, "zero", True),
    ("zero height", dict(height=0), INVALID, "zero", True),
    ("no iterations", dict(iterations=0), INVALID, "iterations", False),
    ("nine iterations", dict(iterations=9), INVALID, "iterations", False),
    ("sigma_luminance zero", dict(sigma_luminance=0.0), INVALID, "sigma", False),
    ("sigma_luminance negative", dict(sigma_luminance=-1.0), INVALID, "sigma", False),
    ("sigma_luminance NaN", dict(sigma_luminance=float("nan")), INVALID, "sigma", False),
    ("sigma_luminance infinite", dict(sigma_luminance=float("inf")), INVALID, "finite", False),
    ("sigma_normal zero", dict(sigma_normal=0.0), INVALID, "sigma", False),
    ("sigma_normal NaN", dict(sigma_normal=float("nan")), INVALID, "sigma", False),
    ("sigma_normal infinite", dict(sigma_normal=float("inf")), INVALID, "finite", False),
    ("sigma_point negative", dict(sigma_point=-0.5), INVALID, "sigma", False),
    ("sigma_point NaN", dict(sigma_point=float("nan")), INVALID, "sigma", False),
    ("sigma_point infinite", dict(sigma_point=float("inf")), INVALID, "finite", False),
    ("min_history below 1", dict(min_history=0.5), INVALID, "min_history", False),
    ("min_history zero", dict(min_history=0.0), INVALID, "min_history", False),
    ("min_history NaN", dict(min_history=float("nan")), INVALID, "min_history", False),
    ("min_history infinite", dict(min_history=float("inf")), INVALID, "min_history", False),
    ("moments without history", dict(history=None), INVALID, "go together", False),
    ("history without moments", dict(moments=None), INVALID, "go together", False),
    ("null color", dict(color=None), INVALID, "color", True),
    ("null normal", dict(normal=None), INVALID, "null", True),
    ("null point", dict(point=None), INVALID, "null", True),
    ("null out", dict(out=None), INVALID, "null", True),
    ("2^31 texels", dict(width=1 << 16, height=1 << 15), CAPACITY, "2^31", True),
    ("more than 2^31 texels", dict(width=0x7fffffff, height=2), CAPACITY, "2^31", True),
]


@pytest.mark.parametrize("what,over,code,text,both", CASES, ids=[c[0] for c in CASES])
def test_errors_leave_the_outputs_untouched(rt, what, over, code, text, both):
    from ray_tracer_2_amd import _abi as A
    L = rt.load()
    p = _planes()
    assert L.rt_denoise_variance_host(C.byref(_desc(A, p, **over))) == code, what
    assert text in L.rt_last_error(None).decode(), (what, L.rt_last_error(None))
    assert np.all(p["out"] == UNTOUCHED) and np.all(p["out_variance"] == UNTOUCHED), what
    rc = L.rt_luminance_moments_host(C.byref(_desc(A, p, **over)))
    if both:
        assert rc == code and text in L.rt_last_error(None).decode(), (what, L.rt_last_error(None))
        assert np.all(p["out"] == UNTOUCHED), what
    else:   # (rt_luminance_moments examines neither the filter's parameters nor the moments planes)
        assert rc == 0 and not np.any(p["out"] == UNTOUCHED), what
    assert np.all(p["out_variance"] == UNTOUCHED), what


def test_null_desc_and_the_calls_that_are_right(rt):
    from ray_tracer_2_amd import _abi as A
    L = rt.load()
    for fn in (L.rt_denoise_variance_host, L.rt_luminance_moments_host):
        assert fn(None) == INVALID and "null" in L.rt_last_error(None).decode()
    p = _planes()
    assert L.rt_denoise_variance_host(C.byref(_desc(A, p))) == 0
    assert not np.any(p["out"] == UNTOUCHED) and not np.any(p["out_variance"] == UNTOUCHED)
    q = _planes()   # the optional planes may be NULL, min_history may be 1, 8 iterations are allowed
    assert L.rt_denoise_variance_host(C.byref(_desc(A, q, albedo=None, emission=None, moments=None, history=None, out_variance=None,
                                                    min_history=1.0, iterations=8))) == 0
    assert not np.any(q["out"] == UNTOUCHED) and np.all(q["out_variance"] == UNTOUCHED)


def test_wrappers_check_their_arguments(rt):
    p = _planes()
    g = {k: p[k] for k in ("normal", "point", "albedo", "emission")}
    out = rt.denoise_variance_host(g, p["color"])
    assert out.shape == (H, W, 4) and out.dtype == np.float32
    out, var = rt.denoise_variance_host(g, p["color"], moments=p["moments"], history=p["history"], out_variance=True)
    assert out.shape == (H, W, 4) and var.shape == (H, W) and var.dtype == np.float32
    assert rt.luminance_moments_host(g, p["color"]).shape == (H, W, 4)
    with pytest.raises(ValueError):
        rt.denoise_variance_host({"normal": p["normal"]}, p["color"])
    with pytest.raises(ValueError):
        rt.denoise_variance_host(g, p["color"][:, :-1])
    with pytest.raises(ValueError):
        rt.denoise_variance_host(g, None)
    with pytest.raises(ValueError):
        rt.denoise_variance_host(g, p["color"], moments=p["moments"])
    with pytest.raises(ValueError):
        rt.denoise_variance_host(g, p["color"], history=p["history"])
    with pytest.raises(ValueError):
        rt.denoise_variance_host(g, p["color"], moments=p["moments"], history=p["history"][:-1])
    with pytest.raises(ValueError):
        rt.denoise_variance_host(g, p["color"], out=np.zeros((H, W, 4), np.float64))
    with pytest.raises(ValueError):
        rt.denoise_variance_host(g, p["color"], out_variance=np.zeros((H, W, 1), np.float32))
    with pytest.raises(ValueError):
        rt.luminance_moments_host({"point": p["point"]}, p["color"])
    with pytest.raises(rt.RtError) as e:
        rt.denoise_variance_host(g, p["color"], iterations=0)
    assert e.value.code == INVALID
    with pytest.raises(rt.RtError) as e:
        rt.denoise_variance_host(g, p["color"], min_history=0.5)
    assert e.value.code == INVALID
    t = rt.RayTracer.__new__(rt.RayTracer)   # (no handle: the checks come before any library call)
    t._L, t._h, t.device = None, None, 0
    with pytest.raises(ValueError):
        t.denoise_variance({"point": p["point"]}, p["color"])
    with pytest.raises(ValueError):
        t.denoise_variance(g, None)
    with pytest.raises(ValueError):
        t.denoise_variance(g, p["color"], moments=p["moments"])
    with pytest.raises(ValueError):
        t.luminance_moments(g, None)
