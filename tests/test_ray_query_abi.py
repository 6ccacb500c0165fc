"""The ray-query structs of include/rt_abi.h (rt_ray, rt_hit) against the ctypes / numpy views of ray_tracer_2_amd._abi,
as the host compiler lays them out; the query wrappers' argument checks, which need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

FIELDS = {
    "rt_ray": ["origin", "tmax", "dir", "_p0"],
    "rt_hit": ["t", "object", "primitive", "flags", "point", "bary_u", "normal", "bary_v", "tex_u", "tex_v", "_p1"],
}


def test_header_layout_matches_the_ctypes_structs(rt, tmp_path):
    from ray_tracer_2_amd import _abi as A
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_abi.h"', "int main(void) {"]
    for s, fs in FIELDS.items():
        lines.append(f'    printf("{s} size %zu\\n", sizeof({s}));')
        for f in fs:
            lines.append(f'    printf("{s} {f} %zu\\n", offsetof({s}, {f}));')
    lines += ['    printf("flags %d %d %d %d\\n", RT_QUERY_HOST_MEMORY, RT_QUERY_PRUNE_TMAX, RT_HIT_HIT, RT_HIT_BACKFACE);',
              "    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c11", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {tuple(l.split()[:2]): int(l.split()[2]) for l in out if l and not l.startswith("flags")}
    for s, cls, dt in (("rt_ray", A.Ray, A.RAY_DTYPE), ("rt_hit", A.Hit, A.HIT_DTYPE)):
        assert got[(s, "size")] == C.sizeof(cls) == dt.itemsize
        assert [n for n, _ in cls._fields_] == FIELDS[s] == list(dt.names)
        for f in FIELDS[s]:
            assert got[(s, f)] == getattr(cls, f).offset == dt.fields[f][1], (s, f)
    flags = [l for l in out if l.startswith("flags")][0].split()[1:]
    assert list(map(int, flags)) == [A.QUERY_HOST_MEMORY, A.QUERY_PRUNE_TMAX, A.HIT_HIT, A.HIT_BACKFACE]


@pytest.fixture
def unbound(rt):
    """A RayTracer without a handle: the argument checks run before any library call."""
    t = rt.RayTracer.__new__(rt.RayTracer)
    t._L, t._h, t.device = None, None, 0
    return t


def test_wrappers_reject_bad_shapes_and_dtypes(unbound):
    t = unbound
    o = np.zeros((4, 3), np.float32)
    bad = [
        lambda: t.trace_rays(np.zeros((4, 2), np.float32), o),
        lambda: t.trace_rays(o, np.zeros((5, 3), np.float32)),
        lambda: t.trace_rays(np.zeros(12, np.float32), np.zeros(12, np.float32)),
        lambda: t.trace_rays(np.zeros((4, 3), np.int32), o),
        lambda: t.trace_rays(o, o.astype(np.complex64)),
        lambda: t.trace_rays(o, o, np.ones(3, np.float32)),
        lambda: t.trace_rays(o, o, np.array(["a"] * 4)),
        lambda: t.occluded(o, o, None),
        lambda: t.occluded(o, o, np.ones((4, 1), np.float32)),
        lambda: t.occluded(np.zeros((4, 3), bool), o, 1.0),
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
        assert t._h is None, i


def test_wrappers_reject_tensors_that_cannot_be_query_inputs(unbound):
    torch = pytest.importorskip("torch")
    t = unbound
    o = torch.zeros((4, 3), dtype=torch.float32)   # (CPU tensors: not on the handle's device)
    for args in [(o, o), (o.double(), o), (o, np.zeros((4, 3), np.float32)), (o, o, torch.ones(4))]:
        with pytest.raises(ValueError):
            t.trace_rays(*args)
    with pytest.raises(ValueError):
        t.occluded(o, o, torch.ones(4))


def test_queries_are_declared_and_bound(rt):
    from ray_tracer_2_amd.lib import EXPORTS
    L = rt.load()
    for name in ("rt_intersect_rays", "rt_occluded_rays", "rt_pick"):
        assert name in EXPORTS and hasattr(L, name) and len(getattr(L, name).argtypes) == 5
