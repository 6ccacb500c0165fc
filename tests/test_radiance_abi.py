"""The radiance query's struct of include/rt_abi.h (rt_path_ray) against the ctypes / numpy views of ray_tracer_2_amd._abi,
as the host compiler lays it out; RayTracer.radiance's argument checks, which need no device; pixel_seeds against wgsl:475."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

FIELDS = ["origin", "seed", "dir", "_p0"]


def test_header_layout_matches_the_ctypes_struct(rt, tmp_path):
    from ray_tracer_2_amd import _abi as A
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt_abi.h"', "int main(void) {",
             '    printf("size %zu\\n", sizeof(rt_path_ray));']
    lines += [f'    printf("{f} %zu\\n", offsetof(rt_path_ray, {f}));' for f in FIELDS]
    lines += ['    printf("flag %d\\n", RT_RADIANCE_HOST_MEMORY);', "    return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-std=c11", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(A.PathRay) == A.PATH_RAY_DTYPE.itemsize == 32
    assert [n for n, _ in A.PathRay._fields_] == FIELDS == list(A.PATH_RAY_DTYPE.names)
    for f in FIELDS:
        assert int(got[f]) == getattr(A.PathRay, f).offset == A.PATH_RAY_DTYPE.fields[f][1], f
    assert int(got["flag"]) == A.RADIANCE_HOST_MEMORY == 1


def test_the_call_is_declared_and_bound(rt):
    from ray_tracer_2_amd.lib import EXPORTS
    L = rt.load()
    assert "rt_radiance_rays" in EXPORTS and len(L.rt_radiance_rays.argtypes) == 6


@pytest.fixture
def unbound(rt):
    """A RayTracer without a handle: the argument checks run before any library call."""
    t = rt.RayTracer.__new__(rt.RayTracer)
    t._L, t._h, t.device = None, None, 0
    return t


def test_wrapper_rejects_bad_arguments(unbound):
    t = unbound
    o = np.zeros((4, 3), np.float32)
    s = np.zeros(4, np.uint32)
    bad = [
        lambda: t.radiance(np.zeros((4, 2), np.float32), o, s, 1, 1),      # shapes
        lambda: t.radiance(o, np.zeros((5, 3), np.float32), s, 1, 1),
        lambda: t.radiance(np.zeros(12, np.float32), np.zeros(12, np.float32), s, 1, 1),
        lambda: t.radiance(o, o, np.zeros(3, np.uint32), 1, 1),            # lengths
        lambda: t.radiance(o, o, np.zeros((4, 1), np.uint32), 1, 1),
        lambda: t.radiance(np.zeros((4, 3), np.int32), o, s, 1, 1),        # dtypes
        lambda: t.radiance(o, o.astype(np.complex64), s, 1, 1),
        lambda: t.radiance(o, o, s.astype(np.int32), 1, 1),
        lambda: t.radiance(o, o, s.astype(np.float32), 1, 1),
        lambda: t.radiance(o, o, s.astype(np.uint64), 1, 1),
        lambda: t.radiance(o, o, s, 1, 0),                                 # samples < 1
        lambda: t.radiance(o, o, s, 1, -3),
        lambda: t.radiance(o, o, s, -1, 1),                                # bounces < 0
    ]
    for i, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
        assert t._h is None, i


def test_wrapper_rejects_tensors_that_cannot_be_inputs(unbound):
    torch = pytest.importorskip("torch")
    t = unbound
    o = torch.zeros((4, 3), dtype=torch.float32)   # (CPU tensors: not on the handle's device)
    s = torch.zeros(4, dtype=torch.int32)
    for args in [(o, o, s), (o.double(), o, s), (o, np.zeros((4, 3), np.float32), s), (o, o, np.zeros(4, np.uint32))]:
        with pytest.raises(ValueError):
            t.radiance(*args, 1, 1)


@pytest.mark.parametrize("frames", [0, 3, -5, 2**31 - 1])
def test_pixel_seeds_are_the_shader_s(rt, frames):
    """wgsl:475: y * width + x + |frames| * 719393 in u32 arithmetic, row-major."""
    for w, h in ((8, 8), (5, 3), (1, 1), (300, 7)):
        got = rt.pixel_seeds(w, h, frames)
        assert got.dtype == np.uint32 and got.shape == (w * h,)
        want = [((y * w + x) + abs(frames) * 719393) % 2**32 for y in range(h) for x in range(w)]
        assert got.tolist() == want


def test_pixel_seeds_wrap_around(rt):
    """A frame whose sum passes 2^32 inside the frame: 5970 * 719393 = 2^32 - 191,086, so the seeds of a 1024 x 256 frame
    (262,144 texels) wrap at texel 191,086."""
    f, w, h = 5970, 1024, 256
    base = f * 719393
    assert base < 2**32 <= base + w * h - 1
    for frames in (f, -f):
        got = rt.pixel_seeds(w, h, frames)
        k = 2**32 - base
        assert got[k - 1] == 2**32 - 1 and got[k] == 0 and got[-1] == w * h - 1 - k
        assert np.array_equal(got, ((np.arange(w * h, dtype=np.uint64) + np.uint64(base)) % np.uint64(2**32)).astype(np.uint32))
