"""Helper of tests/test_gpu_refit.py::test_device_input (run as a script): rt_refit_triangles with a torch tensor on the
device -- produced by torch work still in flight on the current stream when the call is made -- leaves the blob, launch
shape, image and ray queries of a fresh upload of the refitted arrays, for one mesh of many and for all meshes; and a
pipelined render sequence with device refits between its frames renders each frame with its own geometry.  torch is
imported first (ray_tracer_2_amd/__init__.py: its HIP runtime then serves the library too)."""
import os
import sys

import numpy as np
import torch   # first, as in bench.py

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import test_gpu_refit as R  # noqa: E402
import ray_tracer_2_amd as rt  # noqa: E402

F32 = np.float32
W, H = R.W, R.H
L = rt.load_test()
T = rt.RayTracer(0, W, H, lib=L)
Fr = rt.RayTracer(0, W, H, lib=L)


def device_copy(new):
    base = torch.from_numpy(np.ascontiguousarray(new).view(F32).reshape(len(new), 24)).to("cuda:0")
    busy = torch.rand((2048, 2048), device="cuda:0")
    for _ in range(8):   # (queued ahead of the tensor below: the refit must wait for both)
        busy = busy @ busy * 1e-3
    return (base * 4.0) * 0.25


def shape(t):
    d = t.last_launch()
    return tuple(d[k] for k in R.E.LAUNCH_KEYS)


for name in ("cornell", "room", "sponza200", "dragon", "tlas8", "leaf128", "height32"):
    a = R.scene(rt, name)
    for which in ("one", "all"):
        first, n = R.mesh_range(a, *R.which_meshes(a, which))
        new = R.moved(a, first, n, seed=len(name) + n)
        b = R.refitted(a, first, new)
        T.load_scene(a)
        T.refit_triangles(device_copy(new), first)
        blob, lay, _ = T.scene_blob()
        Fr.load_scene(b)
        blob_f, lay_f, _ = Fr.scene_blob()
        assert np.array_equal(lay, lay_f) and np.array_equal(blob, blob_f), (name, which, np.flatnonzero(blob != blob_f)[:8])
        imgs = []
        for t in (T, Fr):
            t.render(R.E.params(rt, 0))
            t.render(R.E.params(rt, 1))
            imgs.append((t.read_image(W, H), shape(t)))
        assert np.array_equal(imgs[0][0].view(np.uint32), imgs[1][0].view(np.uint32)) and imgs[0][1] == imgs[1][1], (name, which)
        ro, rd = R.E.rays(b, n=2000)
        assert T.trace_rays(ro, rd).tobytes() == Fr.trace_rays(ro, rd).tobytes(), (name, which)
        print(name, which, n, "triangles from the device: blob, launch, image and queries == a fresh upload", flush=True)

# device refits between pipelined frames == host refits between them
a = R.scene(rt, "dragon")
first, n = R.mesh_range(a, *R.which_meshes(a, "one"))
news = [R.moved(a, first, n, seed=200 + f, scale=0.01 * (1 + f % 3)) for f in range(8)]
out = []
for dev in (False, True):
    T.load_scene(a)
    T.reset_timing()
    for f in range(8):
        T.refit_triangles(device_copy(news[f]) if dev else news[f], first)
        T.render(R.E.params(rt, f))
    out.append(T.read_image(W, H))
assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))
T.close()
Fr.close()
print("device input ok")
