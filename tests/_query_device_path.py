"""Helper of tests/test_gpu_ray_query.py::test_device_path (run as a script): the ray queries on torch tensors -- device
memory, the call ordered on the handle's stream between the current torch stream's work -- against the host path, and a
pipelined render sequence with device queries between its frames against the same sequence without them.  torch is
imported first (ray_tracer_2_amd/__init__.py: its HIP runtime then serves the library too)."""
import os
import sys

import numpy as np
import torch   # first, as in bench.py

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import _ray_families as RF  # noqa: E402
import ray_tracer_2_amd as rt  # noqa: E402
from ray_tracer_2_amd.ray_tracer import normalize3_f32  # noqa: E402

F32 = np.float32


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, F32)).to("cuda:0")


t = rt.RayTracer(0, 64, 48)
for name in ("cornell", "items", "glass", "tlas9", "dragon"):
    arrays = RF.scene(rt, name)
    fams = RF.families(arrays, name, n_random=20000)
    ro = np.concatenate([v[0] for v in fams.values()])
    nd = normalize3_f32(np.concatenate([v[1] for v in fams.values()]))
    tm = np.random.default_rng(3).uniform(0.01, 4.0, len(ro)).astype(F32)
    for opts in ({}, {"lds_scene": 0}):
        for k, v in {"lds_scene": 1, **opts}.items():
            t.set_option(k, v)
        t.load_scene(arrays)
        host = t.trace_rays(ro, nd, tm)
        got = t.hits_to_numpy(t.trace_rays(dev(ro), dev(nd), dev(tm)))
        assert np.array_equal(got.view(np.uint8), host.view(np.uint8)), (name, opts, "trace_rays")
        for prune in (False, True):
            o = t.occluded(dev(ro), dev(nd), dev(tm), prune=prune)
            assert isinstance(o, torch.Tensor) and o.dtype == torch.bool
            assert np.array_equal(o.cpu().numpy(), t.occluded(ro, nd, tm, prune=prune)), (name, opts, prune)
        # unbounded tmax on the device path
        got = t.hits_to_numpy(t.trace_rays(dev(ro[:777]), dev(nd[:777])))
        assert np.array_equal(got.view(np.uint8), t.trace_rays(ro[:777], nd[:777]).view(np.uint8)), (name, opts)
    print(name, len(ro), "rays: device path == host path", flush=True)
t.set_option("lds_scene", 1)

# no side effects: a pipelined accumulation with device queries issued between its frames
cornell = RF.scene(rt, "cornell")
fams = RF.families(cornell, "cornell", n_random=20000)
ro = dev(np.concatenate([v[0] for v in fams.values()]))
nd = dev(normalize3_f32(np.concatenate([v[1] for v in fams.values()])))
p0 = rt.make_params(64, 48, 3, 2, skybox=1, frames=0)


def run(queries, frame_ahead):
    t.set_option("frame_ahead", frame_ahead)
    t.load_scene(cornell)
    t.reset_timing()
    for f in range(12):
        t.render(rt.make_params(64, 48, 3, 2, skybox=1, frames=f))
        if queries:
            t.trace_rays(ro, nd)
            t.occluded(ro, nd, torch.full((ro.shape[0],), 1.0, device="cuda:0"))
            if f % 4 == 1:
                t.pick(p0, 3, 5)
    img = t.read_image(64, 48)
    s = t.stats()
    return img, (s.segments, s.paths, s.node_tests, s.triangle_tests, s.frames, s.segments_reused, s.frames_speculative)


for fa in (-1, 8):
    a, sa = run(False, fa)
    b, sb = run(True, fa)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), fa
    # (the automatic policy, -1, renders ahead when a call finds the stream busy: how far is a matter of timing, with
    # or without queries -- there only the frames asked for are schedule-free; an explicit depth fixes every counter)
    assert (sa == sb) if fa > 0 else (sa[4] == sb[4]), (fa, sa, sb)
t.close()
print("device path ok")
