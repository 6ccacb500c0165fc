"""Helper of tests/test_gpu_radiance.py::test_device_path (run as a script): RayTracer.radiance on torch tensors -- device
memory, the call ordered on the handle's stream between the current torch stream's work -- against the host path.  torch is
imported first (ray_tracer_2_amd/__init__.py: its HIP runtime then serves the library too)."""
import os
import sys

import numpy as np
import torch   # first, as in bench.py

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import _radiance_cases as RC  # noqa: E402
import ray_tracer_2_amd as rt  # noqa: E402

F32 = np.float32
t = rt.RayTracer(0, 64, 48)
for name in ("cornell", "glass", "tlas9", "dragon"):
    arrays = RC.scene(rt, name)
    cams = RC.cameras(arrays, n=4)
    for lds in (1, 0):
        RC.set_options(t, {"lds_scene": lds})
        t.load_scene(arrays)
        o, d, s, _ = RC.camera_batch(t, rt, cams)
        host = t.radiance(o, d, s, 3, 3)
        assert (host[:, :3] != 0).any(), name
        do, dd = (torch.from_numpy(x).to("cuda:0") for x in (o, d))
        ds = torch.from_numpy(s.view(np.int32)).to("cuda:0")   # (the u32 bits)
        # the inputs are produced by work on the current stream right before the call, the output is consumed right after it
        got = t.radiance(do * 1.0, dd * 1.0, ds + 0, 3, 3)
        total = got.sum()
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and tuple(got.shape) == (len(s), 4)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), host.view(np.uint32)), (name, lds)
        assert np.isfinite(float(total)) or not np.isfinite(host).all()
        assert tuple(t.radiance(do[:0], dd[:0], ds[:0], 3, 3).shape) == (0, 4)
    print(name, len(s), "rays: device path == host path", flush=True)
RC.set_options(t, {})
t.close()
print("device path ok")
