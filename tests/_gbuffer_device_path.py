"""Helper of tests/test_gpu_gbuffer.py::test_device_path (run as a script): rt_render_gbuffer into torch tensors -- device
memory, the call ordered on the handle's stream between the current torch stream's work -- against the host path byte
for byte, and a pipelined render sequence with asynchronous G-buffer calls between its frames against the same sequence
without them.  torch is imported first (ray_tracer_2_amd/__init__.py: its HIP runtime then serves the library too)."""
import os
import sys

import numpy as np
import torch   # first, as in bench.py

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import _ray_families as RF  # noqa: E402
import ray_tracer_2_amd as rt  # noqa: E402
from ray_tracer_2_amd import _abi as A  # noqa: E402

ALL = tuple(A.GBUFFER_CHANNELS)
KINDS = {"<f4": torch.float32, "<u4": torch.int32, "u1": torch.uint8}

t = rt.RayTracer(0, 64, 48)
for name in ("cornell", "items", "glass", "tlas9", "dragon"):
    arrays = RF.scene(rt, name)
    for opts in ({}, {"lds_scene": 0}):
        for k, v in {"lds_scene": 1, **opts}.items():
            t.set_option(k, v)
        t.load_scene(arrays)
        for W, H in ((67, 45), (1, 1), (640, 360)):
            p = rt.make_params(W, H, 1, 1)
            host = t.render_gbuffer(p, ALL)
            # the device call after work on the current stream that the planes must not overtake, and read back after it
            dev = t.render_gbuffer(p, ALL, device=True)
            for c in ALL:
                dt, k = A.GBUFFER_CHANNELS[c]
                assert isinstance(dev[c], torch.Tensor) and dev[c].dtype == KINDS[dt] and dev[c].device.index == 0, c
                assert tuple(dev[c].shape) == ((H, W, k) if k else (H, W)), c
                assert np.array_equal(dev[c].cpu().numpy().view(np.uint8), host[c].view(np.uint8)), (name, opts, W, H, c)
            sub = t.render_gbuffer(p, device=True)   # the default channels
            assert tuple(sub) == ("depth", "normal", "albedo", "object")
            for c in sub:
                assert np.array_equal(sub[c].cpu().numpy().view(np.uint8), host[c].view(np.uint8)), (name, opts, W, H, c)
    print(name, "device path == host path", flush=True)
t.set_option("lds_scene", 1)

# the least alignment the contract allows: the float planes at an odd multiple of 4 bytes (the planes of 2 and 3 floats are
# stored 8 and 12 bytes at a time), albedo / emission at an odd multiple of 16, flags at an odd address
import ctypes as C  # noqa: E402
for name in ("cornell", "tlas9"):   # (the kernels of runs and of tiles)
    t.load_scene(RF.scene(rt, name))
    W, H = 67, 45
    p = rt.make_params(W, H, 1, 1)
    host = t.render_gbuffer(p, ALL)
    g, raw, skew = A.GBuffer(struct_bytes=C.sizeof(A.GBuffer)), {}, {}
    for c in ALL:
        dt, k = A.GBUFFER_CHANNELS[c]
        skew[c] = 16 if c in ("albedo", "emission") else 1 if c == "flags" else 4
        raw[c] = torch.zeros(host[c].nbytes + 32, dtype=torch.uint8, device="cuda:0")
        assert raw[c].data_ptr() % 32 == 0
        setattr(g, c, raw[c].data_ptr() + skew[c])
    torch.cuda.synchronize()
    t._check(t._L.rt_render_gbuffer(t._h, C.byref(p), C.byref(g), 0))
    t.synchronize()
    for c in ALL:
        got = raw[c].cpu().numpy()
        assert np.array_equal(got[skew[c]:skew[c] + host[c].nbytes], host[c].view(np.uint8).ravel()), (name, c)
        assert not got[:skew[c]].any() and not got[skew[c] + host[c].nbytes:].any(), (name, c, "bytes outside the plane")
    print(name, "planes at their least alignment ok", flush=True)

# no side effects: a pipelined accumulation with asynchronous G-buffer calls issued between its frames
cornell = RF.scene(rt, "cornell")
pg = rt.make_params(320, 180, 1, 1)


def run(gbuffers, frame_ahead):
    t.set_option("frame_ahead", frame_ahead)
    t.load_scene(cornell)
    t.reset_timing()
    keep = []
    for f in range(12):
        t.render(rt.make_params(64, 48, 3, 2, skybox=1, frames=f))
        if gbuffers:
            keep.append(t.render_gbuffer(pg, ALL if f % 3 == 0 else ("depth", "normal", "albedo"), device=True))
    img = t.read_image(64, 48)
    s = t.stats()
    return img, (s.segments, s.paths, s.node_tests, s.triangle_tests, s.frames, s.segments_reused, s.frames_speculative), keep


for fa in (-1, 8):
    a, sa, _ = run(False, fa)
    b, sb, keep = run(True, fa)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), fa
    # (the automatic policy, -1, renders ahead when a call finds the stream busy: how far is a matter of timing, with or
    # without the calls -- there only the frames asked for are schedule-free; an explicit depth fixes every counter)
    assert (sa == sb) if fa > 0 else (sa[4] == sb[4]), (fa, sa, sb)
    want = t.render_gbuffer(pg, ALL)
    for g in keep:   # every call of the sequence produced the frame's planes
        for c in g:
            assert np.array_equal(g[c].cpu().numpy().view(np.uint8), want[c].view(np.uint8)), (fa, c)
t.close()
print("device path ok")
