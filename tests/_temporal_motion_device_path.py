"""Helper of tests/test_gpu_temporal_motion.py::test_device_path (run as a script): rt_temporal_accumulate_moving on torch
tensors -- device memory, a device-resident motion table, the call ordered on the handle's stream between the current torch
stream's work -- against the host restatement bit for bit: prev_object and motion on and off, `out` aliasing `color`, a NULL
colour for the handle's image (into another tensor, and into the image itself, read back by the read_image that follows),
every plane and the table at their least alignment, and a handle that holds more than its cap.  torch is imported first
(ray_tracer_2_amd/__init__.py: its HIP runtime then serves the library too)."""
import ctypes as C
import os
import sys

import numpy as np
import torch   # first, as in bench.py

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import ray_tracer_2_amd as rt  # noqa: E402
from ray_tracer_2_amd import _abi as A  # noqa: E402
import _temporal_motion_reference as M  # noqa: E402
import _temporal_reference as R  # noqa: E402
import _over_cap as OC  # noqa: E402

CHANNELS = ("point", "normal", "object")
CAP, TOL, NCOS = 3.0, 0.01, 0.9
dev = torch.device("cuda:0")


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want, what):
    assert len(got) == len(want), what
    for a, b, name in zip(got, want, ("out", "out_history", "motion")):
        assert isinstance(a, torch.Tensor) and a.dtype == torch.float32 and tuple(a.shape) == b.shape, (what, name)
        assert np.array_equal(bits(a), bits(b)), (what, name)


def on_device(table):
    return torch.from_numpy(table.view(np.int32).reshape(-1, 24).copy()).to(dev)


arrays = rt.SceneArrays.load(os.path.join(HERE, "golden", "cornell_scene.npz"))
moved_arrays = M.moved_mesh(arrays, {5: M.rigid((0.06, 0.0, 0.02), 0.05, M.centroid(arrays, 5)),
                                     6: M.rigid((-0.04, 0.0, 0.03), -0.08, M.centroid(arrays, 6))})
table = rt.object_motions(arrays, moved_arrays)
assert table["moved"].nonzero()[0].tolist() == [5, 6]
dev_table = on_device(table)
base = arrays.uniform.camera
moved = R.moved_camera(base, right=0.11, up=-0.04, forward=0.02)
t = rt.RayTracer(0, 130, 70)
t.load_scene(arrays)
for W, H in ((130, 70), (67, 45)):
    pr = rt.make_params(W, H, 4, 8, skybox=1, frames=0)
    g1 = rt.make_params(W, H, 1, 1)
    t.update_instances(arrays)
    t.set_camera(base)
    t.render(pr)
    prev_image = t.read_image(W, H).copy()
    host_pg = t.render_gbuffer(g1, CHANNELS)
    dev_pg = t.render_gbuffer(g1, CHANNELS, device=True)
    t.update_instances(moved_arrays)
    t.set_camera(moved)
    host_g = t.render_gbuffer(g1, CHANNELS)
    dev_g = t.render_gbuffer(g1, CHANNELS, device=True)
    t.render(pr)                       # the current frame stays in the handle's image
    image = t.read_image(W, H).copy()
    history = np.random.default_rng(W).integers(1, 7, (H, W)).astype(np.float32)
    color, prev_color, prev_history = (torch.from_numpy(a).to(dev) for a in (image, prev_image, history))
    for objects, motion in ((True, True), (True, False), (False, True), (False, False)):
        pick = (lambda d: d) if objects else (lambda d: {k: v for k, v in d.items() if k != "object"})
        want = rt.temporal_accumulate_host(host_g, pick(host_pg), base, prev_image, history, image, CAP, TOL, NCOS, motion=motion, motions=table)
        got = t.temporal_accumulate(dev_g, pick(dev_pg), base, prev_color, prev_history, color, CAP, TOL, NCOS, motion=motion, motions=dev_table)
        same(got, want, (W, H, objects, motion))
    want = rt.temporal_accumulate_host(host_g, host_pg, base, prev_image, history, image, CAP, TOL, NCOS, motion=True, motions=table)
    boxes = (host_g["object"] == 5) | (host_g["object"] == 6)
    assert (want[1][boxes] > 1).mean() > 0.5 and (want[1] == 1).any()
    plain = rt.temporal_accumulate_host(host_g, host_pg, base, prev_image, history, image, CAP, TOL, NCOS, motion=True)
    assert not np.array_equal(bits(plain[2][boxes]), bits(want[2][boxes]))       # (the table changes where the boxes' texels look)
    # out aliasing color, the outputs given
    buf, hist, mot = color.clone(), torch.zeros((H, W), device=dev), torch.zeros((H, W, 2), device=dev)
    got = t.temporal_accumulate(dev_g, dev_pg, base, prev_color, prev_history, buf, CAP, TOL, NCOS, out=buf, out_history=hist, motion=mot,
                                motions=dev_table)
    assert got[0] is buf and got[1] is hist and got[2] is mot
    same(got, want, (W, H, "out is color"))
    # a NULL colour is the handle's image (the frame rendered above); the image keeps its bits when out is elsewhere
    got = t.temporal_accumulate(dev_g, dev_pg, base, prev_color, prev_history, None, CAP, TOL, NCOS, motion=True, motions=dev_table)
    same(got, want, (W, H, "NULL colour"))
    assert np.array_equal(bits(t.read_image(W, H)), bits(image)), (W, H, "the image changed")
    # ... and may be the output too: the image accumulated in place, and the read_image that follows sees the result
    d = A.TemporalMotionDesc(struct_bytes=C.sizeof(A.TemporalMotionDesc), width=W, height=H,
                             prev_camera=A.CameraUniform.from_buffer_copy(bytes(base)), max_history=CAP, point_tolerance=TOL, normal_cos=NCOS,
                             motions=dev_table.data_ptr(), n_objects=len(table))
    for k in CHANNELS:
        setattr(d, k, dev_g[k].data_ptr())
        setattr(d, "prev_" + k, dev_pg[k].data_ptr())
    d.prev_color, d.prev_history = prev_color.data_ptr(), prev_history.data_ptr()
    hist.zero_()
    d.out, d.out_history = t.device_image_ptr, hist.data_ptr()
    torch.cuda.synchronize()
    t._check(t._L.rt_temporal_accumulate_moving(t._h, C.byref(d), 0))
    assert np.array_equal(bits(t.read_image(W, H)), bits(want[0])), (W, H, "the image in place")
    assert np.array_equal(bits(hist), bits(want[1])), (W, H, "the image in place: history")
    print(W, H, "device path == host", flush=True)

# the least alignment the contract allows: the planes of 4-byte elements at an odd multiple of 4 bytes, motion at an odd
# multiple of 8, the float4 planes and the table at an odd multiple of 16; nothing is written outside the outputs
assert (W, H) == (67, 45)   # (the frames of the loop's last round)
planes = dict(color=image, **{k: host_g[k] for k in CHANNELS}, prev_color=prev_image, prev_history=history,
              **{"prev_" + k: host_pg[k] for k in CHANNELS})
planes = {k: np.ascontiguousarray(v) for k, v in planes.items()}
pick = lambda pre: {k: planes[pre + k] for k in CHANNELS}  # noqa: E731
want = rt.temporal_accumulate_host(pick(""), pick("prev_"), base, planes["prev_color"], planes["prev_history"], planes["color"], CAP, TOL, NCOS,
                                   motion=True, motions=table)
assert (want[1] > 1).mean() > 0.2
planes.update(out=np.zeros((H, W, 4), np.float32), out_history=np.zeros((H, W), np.float32), motion=np.zeros((H, W, 2), np.float32),
              motions=table)
d = A.TemporalMotionDesc(struct_bytes=C.sizeof(A.TemporalMotionDesc), width=W, height=H, prev_camera=A.CameraUniform.from_buffer_copy(bytes(base)),
                         max_history=CAP, point_tolerance=TOL, normal_cos=NCOS, n_objects=len(table))
align = {"color": 16, "prev_color": 16, "out": 16, "motion": 8, "motions": 16}
raw, skew = {}, {}
for k, v in planes.items():
    skew[k] = align.get(k, 4)
    raw[k] = torch.zeros(v.nbytes + 64, dtype=torch.uint8, device=dev)
    assert raw[k].data_ptr() % 32 == 0
    raw[k][skew[k]:skew[k] + v.nbytes] = torch.from_numpy(v.view(np.uint8).ravel().copy()).to(dev)
    setattr(d, k, raw[k].data_ptr() + skew[k])
torch.cuda.synchronize()
t._check(t._L.rt_temporal_accumulate_moving(t._h, C.byref(d), 0))
t.synchronize()
for k, w in zip(("out", "out_history", "motion"), want):
    got = raw[k].cpu().numpy()
    n = planes[k].nbytes
    assert np.array_equal(got[skew[k]:skew[k] + n].view(np.uint32), bits(w).ravel()), (k, "planes at their least alignment")
    assert not got[:skew[k]].any() and not got[skew[k] + n:].any(), (k, "bytes outside the plane")
for k in planes:
    if k not in ("out", "out_history", "motion"):
        assert np.array_equal(raw[k].cpu().numpy()[skew[k]:skew[k] + planes[k].nbytes], planes[k].view(np.uint8).ravel()), (k, "an input changed")
print("planes at their least alignment ok", flush=True)

# a handle that already holds more than option max_device_mb allows (the denoiser's scratch, once the cap is lowered under
# it): rt_temporal_accumulate_moving on device memory allocates nothing and is done all the same
t.update_instances(arrays)
t.set_camera(base)
host_pg, dev_pg, prev_image = OC.frame(t, 1)
t.update_instances(moved_arrays)
t.set_camera(moved)
host_g, dev_g, image = OC.frame(t, 2)
pick = lambda g: {k: g[k] for k in CHANNELS}  # noqa: E731
history = np.random.default_rng(3).integers(1, 7, (OC.H, OC.W)).astype(np.float32)
color, prev_color, prev_history = (torch.from_numpy(a).to(dev) for a in (image, prev_image, history))
outs = tuple(torch.empty(s, dtype=torch.float32, device=dev) for s in ((OC.H, OC.W, 4), (OC.H, OC.W), (OC.H, OC.W, 2)))
want = rt.temporal_accumulate_host(pick(host_g), pick(host_pg), base, prev_image, history, image, CAP, TOL, NCOS, motion=True, motions=table)
call = lambda: t.temporal_accumulate(pick(dev_g), pick(dev_pg), base, prev_color, prev_history, color, CAP, TOL, NCOS,  # noqa: E731
                                     out=outs[0], out_history=outs[1], motion=outs[2], motions=dev_table)
call()
OC.hold_denoise_scratch(t, dev_g, color)
OC.over_cap(t, call, outs, want, False, "rt_temporal_accumulate_moving")
t.close()
print("device path ok")
