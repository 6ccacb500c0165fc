"""Helper of tests/test_gpu_temporal_deform.py::test_device_path (run as a script): rt_temporal_accumulate_deforming on torch
tensors -- device memory, a device-resident motion table and triangle array, the call ordered on the handle's stream between
the current torch stream's work -- against the host restatement bit for bit, on the 37x19 and 70x21 synthetic frames of the
CPU tests: prev_object and motion on and off, `out` aliasing `color`, a NULL colour for the handle's image (into other
tensors, and into the image itself, read back by the read_image that follows), and every plane and both arrays at their
least alignment with nothing written outside the outputs.  torch is imported first (ray_tracer_2_amd/__init__.py: its HIP
runtime then serves the library too)."""
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
import _temporal_deform_reference as D  # noqa: E402

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


def tensor(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).to(dev)


t = rt.RayTracer(0, 70, 21)
for W, H in ((37, 19), (70, 21)):
    planes, cam, table, tris, _ = D.synthetic_case(W, H)
    g, pg = D.split(planes)
    dev_g, dev_pg = {k: tensor(v) for k, v in g.items()}, {k: tensor(v) for k, v in pg.items()}
    assert dev_g["flags"].dtype == torch.uint8 and dev_g["primitive"].dtype == torch.int32
    dev_table = tensor(table.view(np.uint32).reshape(-1, 24))
    dev_tris = tensor(tris.view(np.float32).reshape(-1, 24))
    color, prev_color, prev_history = (tensor(planes[k]) for k in ("color", "prev_color", "prev_history"))
    kw = dict(motions=dev_table, prev_triangles=dev_tris, tri_first=D.TRI_FIRST)
    hkw = dict(motions=table, prev_triangles=tris, tri_first=D.TRI_FIRST)
    for objects, motion in ((True, True), (True, False), (False, True), (False, False)):
        pick = (lambda d: d) if objects else (lambda d: {k: v for k, v in d.items() if k != "object"})
        want = rt.temporal_accumulate_host(g, pick(pg), cam, planes["prev_color"], planes["prev_history"], planes["color"], CAP, TOL, NCOS,
                                           motion=motion, **hkw)
        got = t.temporal_accumulate(dev_g, pick(dev_pg), cam, prev_color, prev_history, color, CAP, TOL, NCOS, motion=motion, **kw)
        same(got, want, (W, H, objects, motion))
    want = rt.temporal_accumulate_host(g, pg, cam, planes["prev_color"], planes["prev_history"], planes["color"], CAP, TOL, NCOS, motion=True, **hkw)
    deformed = planes["object"] >= 2
    assert (want[1][deformed] > 1).mean() > 0.4 and (want[1][deformed] == 1).any()
    # out aliasing color, the outputs given
    buf, hist, mot = color.clone(), torch.zeros((H, W), device=dev), torch.zeros((H, W, 2), device=dev)
    got = t.temporal_accumulate(dev_g, dev_pg, cam, prev_color, prev_history, buf, CAP, TOL, NCOS, out=buf, out_history=hist, motion=mot, **kw)
    assert got[0] is buf and got[1] is hist and got[2] is mot
    same(got, want, (W, H, "out is color"))
    # a NULL colour is the handle's image; the image keeps its bits when out is elsewhere
    t.write_image(planes["color"])
    got = t.temporal_accumulate(dev_g, dev_pg, cam, prev_color, prev_history, None, CAP, TOL, NCOS, motion=True, **kw)
    same(got, want, (W, H, "NULL colour"))
    assert np.array_equal(bits(t.read_image(W, H)), bits(planes["color"])), (W, H, "the image changed")
    # ... and may be the output too: the image accumulated in place, and the read_image that follows sees the result
    d = A.TemporalDeformDesc(struct_bytes=C.sizeof(A.TemporalDeformDesc), width=W, height=H,
                             prev_camera=A.CameraUniform.from_buffer_copy(bytes(cam)), max_history=CAP, point_tolerance=TOL, normal_cos=NCOS,
                             motions=dev_table.data_ptr(), n_objects=len(table), prev_triangles=dev_tris.data_ptr(),
                             tri_first=D.TRI_FIRST, n_prev_triangles=len(tris))
    for k in ("point", "normal", "object"):
        setattr(d, k, dev_g[k].data_ptr())
        setattr(d, "prev_" + k, dev_pg[k].data_ptr())
    for k in D.GUIDES:
        setattr(d, k, dev_g[k].data_ptr())
    d.prev_color, d.prev_history = prev_color.data_ptr(), prev_history.data_ptr()
    hist.zero_()
    d.out, d.out_history = t.device_image_ptr, hist.data_ptr()
    torch.cuda.synchronize()
    t._check(t._L.rt_temporal_accumulate_deforming(t._h, C.byref(d), 0))
    assert np.array_equal(bits(t.read_image(W, H)), bits(want[0])), (W, H, "the image in place")
    assert np.array_equal(bits(hist), bits(want[1])), (W, H, "the image in place: history")
    print(W, H, "device path == host", flush=True)

# the least alignment the contract allows: the planes of 4-byte elements at an odd multiple of 4 bytes, motion at an odd
# multiple of 8, the float4 planes, the table and the triangles at an odd multiple of 16, flags at an odd address; nothing is
# written outside the outputs
assert (W, H) == (70, 21)   # (the frames of the loop's last round)
arrays = {k: np.ascontiguousarray(v) for k, v in planes.items()}
arrays.update(out=np.zeros((H, W, 4), np.float32), out_history=np.zeros((H, W), np.float32), motion=np.zeros((H, W, 2), np.float32),
              motions=table, prev_triangles=tris)
assert set(arrays) == set(A.TEMPORAL_DEFORM_PLANES)
d = A.TemporalDeformDesc(struct_bytes=C.sizeof(A.TemporalDeformDesc), width=W, height=H, prev_camera=A.CameraUniform.from_buffer_copy(bytes(cam)),
                         max_history=CAP, point_tolerance=TOL, normal_cos=NCOS, n_objects=len(table), tri_first=D.TRI_FIRST,
                         n_prev_triangles=len(tris))
align = {"color": 16, "prev_color": 16, "out": 16, "motion": 8, "motions": 16, "prev_triangles": 16, "flags": 1}
raw, skew = {}, {}
for k, v in arrays.items():
    skew[k] = align.get(k, 4)
    raw[k] = torch.zeros(v.nbytes + 64, dtype=torch.uint8, device=dev)
    assert raw[k].data_ptr() % 32 == 0
    raw[k][skew[k]:skew[k] + v.nbytes] = torch.from_numpy(v.view(np.uint8).ravel().copy()).to(dev)
    setattr(d, k, raw[k].data_ptr() + skew[k])
torch.cuda.synchronize()
t._check(t._L.rt_temporal_accumulate_deforming(t._h, C.byref(d), 0))
t.synchronize()
for k, w in zip(("out", "out_history", "motion"), want):
    got = raw[k].cpu().numpy()
    n = arrays[k].nbytes
    assert np.array_equal(got[skew[k]:skew[k] + n].view(np.uint32), bits(w).ravel()), (k, "planes at their least alignment")
    assert not got[:skew[k]].any() and not got[skew[k] + n:].any(), (k, "bytes outside the plane")
for k in arrays:
    if k not in ("out", "out_history", "motion"):
        assert np.array_equal(raw[k].cpu().numpy()[skew[k]:skew[k] + arrays[k].nbytes], arrays[k].view(np.uint8).ravel()), (k, "an input changed")
print("planes at their least alignment ok", flush=True)
t.close()
print("device path ok")
