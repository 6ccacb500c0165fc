"""Helper of tests/test_gpu_rectify.py::test_device_path (run as a script): rt_temporal_rectify on torch tensors -- device
memory, the call ordered on the handle's stream between the current torch stream's work -- against the host restatement bit
for bit: the optional planes and out_clipped on and off, the outputs given and in place (out = history), a NULL colour for
the handle's image, which keeps its bits, an `out` in the image refused, temporal_reproject on tensors with its cached NaN
plane, every plane at its least alignment, and a handle over its memory cap.  torch is imported first
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
import _rectify_reference as R  # noqa: E402
import _over_cap as OC  # noqa: E402

CHANNELS = ("point", "normal", "object", "albedo")
NAMES = ("out", "out_history", "out_moments", "out_clipped")
dev = torch.device("cuda:0")


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a).view(np.uint8)


def same(got, want, what):
    assert len(got) == len(want), what
    for a, b in zip(got, want):
        kind = torch.uint8 if b.dtype == np.uint8 else torch.float32
        assert isinstance(a, torch.Tensor) and a.dtype == kind and tuple(a.shape) == b.shape, what
        assert np.array_equal(bits(a), bits(b)), what


def to_dev(kw):
    return {k: torch.from_numpy(np.ascontiguousarray(v).view(np.int32) if v.dtype == np.uint32 else np.ascontiguousarray(v)).to(dev)
            for k, v in kw.items()}


arrays = rt.SceneArrays.load(os.path.join(HERE, "golden", "cornell_scene.npz"))
cam = arrays.uniform.camera
t = rt.RayTracer(0, 130, 70)
t.load_scene(arrays)
for W, H in ((67, 45), (130, 70)):
    g = t.render_gbuffer(rt.make_params(W, H, 1, 1), CHANNELS)
    dev_g = t.render_gbuffer(rt.make_params(W, H, 1, 1), CHANNELS, device=True)
    t.render(rt.make_params(W, H, 4, 8, skybox=1, frames=0))
    prev_image = t.read_image(W, H).copy()
    t.render(rt.make_params(W, H, 4, 8, skybox=1, frames=-1))   # the new frame stays in the handle's image
    image = t.read_image(W, H).copy()
    length = np.random.default_rng(W).integers(1, 9, (H, W)).astype(np.float32)
    planes = dict(color=image, history=prev_image, history_length=length, object=g["object"], moments=rt.luminance_moments_host(g, image),
                  history_moments=rt.luminance_moments_host(g, prev_image))
    for name, kw in R.variants(planes):
        for radius in (1, 2, 3):
            want = rt.temporal_rectify_host(**kw, radius=radius, clipped=True)
            same(t.temporal_rectify(**to_dev(kw), radius=radius, clipped=True), want, (W, H, name, radius))
            same(t.temporal_rectify(**to_dev(kw), radius=radius), want[:-1], (W, H, name, radius, "without out_clipped"))
    kw = dict(R.variants(planes))["all"]
    want = rt.temporal_rectify_host(**kw, clipped=True)
    assert (want[3] == R.CLIPPED).mean() > 0.05 and (want[3] == R.KEPT).mean() > 0.05
    # the outputs given, and in place: out = history, out_history = history_length, out_moments = history_moments
    d = to_dev(kw)
    clip = torch.zeros((H, W), dtype=torch.uint8, device=dev)
    got = t.temporal_rectify(**d, out=d["history"], out_history=d["history_length"], out_moments=d["history_moments"], clipped=clip)
    assert got[0] is d["history"] and got[1] is d["history_length"] and got[2] is d["history_moments"] and got[3] is clip
    same(got, want, (W, H, "in place"))
    # a NULL colour is the handle's image (the frame rendered above), which keeps its bits
    d = to_dev(kw)
    del d["color"]
    same(t.temporal_rectify(None, **d, clipped=True), want, (W, H, "NULL colour"))
    assert np.array_equal(bits(t.read_image(W, H)), bits(image)), (W, H, "the image changed")
    # ... and must not be the output: the neighbours read it
    desc = A.RectifyDesc(struct_bytes=C.sizeof(A.RectifyDesc), width=W, height=H, radius=3, clip_sigma=1.0, clip_history=4.0)
    for k, v in d.items():
        setattr(desc, k, v.data_ptr())
    hist = torch.full((H, W), -7.25, device=dev)
    desc.out, desc.out_history, desc.out_moments = t.device_image_ptr, hist.data_ptr(), d["history_moments"].data_ptr()
    torch.cuda.synchronize()
    assert t._L.rt_temporal_rectify(t._h, C.byref(desc), 0) == -1 and b"overlaps the image" in t._L.rt_last_error(t._h)
    t.synchronize()
    assert np.array_equal(bits(t.read_image(W, H)), bits(image)) and (hist == -7.25).all().item(), (W, H, "a refused call wrote")
    # temporal_reproject on tensors: the host's bits; one NaN plane per size, kept by the handle and left as it is
    pg = {k: g[k] for k in ("point", "normal", "object")}
    dpg = {k: dev_g[k] for k in ("point", "normal", "object")}
    hw = rt.temporal_reproject_host(pg, pg, cam, prev_image, length, motion=True)
    for _ in range(2):
        hd = t.temporal_reproject(dpg, dpg, cam, torch.from_numpy(prev_image).to(dev), torch.from_numpy(length).to(dev), motion=True)
        same(hd, hw, (W, H, "reproject"))
    assert set(t._nan_planes) >= {(H, W)} and torch.isnan(t._nan_planes[(H, W)]).all().item()
    acc = rt.temporal_accumulate_host(pg, pg, cam, prev_image, length, image)
    same(t.temporal_rectify(None, hd[0], hd[1], clip_sigma=float("inf")), acc, (W, H, "consequence 1 on tensors"))
    print(W, H, "device path == host", flush=True)
assert len(t._nan_planes) == 2

# the least alignment the contract allows: the planes of 4-byte elements at an odd multiple of 4 bytes, the float4 planes at
# an odd multiple of 16, out_clipped at an odd address; nothing is written outside the outputs
planes = dict(kw, out=np.zeros((H, W, 4), np.float32), out_history=np.zeros((H, W), np.float32), out_moments=np.zeros((H, W, 4), np.float32),
              out_clipped=np.zeros((H, W), np.uint8))
assert list(planes) == list(A.RECTIFY_PLANES)
desc = A.RectifyDesc(struct_bytes=C.sizeof(A.RectifyDesc), width=W, height=H, radius=3, clip_sigma=1.0, clip_history=4.0)
align = {"history_length": 4, "object": 4, "out_history": 4, "out_clipped": 1}
raw, skew = {}, {}
for k, v in planes.items():
    skew[k] = align.get(k, 16)
    raw[k] = torch.zeros(v.nbytes + 64, dtype=torch.uint8, device=dev)
    assert raw[k].data_ptr() % 32 == 0
    raw[k][skew[k]:skew[k] + v.nbytes] = torch.from_numpy(v.view(np.uint8).ravel().copy()).to(dev)
    setattr(desc, k, raw[k].data_ptr() + skew[k])
torch.cuda.synchronize()
t._check(t._L.rt_temporal_rectify(t._h, C.byref(desc), 0))
t.synchronize()
for k, w in zip(NAMES, want):
    got = raw[k].cpu().numpy()
    n = planes[k].nbytes
    assert np.array_equal(got[skew[k]:skew[k] + n], bits(w).ravel()), (k, "planes at their least alignment")
    assert not got[:skew[k]].any() and not got[skew[k] + n:].any(), (k, "bytes outside the plane")
for k in planes:
    if k not in NAMES:
        assert np.array_equal(raw[k].cpu().numpy()[skew[k]:skew[k] + planes[k].nbytes], planes[k].view(np.uint8).ravel()), (k, "an input changed")
print("planes at their least alignment ok", flush=True)

# a handle that already holds more than option max_device_mb allows (the denoiser's scratch, once the cap is lowered under
# it): rt_temporal_rectify on device memory allocates nothing and is done all the same
host_g, dev_g, image = OC.frame(t, 1)
rng = np.random.default_rng(4)
f = lambda *s: (rng.random(s, np.float32) + np.float32(0.25))  # noqa: E731
kw = dict(color=image, history=f(OC.H, OC.W, 4), history_length=rng.integers(1, 9, (OC.H, OC.W)).astype(np.float32), object=host_g["object"],
          moments=f(OC.H, OC.W, 4), history_moments=f(OC.H, OC.W, 4))
d = to_dev(kw)
outs = (torch.empty((OC.H, OC.W, 4), device=dev), torch.empty((OC.H, OC.W), device=dev), torch.empty((OC.H, OC.W, 4), device=dev),
        torch.empty((OC.H, OC.W), dtype=torch.uint8, device=dev))
want = rt.temporal_rectify_host(**kw, clipped=True)
call = lambda: t.temporal_rectify(**d, out=outs[0], out_history=outs[1], out_moments=outs[2], clipped=outs[3])  # noqa: E731
call()
OC.hold_denoise_scratch(t, dev_g, d["color"])
OC.over_cap(t, call, outs, want, False, "rt_temporal_rectify")
t.close()
print("device path ok")
