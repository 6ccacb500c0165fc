"""Helper of tests/test_gpu_display.py::test_device_path (run as a script): rt_display, rt_auto_exposure and
rt_snapshot_display on torch tensors -- device memory, the calls ordered on the handle's stream between the current torch
stream's work -- against the host restatements bit for bit: a NULL color for the handle's image after rt_render, the image
left alone, the scale handed from the meter to the display pass on the device with nothing read back in between, the outputs
given, every plane at its least alignment, and a handle over its memory cap.  torch is imported first
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
import _display_reference as R  # noqa: E402
import _over_cap as OC  # noqa: E402

dev = torch.device("cuda:0")
U32 = np.uint32


def same_bytes(got, want, what):
    assert isinstance(got, torch.Tensor) and got.dtype == torch.uint8 and tuple(got.shape) == want.shape, what
    assert np.array_equal(got.cpu().numpy(), want), what


def same_float(got, want, what):
    assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and tuple(got.shape) == (1,), what
    assert got.cpu().numpy().view(U32)[0] == want.view(U32)[0], (what, got, want)


arrays = rt.SceneArrays.load(os.path.join(HERE, "golden", "cornell_scene.npz"))
t = rt.RayTracer(0, 192, 96)
t.load_scene(arrays)
KW = dict(tone="reinhard", white=4.0, bgra=True, top_first=True, exposure=1.25)
for W, H in ((64, 36), (130, 70), (33, 9)):
    t.render(rt.make_params(W, H, 4, 8, skybox=1, frames=0))   # the frame stays in the handle's image
    image = t.read_image(W, H).copy()
    color = torch.from_numpy(image).to(dev)
    # color=None is the handle's image, which keeps its bits
    same_bytes(t.display(None, width=W, height=H), rt.display_host(image), (W, H, "NULL color"))
    same_bytes(t.display(None, width=W, height=H, **KW), rt.display_host(image, **KW), (W, H, "NULL color, settings"))
    want_scale, want_hist = rt.auto_exposure_host(image, histogram=True)
    scale, hist = t.auto_exposure(None, width=W, height=H, histogram=True)
    same_float(scale, want_scale, (W, H, "meter, NULL color"))
    assert hist.dtype == torch.int32 and np.array_equal(hist.cpu().numpy().view(U32), want_hist), (W, H, "histogram")
    assert np.array_equal(t.read_image(W, H).view(U32), image.view(U32)), (W, H, "the image changed")
    # tensors given
    same_bytes(t.display(color, **KW), rt.display_host(image, **KW), (W, H, "tensor"))
    same_float(t.auto_exposure(color), want_scale, (W, H, "meter, tensor"))
    # the chain on the device: the meter's float goes to the display pass as a tensor, nothing comes to the host in between
    prev = torch.full((1,), 3.0, device=dev)
    s = t.auto_exposure(color, prev_scale=prev, rate=0.25, scale=prev)   # (in place: scale is prev_scale)
    assert s is prev
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
    got = t.display(color, exposure_scale=s, out=out, **KW)
    assert got is out
    host_s = rt.auto_exposure_host(image, prev_scale=3.0, rate=0.25)
    same_bytes(got, rt.display_host(image, exposure_scale=host_s, **KW), (W, H, "chain"))
    same_float(s, host_s, (W, H, "chain scale"))
    same_bytes(t.display(None, width=W, height=H, exposure_scale=t.auto_exposure(None, width=W, height=H)),
               rt.display_host(image, exposure_scale=want_scale), (W, H, "chain on the image"))
    # the display snapshot with the device-resident scale
    t.snapshot_display(W, H, exposure_scale=s, **KW)
    assert np.array_equal(t.read_display_snapshot(W, H), rt.display_host(image, exposure_scale=host_s, **KW)), (W, H, "snapshot")
    print(W, H, "device path == host", flush=True)

# the least alignment the contract allows: color at an odd multiple of 16 bytes, out, exposure_scale and the meter's small
# planes at an odd multiple of 4; nothing is written outside the outputs
W, H = 33, 9
image = R.threshold_frame(W, H)
scale_in = np.array([0.61], np.float32)


def skewed(planes, skews):
    raw = {}
    for k, v in planes.items():
        raw[k] = torch.zeros(v.nbytes + 64, dtype=torch.uint8, device=dev)
        assert raw[k].data_ptr() % 32 == 0
        raw[k][skews[k]:skews[k] + v.nbytes] = torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).ravel().copy()).to(dev)
    return raw


def inside(raw, planes, skews, k, want):
    got = raw[k].cpu().numpy()
    n = planes[k].nbytes
    assert np.array_equal(got[skews[k]:skews[k] + n], np.ascontiguousarray(want).view(np.uint8).ravel()), (k, "planes at their least alignment")
    assert not got[:skews[k]].any() and not got[skews[k] + n:].any(), (k, "bytes outside the plane")


planes = dict(color=image, exposure_scale=scale_in, out=np.zeros((H, W, 4), np.uint8))
skews = dict(color=16, exposure_scale=4, out=4)
raw = skewed(planes, skews)
d = A.DisplayDesc(struct_bytes=C.sizeof(A.DisplayDesc), width=W, height=H, exposure=1.0, white=1.0, layout=3)
for k in planes:
    setattr(d, k, raw[k].data_ptr() + skews[k])
torch.cuda.synchronize()
t._check(t._L.rt_display(t._h, C.byref(d), 0))
t.synchronize()
inside(raw, planes, skews, "out", rt.display_host(image, bgra=True, top_first=True, exposure_scale=scale_in))
inside(raw, planes, skews, "color", image)

planes = dict(color=image, prev_scale=np.array([2.5], np.float32), histogram=np.zeros(256, U32), scale=np.zeros(1, np.float32))
skews = dict(color=16, prev_scale=4, histogram=4, scale=4)
raw = skewed(planes, skews)
m = A.AutoExposureDesc(struct_bytes=C.sizeof(A.AutoExposureDesc), width=W, height=H, low_permille=100, high_permille=950, key=0.18,
                       min_scale=2.0 ** -10, max_scale=2.0 ** 10, rate=0.5)
for k in planes:
    setattr(m, k, raw[k].data_ptr() + skews[k])
torch.cuda.synchronize()
t._check(t._L.rt_auto_exposure(t._h, C.byref(m), 0))
t.synchronize()
ws, wh = rt.auto_exposure_host(image, prev_scale=2.5, rate=0.5, histogram=True)
inside(raw, planes, skews, "scale", ws)
inside(raw, planes, skews, "histogram", wh)
inside(raw, planes, skews, "color", image)
print("planes at their least alignment ok", flush=True)

# a handle that already holds more than option max_device_mb allows (the denoiser's scratch, once the cap is lowered under
# it): rt_display on device memory allocates nothing and is done all the same; rt_auto_exposure keeps a scratch, and the
# calls that do are refused once the handle is over its cap
_, dev_g, image = OC.frame(t, 1)
color = torch.from_numpy(image).to(dev)
out = torch.empty((OC.H, OC.W, 4), dtype=torch.uint8, device=dev)
scale = torch.empty((1,), dtype=torch.float32, device=dev)
show = lambda: t.display(color, out=out, **KW)  # noqa: E731
meter = lambda: t.auto_exposure(color, scale=scale)  # noqa: E731
show()
meter()
OC.hold_denoise_scratch(t, dev_g, color.new_zeros((OC.H, OC.W, 4)) + 0.5)
OC.over_cap(t, show, (out,), (rt.display_host(image, **KW),), False, "rt_display")
OC.over_cap(t, meter, (scale,), (rt.auto_exposure_host(image),), True, "rt_auto_exposure")
t.close()
print("device path ok")
