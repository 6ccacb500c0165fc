"""Helper of tests/test_gpu_upsample.py::test_device_path (run as a script): rt_upsample on torch tensors -- device memory, the
call ordered on the handle's stream between the current torch stream's work -- against the host restatement bit for bit: the
optional planes and `coverage` on and off, the outputs given, a NULL lo_color for the handle's image after rt_render at the
low size (the header's consequence 2 among it), the image left alone, every plane at its least alignment, and a handle over
its memory cap.  torch is imported first (ray_tracer_2_amd/__init__.py: its HIP runtime then serves the library too)."""
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
import _upsample_reference as R  # noqa: E402
import _over_cap as OC  # noqa: E402

CHANNELS = ("depth", "point", "normal", "object", "albedo", "emission")
LO = ("point", "normal", "object", "albedo")
dev = torch.device("cuda:0")


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want, what):
    out, cov = got
    assert isinstance(out, torch.Tensor) and out.dtype == torch.float32 and tuple(out.shape) == want[0].shape, what
    assert np.array_equal(bits(out), bits(want[0])), (what, "out")
    assert isinstance(cov, torch.Tensor) and cov.dtype == torch.uint8 and np.array_equal(cov.cpu().numpy(), want[1]), (what, "coverage")


arrays = rt.SceneArrays.load(os.path.join(HERE, "golden", "cornell_scene.npz"))
t = rt.RayTracer(0, 130, 70)
t.load_scene(arrays)
for w, h, W, H in ((34, 23, 67, 45), (66, 36, 130, 70), (67, 45, 34, 23)):
    lo_p, hi_p = rt.make_params(w, h, 1, 1), rt.make_params(W, H, 1, 1)
    host_lo, dev_lo = ({k: v for k, v in t.render_gbuffer(lo_p, LO, device=d).items()} for d in (False, True))
    host_hi, dev_hi = (t.render_gbuffer(hi_p, CHANNELS, device=d) for d in (False, True))
    t.render(rt.make_params(w, h, 4, 8, skybox=1, frames=0))   # the low frame stays in the handle's image
    image = t.read_image(w, h).copy()
    color = torch.from_numpy(image).to(dev)
    for albedo, emission in ((True, True), (True, False), (False, True), (False, False)):
        drop = (() if albedo else ("albedo",)) + (() if emission else ("emission",))
        hl, dl, hh, dh = (R.without(g, *drop) for g in (host_lo, dev_lo, host_hi, dev_hi))
        want = rt.upsample_host(hl, hh, image, coverage=True)
        same(t.upsample(dl, dh, color, coverage=True), want, (w, h, W, H, albedo, emission))
        alone = t.upsample(dl, dh, color)
        assert isinstance(alone, torch.Tensor) and np.array_equal(bits(alone), bits(want[0])), (w, h, W, H, "without coverage")
    want = rt.upsample_host(host_lo, host_hi, image, coverage=True)
    assert (want[1] == 2).mean() > 0.5
    # the outputs given
    out, cov = torch.zeros((H, W, 4), device=dev), torch.zeros((H, W), dtype=torch.uint8, device=dev)
    got = t.upsample(dev_lo, dev_hi, color, out=out, coverage=cov)
    assert got[0] is out and got[1] is cov
    same(got, want, (w, h, W, H, "outputs given"))
    # a NULL lo_color is the handle's image (the frame rendered above), which keeps its bits
    same(t.upsample(dev_lo, dev_hi, None, coverage=True), want, (w, h, W, H, "NULL lo_color"))
    assert np.array_equal(bits(t.read_image(w, h)), bits(image)), (w, h, "the image changed")
    if (W, H) == (2 * w - 1, 2 * h - 1):
        # consequence 2: the even texels are the image's texels
        got = t.upsample(R.without(dev_lo, "albedo"), R.without(dev_hi, "albedo"), None)
        assert np.isfinite(image).all() and np.array_equal(bits(got)[::2, ::2], bits(image)), (w, h, "consequence 2")
    print(w, h, W, H, "device path == host", flush=True)

# the least alignment the contract allows: the planes of 4-byte elements at an odd multiple of 4 bytes, the float4 planes at
# an odd multiple of 16, coverage at an odd address; nothing is written outside the outputs
w, h, W, H = 34, 23, 67, 45
host_lo, host_hi = t.render_gbuffer(rt.make_params(w, h, 1, 1), LO), t.render_gbuffer(rt.make_params(W, H, 1, 1), CHANNELS)
t.render(rt.make_params(w, h, 4, 8, skybox=1, frames=0))
image = t.read_image(w, h).copy()
want = rt.upsample_host(host_lo, host_hi, image, coverage=True)
planes = dict(lo_color=image, **{"lo_" + k: host_lo[k] for k in LO}, **{k: host_hi[k] for k in CHANNELS},
              out=np.zeros((H, W, 4), np.float32), coverage=np.zeros((H, W), np.uint8))
d = A.UpsampleDesc(struct_bytes=C.sizeof(A.UpsampleDesc), lo_width=w, lo_height=h, width=W, height=H, point_tolerance=0.02, normal_cos=0.9)
align = {"lo_color": 16, "lo_albedo": 16, "albedo": 16, "emission": 16, "out": 16, "coverage": 1}
raw, skew = {}, {}
for k, v in planes.items():
    skew[k] = align.get(k, 4)
    raw[k] = torch.zeros(v.nbytes + 64, dtype=torch.uint8, device=dev)
    assert raw[k].data_ptr() % 32 == 0
    raw[k][skew[k]:skew[k] + v.nbytes] = torch.from_numpy(v.view(np.uint8).ravel().copy()).to(dev)
    setattr(d, k, raw[k].data_ptr() + skew[k])
torch.cuda.synchronize()
t._check(t._L.rt_upsample(t._h, C.byref(d), 0))
t.synchronize()
for k, wnt in zip(("out", "coverage"), want):
    got = raw[k].cpu().numpy()
    n = planes[k].nbytes
    assert np.array_equal(got[skew[k]:skew[k] + n], np.ascontiguousarray(wnt).view(np.uint8).ravel()), (k, "planes at their least alignment")
    assert not got[:skew[k]].any() and not got[skew[k] + n:].any(), (k, "bytes outside the plane")
for k in planes:
    if k not in ("out", "coverage"):
        assert np.array_equal(raw[k].cpu().numpy()[skew[k]:skew[k] + planes[k].nbytes], planes[k].view(np.uint8).ravel()), (k, "an input changed")
print("planes at their least alignment ok", flush=True)

# a handle that already holds more than option max_device_mb allows (the denoiser's scratch, once the cap is lowered under
# it): rt_upsample on device memory allocates nothing and is done all the same
host_hi, dev_hi, _ = OC.frame(t, 1)
w, h = 97, 49
host_lo, dev_lo = (t.render_gbuffer(rt.make_params(w, h, 1, 1), LO, device=d) for d in (False, True))
image = np.random.default_rng(2).random((h, w, 4), np.float32) + np.float32(0.25)
color = torch.from_numpy(image).to(dev)
hi_of = lambda g: dict({k: g[k] for k in ("point", "normal", "object", "albedo", "emission")}, depth=g["depth"])  # noqa: E731
host_hi["depth"], dev_hi["depth"] = (t.render_gbuffer(rt.make_params(OC.W, OC.H, 1, 1), ("depth",), device=d)["depth"] for d in (False, True))
outs = (torch.empty((OC.H, OC.W, 4), dtype=torch.float32, device=dev), torch.empty((OC.H, OC.W), dtype=torch.uint8, device=dev))
want = rt.upsample_host(host_lo, hi_of(host_hi), image, coverage=True)
call = lambda: t.upsample(dev_lo, hi_of(dev_hi), color, out=outs[0], coverage=outs[1])  # noqa: E731
call()
OC.hold_denoise_scratch(t, dev_hi, color.new_zeros((OC.H, OC.W, 4)) + 0.5)
OC.over_cap(t, call, outs, want, False, "rt_upsample")
t.close()
print("device path ok")
