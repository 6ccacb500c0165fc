"""Helper of tests/test_gpu_denoise.py::test_device_path (run as a script): rt_denoise on torch tensors -- device memory, the
call ordered on the handle's stream between the current torch stream's work -- against the host path bit for bit: every
plane at its least alignment, `out` aliasing `color`, a NULL colour for the handle's image (into another tensor, and into
the image itself), and the image left alone when `out` is elsewhere.  torch is imported first
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
import _over_cap as OC  # noqa: E402

SIGMAS = (4.0, 0.3, 1.0)
CHANNELS = ("normal", "point", "albedo", "emission")
dev = torch.device("cuda:0")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


t = rt.RayTracer(0, 130, 70)
t.load_scene(rt.SceneArrays.load(os.path.join(HERE, "golden", "cornell_scene.npz")))
for W, H in ((67, 45), (130, 70), (1, 1)):
    pr = rt.make_params(W, H, 4, 8, skybox=1, frames=0)
    t.render(pr)
    image = t.read_image(W, H).copy()
    host_g = t.render_gbuffer(rt.make_params(W, H, 1, 1), CHANNELS)
    dev_g = t.render_gbuffer(rt.make_params(W, H, 1, 1), CHANNELS, device=True)
    color = torch.from_numpy(image).to(dev)
    for n in (1, 3, 5):
        want = rt.denoise_host(host_g, image, n, *SIGMAS)
        got = t.denoise(dev_g, color, n, *SIGMAS)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float32 and tuple(got.shape) == (H, W, 4)
        assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (W, H, n)
        sub = {k: dev_g[k] for k in ("normal", "point")}
        want2 = rt.denoise_host({k: host_g[k] for k in sub}, image, n, *SIGMAS)
        assert np.array_equal(bits(t.denoise(sub, color, n, *SIGMAS).cpu().numpy()), bits(want2)), (W, H, n, "no optional plane")
    want = rt.denoise_host(host_g, image, 3, *SIGMAS)
    # out aliasing color
    buf = color.clone()
    assert t.denoise(dev_g, buf, 3, *SIGMAS, out=buf) is buf
    assert np.array_equal(bits(buf.cpu().numpy()), bits(want)), (W, H, "out is color")
    # a NULL colour is the handle's image (the frame rendered above); the image keeps its bits when out is elsewhere
    got = t.denoise(dev_g, None, 3, *SIGMAS)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (W, H, "NULL colour")
    assert np.array_equal(bits(t.read_image(W, H)), bits(image)), (W, H, "the image changed")
    # ... and may be the output too: the image denoised in place
    d = A.DenoiseDesc(struct_bytes=C.sizeof(A.DenoiseDesc), width=W, height=H, iterations=3, sigma_color=SIGMAS[0],
                      sigma_normal=SIGMAS[1], sigma_point=SIGMAS[2])
    for k in CHANNELS:
        setattr(d, k, dev_g[k].data_ptr())
    d.out = t.device_image_ptr
    torch.cuda.synchronize()
    t._check(t._L.rt_denoise(t._h, C.byref(d), 0))
    assert np.array_equal(bits(t.read_image(W, H)), bits(want)), (W, H, "the image in place")
    print(W, H, "device path == host path", flush=True)

# the least alignment the contract allows: normal and point at an odd multiple of 4 bytes, the float4 planes at an odd
# multiple of 16; nothing is written outside `out`
W, H = 67, 45
t.render(rt.make_params(W, H, 4, 8, skybox=1, frames=0))
image = t.read_image(W, H).copy()
host_g = t.render_gbuffer(rt.make_params(W, H, 1, 1), CHANNELS)
want = rt.denoise_host(host_g, image, 4, *SIGMAS)
planes = dict(host_g, color=image, out=np.zeros_like(image))
d = A.DenoiseDesc(struct_bytes=C.sizeof(A.DenoiseDesc), width=W, height=H, iterations=4, sigma_color=SIGMAS[0],
                  sigma_normal=SIGMAS[1], sigma_point=SIGMAS[2])
raw, skew = {}, {}
for k, v in planes.items():
    skew[k] = 4 if k in ("normal", "point") else 16
    raw[k] = torch.zeros(v.nbytes + 64, dtype=torch.uint8, device=dev)
    assert raw[k].data_ptr() % 32 == 0
    raw[k][skew[k]:skew[k] + v.nbytes] = torch.from_numpy(v.view(np.uint8).ravel().copy()).to(dev)
    setattr(d, k, raw[k].data_ptr() + skew[k])
torch.cuda.synchronize()
t._check(t._L.rt_denoise(t._h, C.byref(d), 0))
t.synchronize()
got = raw["out"].cpu().numpy()
n = image.nbytes
assert np.array_equal(got[16:16 + n].view(np.uint32), bits(want).ravel()), "planes at their least alignment"
assert not got[:16].any() and not got[16 + n:].any(), "bytes outside the plane"
for k in planes:
    if k != "out":
        assert np.array_equal(raw[k].cpu().numpy()[skew[k]:skew[k] + planes[k].nbytes], planes[k].view(np.uint8).ravel()), (k, "an input changed")
print("planes at their least alignment ok", flush=True)

# a handle that already holds more than option max_device_mb allows (its own scratch, once the cap is lowered under it):
# rt_denoise on device memory is refused, and nothing is written
host_g, dev_g, image = OC.frame(t)
guides, color = {k: dev_g[k] for k in CHANNELS}, torch.from_numpy(image).to(dev)
out = torch.empty((OC.H, OC.W, 4), dtype=torch.float32, device=dev)
want = rt.denoise_host({k: host_g[k] for k in CHANNELS}, image, 2, *SIGMAS)
t.denoise(guides, color, 2, *SIGMAS, out=out)
OC.over_cap(t, lambda: t.denoise(guides, color, 2, *SIGMAS, out=out), (out,), (want,), True, "rt_denoise")
t.close()
print("device path ok")
