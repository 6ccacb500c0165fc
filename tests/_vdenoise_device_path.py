"""Helper of tests/test_gpu_vdenoise.py::test_device_path (run as a script): rt_denoise_variance and rt_luminance_moments on
torch tensors -- device memory, the call ordered on the handle's stream between the current torch stream's work -- against
the host forms bit for bit: every plane at its least alignment, `out` aliasing `color`, a NULL colour for the handle's image
(into another tensor, and into the image itself), and the image left alone when `out` is elsewhere.  torch is imported first
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


def same(got, want, what):
    for a, b in zip(got, want) if isinstance(got, tuple) else ((got, want),):
        assert isinstance(a, torch.Tensor) and a.dtype == torch.float32 and tuple(a.shape) == b.shape, what
        assert np.array_equal(bits(a.cpu().numpy()), bits(b)), what


def desc(W, H, n):
    return A.VDenoiseDesc(struct_bytes=C.sizeof(A.VDenoiseDesc), width=W, height=H, iterations=n, sigma_luminance=SIGMAS[0],
                          sigma_normal=SIGMAS[1], sigma_point=SIGMAS[2], min_history=4.0)


t = rt.RayTracer(0, 130, 70)
t.load_scene(rt.SceneArrays.load(os.path.join(HERE, "golden", "cornell_scene.npz")))
for W, H in ((67, 45), (130, 70), (1, 1)):
    host_g = t.render_gbuffer(rt.make_params(W, H, 1, 1), CHANNELS)
    dev_g = t.render_gbuffer(rt.make_params(W, H, 1, 1), CHANNELS, device=True)
    t.render(rt.make_params(W, H, 4, 8, skybox=1, frames=-1))
    other = t.read_image(W, H).copy()
    t.render(rt.make_params(W, H, 4, 8, skybox=1, frames=0))
    image = t.read_image(W, H).copy()
    color = torch.from_numpy(image).to(dev)
    # the moments of the two frames, on the device and on the host, and a history that puts both branches in the frame
    lm = t.luminance_moments(dev_g, color)
    same(lm, rt.luminance_moments_host(host_g, image), (W, H, "moments"))
    same(t.luminance_moments(dev_g), rt.luminance_moments_host(host_g, image), (W, H, "moments of the image"))
    lm2 = t.luminance_moments({k: dev_g[k] for k in ("normal", "point")}, torch.from_numpy(other).to(dev))
    same(lm2, rt.luminance_moments_host({k: host_g[k] for k in ("normal", "point")}, other), (W, H, "moments, no optional plane"))
    moments = 0.5 * lm + 0.5 * t.luminance_moments(dev_g, torch.from_numpy(other).to(dev))
    history = torch.ones((H, W), dtype=torch.float32, device=dev)
    history[:, :(W + 1) // 2] = 8.0
    host_m, host_h = moments.cpu().numpy(), history.cpu().numpy()
    for n in (1, 3, 5):
        want = rt.denoise_variance_host(host_g, image, n, *SIGMAS, moments=host_m, history=host_h, out_variance=True)
        same(t.denoise_variance(dev_g, color, n, *SIGMAS, moments=moments, history=history, out_variance=True), want, (W, H, n))
        var = torch.empty((H, W), dtype=torch.float32, device=dev)
        got = t.denoise_variance(dev_g, color, n, *SIGMAS, moments=moments, history=history, out_variance=var)
        assert got[1] is var
        same(got, want, (W, H, n, "out_variance given"))
        sub = {k: dev_g[k] for k in ("normal", "point")}
        want2 = rt.denoise_variance_host({k: host_g[k] for k in sub}, image, n, *SIGMAS)
        same(t.denoise_variance(sub, color, n, *SIGMAS), want2[..., :], (W, H, n, "no optional plane"))
    want = rt.denoise_variance_host(host_g, image, 3, *SIGMAS, moments=host_m, history=host_h)
    kw = dict(moments=moments, history=history)
    # out aliasing color
    buf = color.clone()
    assert t.denoise_variance(dev_g, buf, 3, *SIGMAS, out=buf, **kw) is buf
    same(buf, want, (W, H, "out is color"))
    # a NULL colour is the handle's image (the frame rendered above); the image keeps its bits when out is elsewhere
    same(t.denoise_variance(dev_g, None, 3, *SIGMAS, **kw), want, (W, H, "NULL colour"))
    assert np.array_equal(bits(t.read_image(W, H)), bits(image)), (W, H, "the image changed")
    # ... and may be the output too: the image denoised in place
    d = desc(W, H, 3)
    for k in CHANNELS:
        setattr(d, k, dev_g[k].data_ptr())
    d.moments, d.history, d.out = moments.data_ptr(), history.data_ptr(), t.device_image_ptr
    torch.cuda.synchronize()
    t._check(t._L.rt_denoise_variance(t._h, C.byref(d), 0))
    assert np.array_equal(bits(t.read_image(W, H)), bits(want)), (W, H, "the image in place")
    print(W, H, "device path == host path", flush=True)

# the least alignment the contract allows: normal, point, history and out_variance at an odd multiple of 4 bytes, the float4
# planes at an odd multiple of 16; nothing is written outside the outputs
W, H = 67, 45
t.render(rt.make_params(W, H, 4, 8, skybox=1, frames=0))
image = t.read_image(W, H).copy()
host_g = t.render_gbuffer(rt.make_params(W, H, 1, 1), CHANNELS)
host_m = rt.luminance_moments_host(host_g, image)
host_h = np.where(np.arange(W)[None, :] % 2 == 0, np.float32(6), np.float32(2)) * np.ones((H, 1), np.float32)
want = rt.denoise_variance_host(host_g, image, 4, *SIGMAS, moments=host_m, history=host_h, out_variance=True)
planes = dict(host_g, color=image, moments=host_m, history=host_h.astype(np.float32), out=np.zeros_like(image),
              out_variance=np.zeros((H, W), np.float32))
for fn, outs, wants in ((t._L.rt_denoise_variance, ("out", "out_variance"), want),
                        (t._L.rt_luminance_moments, ("out",), (host_m,))):
    d = desc(W, H, 4)
    raw, skew = {}, {}
    for k, v in planes.items():
        skew[k] = 16 if A.VDENOISE_PLANES[k][1] == 4 else 4
        raw[k] = torch.zeros(v.nbytes + 64, dtype=torch.uint8, device=dev)
        assert raw[k].data_ptr() % 32 == 0
        raw[k][skew[k]:skew[k] + v.nbytes] = torch.from_numpy(v.view(np.uint8).ravel().copy()).to(dev)
        setattr(d, k, raw[k].data_ptr() + skew[k])
    torch.cuda.synchronize()
    t._check(fn(t._h, C.byref(d), 0))
    t.synchronize()
    for k, w in zip(outs, wants):
        got = raw[k].cpu().numpy()
        n, s = planes[k].nbytes, skew[k]
        assert np.array_equal(got[s:s + n].view(np.uint32), bits(w).ravel()), (k, "planes at their least alignment")
        assert not got[:s].any() and not got[s + n:].any(), (k, "bytes outside the plane")
    for k in planes:
        if k not in outs:
            assert np.array_equal(raw[k].cpu().numpy()[skew[k]:skew[k] + planes[k].nbytes], planes[k].view(np.uint8).ravel()), (k, "an input changed")
print("planes at their least alignment ok", flush=True)

# a handle that already holds more than option max_device_mb allows (the denoisers' scratch, once the cap is lowered under
# it): both calls on device memory are refused, rt_luminance_moments too, which uses no scratch, and nothing is written
host_g, dev_g, image = OC.frame(t)
guides, host_guides, color = {k: dev_g[k] for k in CHANNELS}, {k: host_g[k] for k in CHANNELS}, torch.from_numpy(image).to(dev)
out = torch.empty((OC.H, OC.W, 4), dtype=torch.float32, device=dev)
var = torch.empty((OC.H, OC.W), dtype=torch.float32, device=dev)
want = rt.denoise_variance_host(host_guides, image, 2, *SIGMAS, out_variance=True)
t.denoise_variance(guides, color, 2, *SIGMAS, out=out, out_variance=var)
OC.over_cap(t, lambda: t.denoise_variance(guides, color, 2, *SIGMAS, out=out, out_variance=var), (out, var), want, True,
            "rt_denoise_variance")
OC.over_cap(t, lambda: t.luminance_moments(guides, color, out=out), (out,), (rt.luminance_moments_host(host_guides, image),), True,
            "rt_luminance_moments")
t.close()
print("device path ok")
