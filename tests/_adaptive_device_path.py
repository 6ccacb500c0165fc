"""Helper of tests/test_gpu_adaptive.py::test_device_path (run as a script): rt_adaptive_plan, rt_adaptive_merge and
RayTracer.adaptive_samples on torch tensors -- device memory, the calls ordered on the handle's stream between the current
torch stream's work, no host synchronisation inside adaptive_samples -- against the host forms bit for bit: a NULL colour
for the handle's image (into another tensor, and into the image itself), the outputs aliasing the inputs, every plane at its
least alignment, and the scratch's accounting on a frame large enough to show in whole MiB.  torch is imported first
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

F32, U32 = np.float32, np.uint32
dev = torch.device("cuda:0")


def raw(a):
    """The bytes of a tensor or an array."""
    if isinstance(a, torch.Tensor):
        a = a.cpu().numpy()
    return np.ascontiguousarray(a).view(np.uint8).ravel()


def same(got, want, what):
    for a, b in zip(got, want):
        assert np.array_equal(raw(a), raw(b)), what


def up(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == U32 else a).to(dev)


W, H = 67, 45
t = rt.RayTracer(0, 130, 70)
scene = rt.SceneArrays.load(os.path.join(HERE, "golden", "cornell_scene.npz"))
t.load_scene(scene)
origin = np.asarray(scene.uniform.camera.cam_to_world, F32)[3, :3].copy()
CH = ("dir", "normal", "point", "albedo", "emission")
host_g = t.render_gbuffer(rt.make_params(W, H, 1, 1), CH)
dev_g = t.render_gbuffer(rt.make_params(W, H, 1, 1), CH, device=True)
for f in range(4):
    t.render(rt.make_params(W, H, 4, 8, skybox=1, frames=f))
image = t.read_image(W, H).copy()
variance = t.denoise_variance(host_g, image, out_variance=True)[1]
moments = rt.luminance_moments_host(host_g, image)
hist = np.full((H, W), 4, F32)
budget = 4 * W * H

# the plan on device tensors
want_plan = rt.adaptive_plan_host(variance, host_g["dir"], origin, budget, 1, 16, 4)
got_plan = t.adaptive_plan(up(variance), dev_g["dir"], origin, budget, 1, 16, 4)
assert all(isinstance(v, torch.Tensor) for v in got_plan) and tuple(got_plan[2].shape) == (budget, 8)
same(got_plan, want_plan, "plan on tensors")
total = int(want_plan[3][0])
assert 0 < total < budget

# adaptive_samples on device tensors against the host pipeline fed the same radiance
rays = want_plan[2]
radiance = t.radiance(rays["origin"], rays["dir"], rays["seed"], 4, 8)
assert not radiance[total:].view(U32).any()
want = rt.adaptive_merge_host(radiance, want_plan[0], want_plan[1], image, hist, np.inf, host_g["albedo"], moments)
got = t.adaptive_samples(dev_g, up(variance), up(image), up(hist), budget, 4, 8, origin, first_frame=4, moments=up(moments))
assert len(got) == 5 and all(isinstance(v, torch.Tensor) for v in got)
same(got[:3], want, "adaptive_samples on tensors")
same(got[3:], (want_plan[0], want_plan[3]), "adaptive_samples: counts and totals")
print("adaptive_samples on tensors == the host pipeline", flush=True)

# the merge: a NULL colour is the handle's image (the 4 frames rendered above); the image keeps its bits when out is elsewhere
d_rad, d_counts, d_offsets = up(radiance), up(want_plan[0]), up(want_plan[1])
want2 = rt.adaptive_merge_host(radiance, want_plan[0], want_plan[1], image, hist, 6.0)
same(t.adaptive_merge(d_rad, d_counts, d_offsets, None, up(hist), 6.0), want2, "NULL colour")
assert np.array_equal(raw(t.read_image(W, H)), raw(image)), "the image changed"
# the outputs aliasing the inputs
c, h_, m_ = up(image), up(hist), up(moments)
got = t.adaptive_merge(d_rad, d_counts, d_offsets, c, h_, np.inf, dev_g["albedo"], m_, out=c, out_history=h_, out_moments=m_)
assert got[0] is c and got[1] is h_ and got[2] is m_
same(got, want, "the outputs are the inputs")
# ... and the image in place
d = A.AdaptiveMergeDesc(struct_bytes=C.sizeof(A.AdaptiveMergeDesc), width=W, height=H, budget=budget, max_history=6.0)
h2 = up(hist)
d.radiance, d.counts, d.offsets, d.history = d_rad.data_ptr(), d_counts.data_ptr(), d_offsets.data_ptr(), h2.data_ptr()
d.out, d.out_history = t.device_image_ptr, h2.data_ptr()
torch.cuda.synchronize()
t._check(t._L.rt_adaptive_merge(t._h, C.byref(d), 0))
assert np.array_equal(raw(t.read_image(W, H)), raw(want2[0])), "the image in place"
same((h2,), (want2[1],), "the history in place")
print("merge on tensors ok", flush=True)

# the least alignment the contract allows: 4 bytes for variance, dir, counts, offsets, totals and history, 16 for the rest;
# nothing is written outside the outputs
def skewed(planes, aligned16):
    bufs, ptrs, skew = {}, {}, {}
    for k, v in planes.items():
        skew[k] = 16 if k in aligned16 else 4
        bufs[k] = torch.zeros(v.nbytes + 64, dtype=torch.uint8, device=dev)
        assert bufs[k].data_ptr() % 32 == 0
        bufs[k][skew[k]:skew[k] + v.nbytes] = torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).ravel().copy()).to(dev)
        ptrs[k] = bufs[k].data_ptr() + skew[k]
    return bufs, ptrs, skew


def check_skewed(bufs, skew, planes, outs, wants, what):
    for k, w in zip(outs, wants):
        got = bufs[k].cpu().numpy()
        n, s = planes[k].nbytes, skew[k]
        assert np.array_equal(got[s:s + n], raw(w)), (what, k)
        assert not got[:s].any() and not got[s + n:].any(), (what, k, "bytes outside the plane")
    for k in planes:
        if k not in outs:
            assert np.array_equal(bufs[k].cpu().numpy()[skew[k]:skew[k] + planes[k].nbytes], raw(planes[k])), (what, k, "an input changed")


planes = dict(variance=variance, dir=host_g["dir"], counts=np.zeros((H, W), U32), offsets=np.zeros((H, W), U32),
              rays=np.zeros((budget, 8), U32), totals=np.zeros(4, U32))
bufs, ptrs, skew = skewed(planes, ("rays",))
d = A.AdaptivePlanDesc(struct_bytes=C.sizeof(A.AdaptivePlanDesc), width=W, height=H, budget=budget, min_samples=1, max_samples=16,
                       first_frame=4, origin=(C.c_float * 3)(*origin.tolist()))
for k, v in ptrs.items():
    setattr(d, k, v)
torch.cuda.synchronize()
t._check(t._L.rt_adaptive_plan(t._h, C.byref(d), 0))
t.synchronize()
check_skewed(bufs, skew, planes, ("counts", "offsets", "rays", "totals"), want_plan, "plan at the least alignment")
planes = dict(radiance=radiance, counts=want_plan[0], offsets=want_plan[1], color=image, history=hist, albedo=host_g["albedo"],
              moments=moments, out=np.zeros_like(image), out_history=np.zeros_like(hist), out_moments=np.zeros_like(moments))
bufs, ptrs, skew = skewed(planes, ("radiance", "color", "albedo", "moments", "out", "out_moments"))
d = A.AdaptiveMergeDesc(struct_bytes=C.sizeof(A.AdaptiveMergeDesc), width=W, height=H, budget=budget, max_history=float("inf"))
for k, v in ptrs.items():
    setattr(d, k, v)
torch.cuda.synchronize()
t._check(t._L.rt_adaptive_merge(t._h, C.byref(d), 0))
t.synchronize()
check_skewed(bufs, skew, planes, ("out", "out_history", "out_moments"), want, "merge at the least alignment")
print("planes at their least alignment ok", flush=True)

# a handle that already holds more than option max_device_mb allows (the denoiser's scratch, once the cap is lowered under
# it): rt_adaptive_plan on device memory is refused, though its own scratch is there, and nothing is written;
# rt_adaptive_merge allocates nothing and is done all the same
og_host, og_dev, big_image = OC.frame(t)
rng = np.random.default_rng(5)
big_var, big_hist = rng.random((OC.H, OC.W), F32), rng.integers(1, 7, (OC.H, OC.W)).astype(F32)
big_budget = 4 * OC.W * OC.H
big_plan = rt.adaptive_plan_host(big_var, og_host["dir"], origin, big_budget, 1, 16, 4)
big_rad = rng.random((big_budget, 4), F32)
big_want = rt.adaptive_merge_host(big_rad, big_plan[0], big_plan[1], big_image, big_hist, 6.0)
d_var, d_color = up(big_var), up(big_image)
plan_outs = (torch.empty((OC.H, OC.W), dtype=torch.int32, device=dev), torch.empty((OC.H, OC.W), dtype=torch.int32, device=dev),
             torch.empty((big_budget, 8), dtype=torch.float32, device=dev), torch.empty(4, dtype=torch.int32, device=dev))
d = A.AdaptivePlanDesc(struct_bytes=C.sizeof(A.AdaptivePlanDesc), width=OC.W, height=OC.H, budget=big_budget, min_samples=1,
                       max_samples=16, first_frame=4, origin=(C.c_float * 3)(*origin.tolist()))
d.variance, d.dir = d_var.data_ptr(), og_dev["dir"].data_ptr()
d.counts, d.offsets, d.rays, d.totals = (o.data_ptr() for o in plan_outs)
torch.cuda.synchronize()
plan_call = lambda: t._check(t._L.rt_adaptive_plan(t._h, C.byref(d), 0))  # noqa: E731
plan_call()
OC.hold_denoise_scratch(t, og_dev, d_color)
OC.over_cap(t, plan_call, plan_outs, big_plan, True, "rt_adaptive_plan")
merge_outs = (torch.empty((OC.H, OC.W, 4), dtype=torch.float32, device=dev), torch.empty((OC.H, OC.W), dtype=torch.float32, device=dev))
merge_in = (up(big_rad), up(big_plan[0]), up(big_plan[1]), d_color, up(big_hist))
merge_call = lambda: t.adaptive_merge(*merge_in, 6.0, out=merge_outs[0], out_history=merge_outs[1])  # noqa: E731
merge_call()
OC.over_cap(t, merge_call, merge_outs, big_want, False, "rt_adaptive_merge")
t.close()

# The scratch: 32 bytes per 1024 texels and a header of 256.  8192 x 4096 texels make 32768 blocks: 1 MiB and 256 bytes, which
# rt_last_launch out[4] shows and a cap of the same MiB cannot hold.  A zero variance, min_samples = 0 and a budget of 1 keep
# the plan itself trivial: every count is 0 and the one record is the tail.  No scene is needed.
t = rt.RayTracer(0, 16, 16)
BW, BH = 8192, 4096
before = t.last_launch()["device_mb_held"]
big_v = torch.zeros((BH, BW), dtype=torch.float32, device=dev)
big_d = torch.empty((BH, BW, 3), dtype=torch.float32, device=dev)
t.set_option("max_device_mb", max(before, 1))
try:
    t.adaptive_plan(big_v, big_d, origin, 1, 0, 4)
    raise AssertionError("the cap held the scratch")
except rt.RtError as e:
    assert e.code == -8 and "max_device_mb" in str(e), e
assert t.last_launch()["device_mb_held"] == before
t.set_option("max_device_mb", 0)
counts, offsets, rays, totals = t.adaptive_plan(big_v, big_d, origin, 1, 0, 4)
assert not bool(counts.any()) and not bool(offsets.any()) and not bool(rays.view(torch.int32).any()) and totals.tolist() == [0, 0, 0, 0]
held = t.last_launch()["device_mb_held"]
assert before + 1 <= held <= before + 2, (before, held)
small = t.adaptive_plan(up(variance), up(host_g["dir"]), origin, budget, 1, 16, 4)     # a smaller frame reuses the scratch
same(small, want_plan, "a small plan in the large scratch")
assert t.last_launch()["device_mb_held"] == held
t.close()
print("scratch accounting ok", flush=True)
print("device path ok")
