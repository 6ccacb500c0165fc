#!/usr/bin/env python3
"""Times of the radiance query (rt_radiance_rays; device path) in ms and Mpaths/s: device events around each call, after a
warm-up, five windows, medians.  A timed call is RayTracer.radiance on tensors: the wrapper's packing of the ray records (one
torch.cat) is inside the window.  Writes the table to profiles/radiance_bench.txt (--out).

    python tools/radiance_bench.py [--out profiles/radiance_bench.txt] [--windows 5] [--warmup 2]

Workloads, all on the Cornell box of the bench configuration (4 bounces, skybox on):
  (a) camera   the 1920 x 1080 camera rays of the bench frame (8 spp) in texel order -- origin cam_to_world[3], the `dir`
               plane of rt_render_gbuffer, pixel_seeds(1920, 1080, 0) --, beside one lone rt_render of the same frame on
               the same handle (its launches' device time, rt_get_stats); the call's output is compared with that image;
  (b) shuffled the same rays in a seeded random order: incoherent refill;
  (c) probes   4096 probe origins inside the box x 256 seeded directions each, 4 spp."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, SPP, BOUNCES = 1920, 1080, 8, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "radiance_bench.txt"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import numpy as np
    import torch

    import ray_tracer_2_amd as rt
    dev = torch.device("cuda:0")
    arrays = rt.SceneArrays.load(os.path.join(ROOT, "tests", "golden", "cornell_scene.npz"))
    tr = rt.RayTracer(0, W, H)
    tr.load_scene(arrays)
    p = rt.make_params(W, H, BOUNCES, SPP, skybox=1, frames=0)

    def timed(fn):
        """median and spread of `windows` device-event times of fn (ms), after `warmup` untimed calls"""
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(a.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms), max(ms)

    def render_ms():
        """one lone rt_render of the frame: the device time of its launches (the library's own events)"""
        tr.synchronize()
        tr.reset_timing()
        tr.render(p)
        tr.synchronize()
        return float(tr.stats().kernel_ms)

    for _ in range(a.warmup):
        render_ms()
    r = sorted(render_ms() for _ in range(a.windows))
    image = tr.read_image(W, H)

    # (a) the frame's camera rays in texel order
    d = tr.render_gbuffer(p, channels=("dir",), device=True)["dir"].reshape(-1, 3).contiguous()
    n = d.shape[0]
    cam = torch.tensor(np.asarray(arrays.uniform.camera.cam_to_world, np.float32)[3, :3], device=dev)
    o = cam.expand(n, 3).contiguous()
    s = torch.from_numpy(rt.pixel_seeds(W, H, 0).view(np.int32)).to(dev)
    got = tr.radiance(o, d, s, BOUNCES, SPP).cpu().numpy()
    equal = bool(np.array_equal(got.view(np.uint32), image.reshape(-1, 4).view(np.uint32)))
    rows = [("(a) camera rays, texel order", n, SPP, timed(lambda: tr.radiance(o, d, s, BOUNCES, SPP)))]
    # (b) the same rays, shuffled
    perm = torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    ob, db, sb = o[perm].contiguous(), d[perm].contiguous(), s[perm].contiguous()
    rows.append(("(b) camera rays, shuffled", n, SPP, timed(lambda: tr.radiance(ob, db, sb, BOUNCES, SPP))))
    # (c) probes
    g = torch.Generator(device=dev).manual_seed(11)
    pts = np.concatenate([np.concatenate([t["v1"], t["v2"], t["v3"]]) for t in (arrays.triangles,)]).astype(np.float32)
    lo, hi = torch.tensor(pts.min(0), device=dev), torch.tensor(pts.max(0), device=dev)   # (the Cornell meshes sit in world space)
    probes = lo + (hi - lo) * (0.1 + 0.8 * torch.rand((4096, 3), device=dev, generator=g))
    oc = probes.repeat_interleave(256, dim=0).contiguous()
    dc = torch.randn((4096 * 256, 3), device=dev, generator=g)
    dc = (dc / dc.norm(dim=1, keepdim=True)).contiguous()
    sc = torch.arange(4096 * 256, device=dev, dtype=torch.int32)
    rows.append(("(c) 4096 probes x 256 directions", oc.shape[0], 4, timed(lambda: tr.radiance(oc, dc, sc, BOUNCES, 4))))
    tr.close()

    med_r = statistics.median(r)
    lines = [f"radiance_bench: Cornell box, {BOUNCES} bounces, skybox on; device path, device events, {a.warmup} warm-up calls, "
             f"{a.windows} windows, medians (min .. max)",
             f"device: {torch.cuda.get_device_name(0)}",
             "",
             f"{'workload':36s} {'rays':>9s} {'spp':>4s} {'ms':>9s} {'(min .. max)':>20s} {'Mpaths/s':>9s}"]
    for what, nr, spp, (med, lo_, hi_) in rows:
        lines.append(f"{what:36s} {nr:9d} {spp:4d} {med:9.3f} {f'({lo_:.3f} .. {hi_:.3f})':>20s} {nr * spp / med / 1e3:9.1f}")
    lines += [f"{'rt_render of the same frame (alone)':36s} {W * H:9d} {SPP:4d} {med_r:9.3f} {f'({r[0]:.3f} .. {r[-1]:.3f})':>20s} {W * H * SPP / med_r / 1e3:9.1f}",
              "",
              f"(a) / rt_render: {rows[0][3][0] / med_r:.2f}x    (b) / (a): {rows[1][3][0] / rows[0][3][0]:.2f}x",
              f"(a)'s output equals the rendered image bit for bit: {equal}"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(json.dumps({"camera_ms": rows[0][3][0], "shuffled_ms": rows[1][3][0], "probes_ms": rows[2][3][0], "render_ms": med_r,
                      "equals_render": equal}))


if __name__ == "__main__":
    main()
