#!/usr/bin/env python3
"""Time of adaptive sampling's three steps (device path) at 1920 x 1080 on the Cornell fixture: rt_adaptive_plan,
rt_radiance_rays over the planned list and rt_adaptive_merge, each beside the same ray total allocated uniformly, in one run.
tools/vdenoise_bench.py's method: host clock around a synchronised window of repeated calls, the median of --windows windows
after a warm-up, the rows taken in turn inside every round so that they share whatever else the machine does.

    python tools/adaptive_bench.py [--per-texel 4] [--windows 7] [--width 1920 --height 1080] [--bounces 4 --samples 1]

The variance is rt_denoise_variance's out_variance of a pilot of 4 accumulated frames (8 spp, 4 bounces); the budget is
--per-texel rays per texel; `adaptive` plans it with min 1, max 16, `uniform` with min = max = --per-texel.  Rows, one JSON
line each (median, smallest and largest window in ms per call):
    plan adaptive / plan uniform        the six kernels of the plan
    trace adaptive / trace uniform      rt_radiance_rays over all `budget` records (the tail past the plan's total included)
    merge adaptive / merge uniform      with moments and albedo
    copy plan / copy merge              a device-to-device copy that moves the bytes the step moves: the plan reads the
                                        variance three times and the directions once per record at most and writes counts
                                        (read again), offsets and 32 B per record -- 24 B x texels + 44 B x records, counting
                                        one direction per record --; the merge reads 16 B per record and 60 B per texel and
                                        writes 36 B per texel.  A copy of n bytes reads n and writes n: n is half of that.
Nothing is checked here (tests/test_gpu_adaptive.py does that)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--per-texel", type=int, default=4)
    ap.add_argument("--bounces", type=int, default=4)
    ap.add_argument("--samples", type=int, default=1)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-seconds", type=float, default=0.3)
    a = ap.parse_args()
    import numpy as np
    import torch

    import ray_tracer_2_amd as rt
    from ray_tracer_2_amd import _abi as A
    if not torch.cuda.is_available():
        sys.exit("adaptive_bench needs the GPU: there is no other path to time")
    dev = torch.device("cuda:0")
    W, H = a.width, a.height
    texels, budget = W * H, a.per_texel * W * H
    tr = rt.RayTracer(0, W, H)
    scene = rt.SceneArrays.load(os.path.join(ROOT, "tests", "golden", "cornell_scene.npz"))
    tr.load_scene(scene)
    origin = np.asarray(scene.uniform.camera.cam_to_world, np.float32)[3, :3].copy()
    g = tr.render_gbuffer(rt.make_params(W, H, 1, 1), ("dir", "normal", "point", "albedo", "emission"), device=True)
    for f in range(4):
        tr.render(rt.make_params(W, H, 4, 8, skybox=1, frames=f))
    color = torch.from_numpy(tr.read_image(W, H)).to(dev)
    history = torch.full((H, W), 4.0, dtype=torch.float32, device=dev)
    moments = tr.luminance_moments(g, color)
    _, variance = tr.denoise_variance(g, color, out_variance=True)
    out, out_history, out_moments = torch.empty_like(color), torch.empty_like(history), torch.empty_like(moments)
    cur = torch.cuda.current_stream(dev)
    ext = torch.cuda.ExternalStream(tr.stream_ptr, device=dev)
    params = rt.make_params(0, 0, a.bounces, a.samples, skybox=1)

    def on_stream(call):   # what the RayTracer methods do around the library call, on planes allocated beforehand
        def f():
            ext.wait_stream(cur)
            tr._check(call())
            cur.wait_stream(ext)
        return f

    rows, facts = {}, {}
    for kind, (mn, mx) in (("adaptive", (1, 16)), ("uniform", (a.per_texel, a.per_texel))):
        counts, offsets, rays, totals = tr.adaptive_plan(variance, g["dir"], origin, budget, mn, mx, 4)
        radiance = torch.empty((budget, 4), dtype=torch.float32, device=dev)
        facts[kind] = [int(v) for v in totals.cpu().tolist()]
        pd = A.AdaptivePlanDesc(struct_bytes=C.sizeof(A.AdaptivePlanDesc), width=W, height=H, budget=budget, min_samples=mn, max_samples=mx,
                                first_frame=4, origin=(C.c_float * 3)(*origin.tolist()), variance=variance.data_ptr(), dir=g["dir"].data_ptr(),
                                counts=counts.data_ptr(), offsets=offsets.data_ptr(), rays=rays.data_ptr(), totals=totals.data_ptr())
        md = A.AdaptiveMergeDesc(struct_bytes=C.sizeof(A.AdaptiveMergeDesc), width=W, height=H, budget=budget, max_history=float("inf"),
                                 radiance=radiance.data_ptr(), counts=counts.data_ptr(), offsets=offsets.data_ptr(), color=color.data_ptr(),
                                 history=history.data_ptr(), albedo=g["albedo"].data_ptr(), moments=moments.data_ptr(), out=out.data_ptr(),
                                 out_history=out_history.data_ptr(), out_moments=out_moments.data_ptr())
        rows[f"plan {kind}"] = on_stream(lambda pd=pd: tr._L.rt_adaptive_plan(tr._h, C.byref(pd), 0))
        rows[f"trace {kind}"] = on_stream(lambda rays=rays, radiance=radiance: tr._L.rt_radiance_rays(tr._h, C.byref(params), rays.data_ptr(), budget,
                                                                                                      radiance.data_ptr(), 0))
        rows[f"merge {kind}"] = on_stream(lambda md=md: tr._L.rt_adaptive_merge(tr._h, C.byref(md), 0))
        rows[f"trace {kind}"]()   # (the merge rows read this radiance)
    moved = {"plan": 24 * texels + 44 * budget, "merge": 16 * budget + 96 * texels}
    for k, n in moved.items():
        src = torch.empty(n // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        rows[f"copy {k}"] = lambda src=src, dst=dst: dst.copy_(src)

    def window(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3

    reps = {}
    for k, fn in rows.items():   # warm-up, and as many calls per window as fill window_seconds
        window(fn, 2)
        reps[k] = max(3, int(a.window_seconds * 1e3 / max(window(fn, 3), 1e-3)) + 1) if a.windows > 1 else 3
    ms = {k: [] for k in rows}
    for _ in range(a.windows):
        for k, fn in rows.items():
            ms[k].append(window(fn, reps[k]))
    tr.close()
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k, v in ms.items():
        step, kind = k.split(" ")
        line = {"row": k, "width": W, "height": H, "budget": budget, "ms_median": round(med[k], 4), "ms_min": round(min(v), 4),
                "ms_max": round(max(v), 4), "windows": len(v), "calls_per_window": reps[k]}
        if step == "copy":
            line["bytes_moved"] = moved[kind]
            line["gb_per_s"] = round(moved[kind] / (med[k] * 1e-3) / 1e9, 1)
        else:
            line["rays_planned"], line["texels_above_min"], line["texels_clamped"] = facts[kind][:3]
            if step in moved:
                line["gb_per_s"] = round(moved[step] / (med[k] * 1e-3) / 1e9, 1)
                line["of_copy"] = round(med[f"copy {step}"] / med[k], 3)
            else:
                line["bounces"], line["samples"] = a.bounces, a.samples
                line["mrays_per_s"] = round(facts[kind][0] / (med[k] * 1e-3) / 1e6, 1)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
