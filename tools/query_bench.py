#!/usr/bin/env python3
"""Rates of the public ray queries (rt_intersect_rays, rt_occluded_rays; device path) in Mrays/s, host clock around a
synchronised window after a warm-up.

    python tools/query_bench.py [--scenes cornell,dragon11] [--rays 8388608] [--reps 5]

Ray sets, built on the device from the scene's camera:
  camera   one primary ray per texel of a 4096 x 2048 view (the debug views' ray, no jitter);
  bounce   cosine-distributed rays about the shading normal at the camera rays' hits (a miss repeats its camera ray);
  shadow   from those hits to uniform points on the ceiling light (the emissive mesh's top face), tmax = 0.999 x the
           distance to the light point.
Queries: closest hit (trace_rays) on every set; occlusion (occluded) on the shadow set, exact and with
RT_QUERY_PRUNE_TMAX; and the closest hit on camera rays once more with one workgroup per 256 rays (option
persistent_blocks set beyond the ray count) instead of the persistent grid.  Prints one JSON line per measurement.
Kernel times come from a separate run under rocprofv3 --kernel-trace --stats."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load(name):
    import ray_tracer_2_amd as rt
    from ray_tracer_2_amd import scenes
    g = os.path.join(ROOT, "tests", "golden")
    if name == "cornell":
        return rt.SceneArrays.load(os.path.join(g, "cornell_scene.npz"))
    n = int(name[6:])   # dragonN: the Cornell dragon with every triangle split N x N (dragon11: x121)
    return rt.SceneArrays.from_scene(scenes.cornell_dragon(scenes.load_raw_meshes(os.path.join(g, "cornell_raw.npz")),
                                                           scenes.load_raw_meshes(os.path.join(g, "dragon_raw.npz")),
                                                           subdivide=n, device=0 if n > 3 else None))


def camera_rays(torch, arrays, n, dev):
    import numpy as np
    cam = arrays.uniform.camera
    c2w = torch.tensor(np.asarray(cam.cam_to_world, np.float32), device=dev)   # [col][row]
    vp = torch.tensor(np.asarray(cam.view_params, np.float32), device=dev)
    W = 4096
    H = (n + W - 1) // W
    i = torch.arange(n, device=dev)
    x, y = (i % W).float(), (i // W).float()
    local = torch.stack([x / (W - 1) - 0.5, y / (H - 1) - 0.5, torch.ones_like(x)], 1) * vp
    focus = local @ c2w[:3, :3] + c2w[3, :3]
    o = c2w[3, :3].expand(n, 3).contiguous()
    return o, focus - o


def light_box(arrays):
    import numpy as np
    for m in arrays.meshes:
        if float(m["material"]["emission_strength"]) > 0:
            t = arrays.triangles[int(m["triangle_offset"]):int(m["triangle_offset"]) + int(m["triangles"])]
            v = np.concatenate([t["v1"], t["v2"], t["v3"]]).astype(np.float64)
            c = np.asarray(m["model_to_world"], np.float64)
            w = v @ c[:3, :3] + c[3, :3]
            return w.min(0), w.max(0)
    raise RuntimeError("no emissive mesh")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell,dragon11")
    ap.add_argument("--rays", type=int, default=8 << 20)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch

    import ray_tracer_2_amd as rt
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(7)
    for name in a.scenes.split(","):
        arrays = load(name)
        tr = rt.RayTracer(0, 64, 64)
        tr.load_scene(arrays)
        n = a.rays
        o, d = camera_rays(torch, arrays, n, dev)
        hits = tr.trace_rays(o, d).view(torch.float32)
        hit = (hits[:, 3].view(torch.int32) & 1) != 0
        p, nrm = hits[:, 4:7], hits[:, 8:11]
        # cosine-distributed about the normal: normal + a uniform unit vector
        u = torch.randn((n, 3), device=dev, generator=g)
        u = u / u.norm(dim=1, keepdim=True)
        bd = torch.where(hit[:, None], nrm + u, d)
        bo = torch.where(hit[:, None], p + nrm * 1e-4, o)
        lo, hi = light_box(arrays)
        r = torch.rand((n, 2), device=dev, generator=g)
        lp = torch.stack([lo[0] + (hi[0] - lo[0]) * r[:, 0], torch.full((n,), hi[1], device=dev), lo[2] + (hi[2] - lo[2]) * r[:, 1]], 1).float()
        sd = lp - bo
        st = (sd.norm(dim=1) * 0.999).contiguous()
        sets = {"camera": (o, d, None), "bounce": (bo.contiguous(), bd.contiguous(), None), "shadow": (bo.contiguous(), sd.contiguous(), st)}

        def rate(fn):
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                fn()
            torch.cuda.synchronize()
            return n * a.reps / (time.perf_counter() - t0) / 1e6

        out = []
        for k, (so, sdir, tm) in sets.items():
            out.append((f"trace_rays/{k}", rate(lambda: tr.trace_rays(so, sdir, tm))))
        so, sdir, tm = sets["shadow"]
        occ = tr.occluded(so, sdir, tm)
        out.append(("occluded/shadow", rate(lambda: tr.occluded(so, sdir, tm))))
        out.append(("occluded+prune/shadow", rate(lambda: tr.occluded(so, sdir, tm, prune=True))))
        diff = int((tr.occluded(so, sdir, tm, prune=True) != occ).sum())
        tr.set_option("persistent_blocks", 1 << 24)
        out.append(("trace_rays/camera/one_block_per_256", rate(lambda: tr.trace_rays(o, d))))
        tr.close()
        for what, mr in out:
            print(json.dumps({"scene": name, "query": what, "rays": n, "mrays_per_s": round(mr, 1)}), flush=True)
        print(json.dumps({"scene": name, "shadow_occluded_fraction": round(float(occ.float().mean()), 4),
                          "camera_hit_fraction": round(float(hit.float().mean()), 4), "prune_tmax_differences": diff}), flush=True)


if __name__ == "__main__":
    main()
