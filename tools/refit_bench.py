#!/usr/bin/env python3
"""Cost of moving vertices: rt_refit_triangles (refit_triangles: triangle records rewritten and the BVH refitted on the
device) from host memory and from a torch tensor on the device, against rt_upload_scene of the same arrays
(update_buffers: the whole blob from the host, nodes refitted on the host first) and against a host rebuild plus upload
(Scene.build + load_built_scene), per call on the host clock and from the call to the first finished frame after it.

    python tools/refit_bench.py [--scenes cornell,sponza340,dragon11] [--reps 15] [--calls host,device,upload,rebuild]

Two vertex sets are sent alternately, so that every call changes the geometry, for one mesh (the biggest) and for all
meshes.  Scenes as tools/edit_bench.py: cornell (32 triangles), sponza340 (340 meshes, 261 k triangles), dragonN (the
Cornell dragon with every triangle split N x N; dragon11: x121, 1.05 M triangles).  The frame after each call is 320 x 180,
1 sample, 2 bounces; `frame_ms` is that frame alone.  Prints one JSON line per (scene, meshes, call) with medians in ms.
Kernel times: run it under rocprofv3 --kernel-trace --stats with --calls device."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def load(name):
    import ray_tracer_2_amd as rt
    from ray_tracer_2_amd import scenes
    g = os.path.join(ROOT, "tests", "golden")
    if name == "cornell":
        return rt.Scene.from_name("cornell_box", os.path.join(g, "assets")), None
    if name == "sponza340":
        return scenes.sponza_standin(340, detail=8), None
    n = int(name[6:])
    return scenes.cornell_dragon(scenes.load_raw_meshes(os.path.join(g, "cornell_raw.npz")),
                                 scenes.load_raw_meshes(os.path.join(g, "dragon_raw.npz")), subdivide=n,
                                 device=0 if n > 3 else None), (0 if n > 3 else None)


def moved(tris, seed):
    rng = np.random.RandomState(seed)
    t = tris.copy()
    pts = np.concatenate([t["v1"], t["v2"], t["v3"]])
    ext = np.float32(np.max(pts.max(0) - pts.min(0)))
    for k in ("v1", "v2", "v3"):
        t[k] = (t[k] + rng.normal(0, 0.002, t[k].shape).astype(np.float32) * ext).astype(np.float32)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell,sponza340,dragon11")
    ap.add_argument("--calls", default="host,device,upload,rebuild")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--rebuild-reps", type=int, default=3)
    args = ap.parse_args()
    import torch

    import ray_tracer_2_amd as rt
    W, H = 320, 180
    p = rt.make_params(W, H, 2, 1, skybox=1, frames=0)
    calls = args.calls.split(",")
    for name in args.scenes.split(","):
        sc, device = load(name)
        arrays = rt.SceneArrays.from_scene(sc)
        t = rt.RayTracer(device=0, max_width=W, max_height=H)
        t.load_scene(arrays)
        t.render(p)
        t.synchronize()
        frame = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            t.render(p)
            t.synchronize()
            frame.append(time.perf_counter() - t0)
        big = int(np.argmax(arrays.meshes["triangles"]))
        for which, (i0, i1) in (("one", (big, big + 1)), ("all", (0, len(arrays.meshes)))):
            m = arrays.meshes[i0:i1]
            first = int(m["triangle_offset"].min())
            n = int((m["triangle_offset"] + m["triangles"]).max()) - first
            sets = [moved(arrays.triangles[first:first + n], s) for s in (1, 2)]
            dev = [torch.from_numpy(np.ascontiguousarray(s).view(np.float32).reshape(n, 24)).to("cuda:0") for s in sets]
            fulls = [rt.SceneArrays(arrays.uniform, arrays.spheres, arrays.meshes, arrays.triangles.copy(), arrays.nodes.copy(),
                                    arrays.textures).refit_bvh(first, n, s) for s in sets]
            torch.cuda.synchronize()
            for call in calls:
                reps = args.rebuild_reps if call == "rebuild" else args.reps
                t.load_scene(arrays)
                t.synchronize()
                host, to_frame = [], []
                for r in range(reps):
                    k = r % 2
                    t0 = time.perf_counter()
                    if call == "host":
                        t.refit_triangles(sets[k], first)
                    elif call == "device":
                        t.refit_triangles(dev[k], first)
                    elif call == "upload":
                        t.update_buffers(fulls[k])
                    else:   # a host rebuild (every mesh, as rt_scene_build does; the cost does not depend on the vertices) + upload
                        sc.build(1, device=device)
                        t.load_built_scene(sc)
                    t1 = time.perf_counter()
                    t.render(p)
                    t.synchronize()
                    t2 = time.perf_counter()
                    host.append(t1 - t0)
                    to_frame.append(t2 - t0)
                print(json.dumps({"scene": name, "meshes": which, "call": call, "triangles_sent": n,
                                  "triangles": int(len(arrays.triangles)), "reps": reps,
                                  "host_ms": round(1e3 * statistics.median(host), 3),
                                  "to_first_frame_ms": round(1e3 * statistics.median(to_frame), 3),
                                  "frame_ms": round(1e3 * statistics.median(frame), 3)}), flush=True)
        t.close()


if __name__ == "__main__":
    main()
