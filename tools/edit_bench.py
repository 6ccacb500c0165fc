#!/usr/bin/env python3
"""Cost of a scene edit: rt_upload_scene (update_buffers, the whole blob) against rt_update_instances (update_instances,
the head only), per call on the host clock and from the call to the first finished frame after it.

    python tools/edit_bench.py [--scenes cornell,sponza340,dragon11] [--reps 15] [--edits color,split]

Edits, applied alternately forth and back so that every call changes the scene:
  color   one mesh's material colour (the head keeps its size: written in place);
  split   one mesh moved out of its run of shared transforms (on the many-mesh stand-in the head changes size: a new
          blob, the tail copied on the device; a few-mesh scene may keep the size).
Scenes: cornell (the Cornell box, blob in LDS), sponza340 (sponza_standin(340, detail=8): 340 meshes, 261 k triangles),
dragonN (the Cornell dragon with every triangle split N x N; dragon11: x121, 1.05 M triangles).  The frame after each call
is a small one (320 x 180, 1 sample, 2 bounces), so that the call dominates; `frame_ms` is that frame alone.  Prints one
JSON line per (scene, edit, call) with medians in ms."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def load(name):
    import ray_tracer_2_amd as rt
    from ray_tracer_2_amd import scenes
    g = os.path.join(ROOT, "tests", "golden")
    if name == "cornell":
        return rt.SceneArrays.load(os.path.join(g, "cornell_scene.npz"))
    if name == "sponza340":
        return rt.SceneArrays.from_scene(scenes.sponza_standin(340, detail=8))
    n = int(name[6:])
    return rt.SceneArrays.from_scene(scenes.cornell_dragon(scenes.load_raw_meshes(os.path.join(g, "cornell_raw.npz")),
                                                           scenes.load_raw_meshes(os.path.join(g, "dragon_raw.npz")),
                                                           subdivide=n, device=0 if n > 3 else None))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="cornell,sponza340,dragon11")
    ap.add_argument("--edits", default="color,split")
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    import ray_tracer_2_amd as rt
    from test_gpu_scene_edits import edit_pair
    W, H = 320, 180
    p = rt.make_params(W, H, 2, 1, skybox=1, frames=0)
    for name in args.scenes.split(","):
        arrays = load(name)
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
        for edit in args.edits.split(","):
            a, b = edit_pair(rt, arrays, edit)
            for call in ("upload_scene", "update_instances"):
                fn = t.update_buffers if call == "upload_scene" else t.update_instances
                t.update_buffers(a)
                t.synchronize()
                host, first = [], []
                for r in range(args.reps):
                    target = b if r % 2 == 0 else a
                    t0 = time.perf_counter()
                    fn(target)
                    t1 = time.perf_counter()
                    t.render(p)
                    t.synchronize()
                    t2 = time.perf_counter()
                    host.append(t1 - t0)
                    first.append(t2 - t0)
                print(json.dumps({"scene": name, "edit": edit, "call": call, "triangles": int(len(arrays.triangles)),
                                  "meshes": int(len(arrays.meshes)), "reps": args.reps,
                                  "host_ms": round(1e3 * statistics.median(host), 3),
                                  "to_first_frame_ms": round(1e3 * statistics.median(first), 3),
                                  "frame_ms": round(1e3 * statistics.median(frame), 3)}), flush=True)
        t.close()


if __name__ == "__main__":
    main()
