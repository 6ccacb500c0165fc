#!/usr/bin/env python3
"""Time of temporal accumulation (rt_temporal_accumulate, device path) at 1920 x 1080 on the Cornell fixture with every
plane (object planes and motion included): host clock around a synchronised window of repeated calls, the median of
--windows windows after a warm-up, the rows taken in turn inside every round so that they share whatever else the machine
does.

    python tools/temporal_bench.py [--windows 7] [--width 1920 --height 1080]

Rows: one per camera move -- `unmoved`, `1 texel` and `16 texels` (the camera translated to its right by what shifts the
image by about that much at the scene's mean depth; the row reports the mean |motion| the call itself measured and the share
of hit texels that found history) --, two of the call with a motion table (rt_temporal_accumulate_moving) under the unmoved
camera: `table, all still`, every record with moved == 0, and `table, both boxes moved`, the fixture's two boxes moved by
update_instances between the frames (the row also reports the motion and the history found on the boxes' texels) --, `16x16`, the same call on a frame of 256 misses, which is what a call costs before it
moves anything (the host's part and the launch), and `copy`, a device-to-device copy that moves the bytes the call must move: every
input plane read once (92 B per texel) and every output written once (28 B per texel), so the copy reads and writes 60 B
per texel.  Per row one JSON line: the median, the smallest and the largest window in ms per call, the bytes per second, and
for the calls the fraction of the copy's rate (`of_copy`).  The previous frame is the fixture's camera's (8 spp, 4 bounces),
the current one the moved camera's; the result is checked against nothing here (tests/test_gpu_temporal.py does that)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BYTES_IN, BYTES_OUT = 16 + 12 + 12 + 4 + 16 + 4 + 12 + 12 + 4, 16 + 4 + 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-seconds", type=float, default=0.3)
    a = ap.parse_args()
    import numpy as np
    import torch

    import ray_tracer_2_amd as rt
    from ray_tracer_2_amd import _abi as A
    if not torch.cuda.is_available():
        sys.exit("temporal_bench needs the GPU: there is no other path to time")
    dev = torch.device("cuda:0")
    W, H = a.width, a.height
    texels = W * H
    arrays = rt.SceneArrays.load(os.path.join(ROOT, "tests", "golden", "cornell_scene.npz"))
    base = arrays.uniform.camera
    channels = ("point", "normal", "object")
    tr = rt.RayTracer(0, W, H)
    tr.load_scene(arrays)

    def frame(cam):
        tr.set_camera(cam)
        tr.render(rt.make_params(W, H, 4, 8, skybox=1, frames=0))
        return torch.from_numpy(tr.read_image(W, H)).to(dev), tr.render_gbuffer(rt.make_params(W, H, 1, 1), channels, device=True)

    prev_color, pg = frame(base)
    prev_history = torch.full((H, W), 4.0, device=dev)
    # the mean view depth of the hit texels gives the world size of a texel: pw / (W - 1) per unit of depth
    pt = pg["point"].cpu().numpy()
    hit = (pg["normal"].cpu().numpy() != 0).any(-1)
    m = np.array(base.cam_to_world, np.float64).reshape(4, 4)
    depth = float((((pt - m[3, :3]) @ m[2, :3])[hit]).mean())
    texel = depth * float(base.view_params[0]) / float(base.view_params[2]) / (W - 1)
    out, out_history, motion = torch.empty_like(prev_color), torch.empty_like(prev_history), torch.empty((H, W, 2), device=dev)
    cur = torch.cuda.current_stream(dev)
    ext = torch.cuda.ExternalStream(tr.stream_ptr, device=dev)
    rows, notes = {}, {}
    for name, shift in (("unmoved", 0.0), ("1 texel", 1.0), ("16 texels", 16.0)):
        cam = type(base).from_buffer_copy(bytes(base))
        for k in range(3):
            cam.cam_to_world[3][k] = float(m[3, k] + shift * texel * m[0, k])
        color, g = frame(cam)
        d = A.TemporalDesc(struct_bytes=C.sizeof(A.TemporalDesc), width=W, height=H, prev_camera=type(base).from_buffer_copy(bytes(base)),
                           max_history=float("inf"), point_tolerance=rt.ray_tracer.TEMPORAL_POINT_TOLERANCE,
                           normal_cos=rt.ray_tracer.TEMPORAL_NORMAL_COS, color=color.data_ptr(), prev_color=prev_color.data_ptr(),
                           prev_history=prev_history.data_ptr(), out=out.data_ptr(), out_history=out_history.data_ptr(),
                           motion=motion.data_ptr(), **{k: v.data_ptr() for k, v in g.items()},
                           **{"prev_" + k: v.data_ptr() for k, v in pg.items()})

        def f(d=d, keep=(color, g)):   # what RayTracer.temporal_accumulate does around the library call, on planes allocated beforehand
            ext.wait_stream(cur)
            tr._check(tr._L.rt_temporal_accumulate(tr._h, C.byref(d), 0))
            cur.wait_stream(ext)
        rows[name] = f
        f()
        torch.cuda.synchronize()
        mo, hi = motion.cpu().numpy(), out_history.cpu().numpy()
        now_hit = (g["normal"].cpu().numpy() != 0).any(-1)
        found = now_hit & (hi > 1)
        notes[name] = {"mean_motion_texels": round(float(np.linalg.norm(mo[found], axis=-1).mean()), 3),
                       "history_found": round(float(found.sum() / now_hit.sum()), 4)}
    tr.set_camera(base)

    # the call with a motion table (rt_temporal_accumulate_moving), under the unmoved camera: `table, all still` on the
    # frames of the `unmoved` row with a table of identical states, and `table, both boxes moved` on a current frame
    # rendered after update_instances moved meshes 5 and 6 (0.06 / -0.04 along x, turned 0.05 / -0.08 rad about the
    # vertical axis through their centroids), with the table of object_motions
    def moved_mesh(meshes, k, shift, angle):
        tri = arrays.triangles[int(meshes[k]["triangle_offset"]):int(meshes[k]["triangle_offset"]) + int(meshes[k]["triangles"])]
        m2w = np.array(meshes[k]["model_to_world"], np.float64).T
        v = np.concatenate([tri["v1"], tri["v2"], tri["v3"]]).astype(np.float64)
        pivot = (v @ m2w[:3, :3].T + m2w[:3, 3]).mean(0)
        c, s = np.cos(angle), np.sin(angle)
        T = np.eye(4)
        T[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
        T[:3, 3] = pivot - T[:3, :3] @ pivot + np.array([shift, 0.0, 0.0])
        new = T @ m2w
        meshes["model_to_world"][k], meshes["world_to_model"][k] = new.T, np.linalg.inv(new).T

    meshes = arrays.meshes.copy()
    moved_mesh(meshes, 5, 0.06, 0.05)
    moved_mesh(meshes, 6, -0.04, -0.08)
    moved = rt.SceneArrays(arrays.uniform, arrays.spheres, meshes, arrays.triangles, arrays.nodes, arrays.textures)
    for name, state in (("table, all still", arrays), ("table, both boxes moved", moved)):
        tr.update_instances(state)
        color, g = frame(base)
        table = rt.object_motions(arrays, state)
        dev_table = torch.from_numpy(table.view(np.int32).reshape(-1, 24).copy()).to(dev)
        d = A.TemporalMotionDesc(struct_bytes=C.sizeof(A.TemporalMotionDesc), width=W, height=H, prev_camera=type(base).from_buffer_copy(bytes(base)),
                                 max_history=float("inf"), point_tolerance=rt.ray_tracer.TEMPORAL_POINT_TOLERANCE,
                                 normal_cos=rt.ray_tracer.TEMPORAL_NORMAL_COS, color=color.data_ptr(), prev_color=prev_color.data_ptr(),
                                 prev_history=prev_history.data_ptr(), out=out.data_ptr(), out_history=out_history.data_ptr(),
                                 motion=motion.data_ptr(), motions=dev_table.data_ptr(), n_objects=len(table),
                                 **{k: v.data_ptr() for k, v in g.items()}, **{"prev_" + k: v.data_ptr() for k, v in pg.items()})

        def f(d=d, keep=(color, g, dev_table)):
            ext.wait_stream(cur)
            tr._check(tr._L.rt_temporal_accumulate_moving(tr._h, C.byref(d), 0))
            cur.wait_stream(ext)
        rows[name] = f
        f()
        torch.cuda.synchronize()
        mo, hi, ob = motion.cpu().numpy(), out_history.cpu().numpy(), g["object"].cpu().numpy()
        now_hit = (g["normal"].cpu().numpy() != 0).any(-1)
        found = now_hit & (hi > 1)
        boxes = (ob == 5) | (ob == 6)
        notes[name] = {"mean_motion_texels": round(float(np.linalg.norm(mo[found], axis=-1).mean()), 3),
                       "history_found": round(float(found.sum() / now_hit.sum()), 4),
                       "objects_moved": int(table["moved"].sum()), "texels_of_moved_objects": int((boxes & (table["moved"][5] != 0)).sum()),
                       "mean_motion_on_them": round(float(np.linalg.norm(mo[found & boxes], axis=-1).mean()), 3),
                       "history_found_on_them": round(float((found & boxes).sum() / boxes.sum()), 4)}
    tr.update_instances(arrays)
    # what a call costs before it moves anything: the same call on a 16 x 16 frame of misses
    tiny = {k: torch.zeros(16 * 16 * 4, dtype=torch.float32, device=dev) for k in A.TEMPORAL_PLANES}
    d16 = A.TemporalDesc(struct_bytes=C.sizeof(A.TemporalDesc), width=16, height=16, prev_camera=type(base).from_buffer_copy(bytes(base)),
                         max_history=float("inf"), point_tolerance=rt.ray_tracer.TEMPORAL_POINT_TOLERANCE,
                         normal_cos=rt.ray_tracer.TEMPORAL_NORMAL_COS, **{k: v.data_ptr() for k, v in tiny.items()})

    def call16():
        ext.wait_stream(cur)
        tr._check(tr._L.rt_temporal_accumulate(tr._h, C.byref(d16), 0))
        cur.wait_stream(ext)
    rows["16x16 (the call's overhead)"] = call16
    src = torch.empty(texels * (BYTES_IN + BYTES_OUT) // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    rows["copy"] = lambda: dst.copy_(src)

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
    moved = (BYTES_IN + BYTES_OUT) * texels
    copy_rate = moved / (med["copy"] * 1e-3)
    print(json.dumps({"width": W, "height": H, "bytes_per_texel_read": BYTES_IN, "bytes_per_texel_written": BYTES_OUT,
                      "bytes_per_call": moved, "mean_depth": round(depth, 3), "texel_world_size": round(texel, 6)}), flush=True)
    for k, v in ms.items():
        line = {"row": k, "ms_median": round(med[k], 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "windows": len(v),
                "calls_per_window": reps[k]}
        if k == "copy" or k in notes:
            line["gb_per_s"] = round(moved / (med[k] * 1e-3) / 1e9, 1)
        if k in notes:
            line["of_copy"] = round(moved / (med[k] * 1e-3) / copy_rate, 3)
            line.update(notes[k])
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
