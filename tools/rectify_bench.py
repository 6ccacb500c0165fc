#!/usr/bin/env python3
"""Time of history rectification (rt_temporal_rectify, device path) and what it buys on the Cornell fixture.

    python tools/rectify_bench.py [--windows 7] [--window-seconds 0.3] [--moments both|off|on] [--skip-quality] [--skip-timing]

TIMING.  At 1920 x 1080 and 3840 x 2160, for radius 1, 2 and 3, with the object plane, without and with the moments: host
clock around a synchronised window of repeated calls, the median of --windows windows after a warm-up, the rows taken in
turn inside every round so that they share whatever else the machine does.  The planes are noise (uniform colours, history
lengths 1 .. 8, an object plane of vertical bands 64 texels wide): the kernel's work does not depend on their content -- what
a tap adds and whether a texel is clipped are selects, not branches.  Beside each size, `copy`: a device-to-device copy that
moves the bytes the call must move -- color, history, history_length and object read once (40 B per texel), out and
out_history written once (20 B), so the copy reads and writes 30 B per texel; with the moments 32 B more are read and 16 B
written (`copy+moments`: 54 B each way).  `16x16` is what a call costs before it moves anything.  Per row one JSON line: the
median, the smallest and the largest window in ms per call, the bytes per second, and for the calls the fraction of the
copy's rate (`of_copy`).  The kernels' own times come from separate runs under rocprofv3 --kernel-trace
(--windows 2 --window-seconds 0.05 --skip-quality, once with --moments off and once with --moments on: the two use the same
kernels on the same grids).

QUALITY.  The table of tests/test_rectify_host.py::test_a_dimmed_lamp_stops_lagging_and_a_still_scene_loses_nothing from
frames the device rendered: 67 x 45, 8 spp, 4 bounces, the camera still, 24 frames, frame k the raw sample of seed k;
temporal_reproject then temporal_rectify with the defaults in every frame from k = 1 against plain temporal_accumulate; mean
squared rgb error against a 256-frame accumulation of the final scene over the hit texels that are not the lamp.  Nothing is
asserted here (the tests do that)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BYTES = 16 + 16 + 4 + 4 + 16 + 4          # color, history, history_length, object; out, out_history
BYTES_MOMENTS = BYTES + 16 + 16 + 16      # moments, history_moments; out_moments


def timing(a, torch, rt, A):
    dev = torch.device("cuda:0")
    tr = rt.RayTracer(0, 16, 16)
    cur = torch.cuda.current_stream(dev)
    ext = torch.cuda.ExternalStream(tr.stream_ptr, device=dev)
    rows, moved = {}, {}
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    keep = []

    def call_of(d):
        def f():   # what RayTracer.temporal_rectify does around the library call, on planes allocated beforehand
            ext.wait_stream(cur)
            tr._check(tr._L.rt_temporal_rectify(tr._h, C.byref(d), 0))
            cur.wait_stream(ext)
        return f

    for W, H in ((1920, 1080), (3840, 2160)):
        texels = W * H
        f4 = lambda: torch.rand((H, W, 4), generator=gen, device=dev)   # noqa: E731
        p = dict(color=f4(), history=f4(), history_length=torch.randint(1, 9, (H, W), generator=gen, device=dev).float(),
                 object=(torch.arange(W, device=dev, dtype=torch.int32) // 64).repeat(H, 1).contiguous(), moments=f4(),
                 history_moments=f4(), out=f4(), out_history=torch.empty((H, W), device=dev), out_moments=f4())
        keep.append(p)
        for radius in (1, 2, 3):
            for with_moments in {"both": (False, True), "off": (False,), "on": (True,)}[a.moments]:
                d = A.RectifyDesc(struct_bytes=C.sizeof(A.RectifyDesc), width=W, height=H, radius=radius, clip_sigma=1.0, clip_history=4.0,
                                  **{k: v.data_ptr() for k, v in p.items() if with_moments or "moments" not in k})
                keep.append(d)
                name = f"{W}x{H} radius {radius}" + (" +moments" if with_moments else "")
                rows[name] = call_of(d)
                moved[name] = (BYTES_MOMENTS if with_moments else BYTES) * texels, f"{W}x{H} copy" + ("+moments" if with_moments else "")
        for per, name in ((BYTES, f"{W}x{H} copy"), (BYTES_MOMENTS, f"{W}x{H} copy+moments")):
            src = torch.empty(texels * per // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            rows[name] = lambda dst=dst, src=src: dst.copy_(src)
            moved[name] = per * texels, None
    tiny = {k: torch.zeros(16 * 16 * 4, dtype=torch.float32, device=dev) for k in A.RECTIFY_PLANES if k != "out_clipped"}
    tiny["history_length"] += 2
    d16 = A.RectifyDesc(struct_bytes=C.sizeof(A.RectifyDesc), width=16, height=16, radius=3, clip_sigma=1.0, clip_history=4.0,
                        **{k: v.data_ptr() for k, v in tiny.items()})
    rows["16x16 (the call's overhead)"] = call_of(d16)

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
    print(json.dumps({"bytes_per_texel": BYTES, "bytes_per_texel_with_moments": BYTES_MOMENTS}), flush=True)
    for k, v in ms.items():
        line = {"row": k, "ms_median": round(med[k], 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "windows": len(v),
                "calls_per_window": reps[k]}
        if k in moved:
            line["gb_per_s"] = round(moved[k][0] / (med[k] * 1e-3) / 1e9, 1)
            if moved[k][1]:
                line["of_copy"] = round(med[moved[k][1]] / med[k], 3)
        print(json.dumps(line), flush=True)


def quality(rt, np):
    W, H, N, CHANGE, BRIGHT, DIM = 67, 45, 24, 16, 34.0, 8.5
    arrays = rt.SceneArrays.load(os.path.join(ROOT, "tests", "golden", "cornell_scene.npz"))
    lamp = int(np.flatnonzero(arrays.meshes["material"]["emission_strength"] > 0)[0])
    tr = rt.RayTracer(0, W, H)

    def with_lamp(s):
        meshes = arrays.meshes.copy()
        meshes["material"]["emission_strength"][lamp] = s
        return rt.SceneArrays(arrays.uniform, arrays.spheres, meshes, arrays.triangles, arrays.nodes, arrays.textures)

    raw, truth = {}, {}
    for s in (BRIGHT, DIM):
        tr.load_scene(with_lamp(s))
        raw[s] = []
        for k in range(N):
            tr.render(rt.make_params(W, H, 4, 8, skybox=1, frames=-k if k else 0))
            raw[s].append(tr.read_image(W, H).copy())
        for f in range(256):
            tr.render(rt.make_params(W, H, 4, 8, skybox=1, frames=f))
        truth[s] = tr.read_image(W, H).copy()
    g = tr.render_gbuffer(rt.make_params(W, H, 1, 1), ("point", "normal", "object"))
    mask = (g["normal"] != 0).any(-1) & (g["object"] != lamp)
    cam = arrays.uniform.camera
    mse = lambda img, t: float(((img[..., :3].astype(np.float64) - t[..., :3].astype(np.float64))[mask] ** 2).mean())   # noqa: E731
    for name, first, then in (("dimmed", BRIGHT, DIM), ("still", BRIGHT, BRIGHT), ("brightened", DIM, BRIGHT)):
        frames = raw[first][:CHANGE] + raw[then][CHANGE:]
        plain, pn = frames[0].copy(), np.ones((H, W), np.float32)
        rect, rn = plain.copy(), pn.copy()
        for k in range(1, N):
            plain, pn = tr.temporal_accumulate(g, g, cam, plain, pn, frames[k])
            h, hn = tr.temporal_reproject(g, g, cam, rect, rn)
            rect, rn, clip = tr.temporal_rectify(frames[k], h, hn, object=g["object"], clipped=True)
            if k in (16, 19, 23):
                p, r = mse(plain, truth[then]), mse(rect, truth[then])
                print(json.dumps({"sequence": name, "frame": k, "plain": round(p, 5), "rectified": round(r, 5), "ratio": round(r / p, 3),
                                  "single_frame": round(mse(frames[k], truth[then]), 5),
                                  "clipped_share": round(float((clip[mask] == 2).mean()), 3)}), flush=True)
    tr.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-seconds", type=float, default=0.3)
    ap.add_argument("--moments", choices=("both", "off", "on"), default="both",
                    help="the rows timed: without the moments, with them, or both (a kernel trace tells the two apart only by run)")
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--skip-timing", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch

    import ray_tracer_2_amd as rt
    from ray_tracer_2_amd import _abi as A
    if not torch.cuda.is_available():
        sys.exit("rectify_bench needs the GPU: there is no other path to time")
    if not a.skip_timing:
        timing(a, torch, rt, A)
    if not a.skip_quality:
        quality(rt, np)


if __name__ == "__main__":
    main()
