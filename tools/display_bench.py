#!/usr/bin/env python3
"""Time of the display pass (rt_display), the exposure meter (rt_auto_exposure) and the shown frame they are for, on the
device path: host clock around a synchronised window of repeated calls, the median of --windows windows after a warm-up, the
rows taken in turn inside every round so that they share whatever else the machine does.

    python tools/display_bench.py [--windows 5] [--window-seconds 0.3] [--skip-shown] [--out profiles/display_bench.txt]

Kernel rows, at 1920x1080 and 3840x2160 on a rendered Cornell frame (8 spp, tiled up to the size):
`display <tone> <transfer>` for each tone and transfer (layout 0), `display clamp srgb bgra top-first` (the flip), and beside
them `copy 20 B/texel`, a device-to-device copy that moves the bytes the pass must move -- 16 read and 4 written per texel, so
the copy reads and writes 10 each; `auto_exposure rendered` and `auto_exposure one bin` (every texel in one bin: the worst
case of the LDS atomics) beside `copy 16 B/texel`.  Per row one JSON line: the median, the smallest and the largest window
in ms per call, the bytes moved, the bytes per second and the copy's time over the row's (`of_copy`: 1 = as fast as the copy).
A row is a call as RayTracer.display makes it: ordered behind the current torch stream and that stream behind it, two event
hand-offs a call.  The `(queued)` rows are the same calls queued back to back on the handle's stream with no hand-off, as a
C host issues them: the kernels' own rate.  The copies run on the torch stream, back to back, and at these sizes inside the
256 MB last-level cache.
Shown-frame rows, bench.py's own loop (Cornell 1920x1080, 4 bounces, 8 spp, one launch per frame, 48 frames a
repetition), three ways in alternation in one process: `render only` (no read), `float snapshot pair` (rt_snapshot_image +
rt_read_snapshot under the next frame: 33 MB a frame) and `display snapshot pair` (rt_snapshot_display +
rt_read_display_snapshot: 8.3 MB).  ms per shown frame, PCIe included.
Nothing is checked against anything here (tests/test_gpu_display.py does that)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZES = ((1920, 1080), (3840, 2160))
BENCH_W, BENCH_H, BENCH_SPP, BENCH_BOUNCES, N_SHOWN = 1920, 1080, 8, 4, 48
QUEUED = " (queued)"


def window(torch, fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def measure(torch, rows, windows, window_seconds):
    """rows: name -> callable.  Returns name -> (list of ms per call, one per window; calls per window)."""
    reps = {}
    for k, fn in rows.items():   # warm-up, and as many calls per window as fill window_seconds
        window(torch, fn, 2)
        reps[k] = max(3, int(window_seconds * 1e3 / max(window(torch, fn, 3), 1e-3)) + 1)
    ms = {k: [] for k in rows}
    for _ in range(windows):
        for k, fn in rows.items():
            ms[k].append(window(torch, fn, reps[k]))
    return {k: (v, reps[k]) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-seconds", type=float, default=0.3)
    ap.add_argument("--skip-shown", action="store_true")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    import torch

    import _display_reference as R
    import ray_tracer_2_amd as rt
    from ray_tracer_2_amd import _abi as A
    if not torch.cuda.is_available():
        sys.exit("display_bench needs the GPU: there is no other path to time")
    dev = torch.device("cuda:0")
    lines = []

    def emit(line):
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)

    arrays = rt.SceneArrays.load(os.path.join(ROOT, "tests", "golden", "cornell_scene.npz"))
    tr = rt.RayTracer(0, 1920, 1080)
    tr.load_scene(arrays)
    cur = torch.cuda.current_stream(dev)
    ext = torch.cuda.ExternalStream(tr.stream_ptr, device=dev)

    def on_stream(call):   # what RayTracer.display does around the library call, on planes allocated beforehand
        ext.wait_stream(cur)
        call()
        cur.wait_stream(ext)

    tr.render(rt.make_params(BENCH_W, BENCH_H, BENCH_BOUNCES, BENCH_SPP, skybox=1, frames=0))
    frame = tr.read_image(BENCH_W, BENCH_H)
    rows, moved, yard, keep = {}, {}, {}, []
    for W, H in SIZES:
        rendered = torch.from_numpy(np.ascontiguousarray(np.tile(frame, (H // BENCH_H, W // BENCH_W, 1)))).to(dev)
        one_bin = torch.from_numpy(np.ascontiguousarray(np.tile(R.one_bin_frame(240, 135), (H // 135, W // 240, 1)))).to(dev)
        out = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
        scale = torch.ones((1,), device=dev)
        hist = torch.zeros((256,), dtype=torch.int32, device=dev)
        size = f"{W}x{H}"
        copies = {}
        for per_texel in (20, 16):
            src = torch.empty(W * H * per_texel // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            copies[per_texel] = f"{size} copy {per_texel} B/texel"
            rows[copies[per_texel]] = lambda src=src, dst=dst: dst.copy_(src)
            moved[copies[per_texel]] = W * H * per_texel
        settings = [(f"{tone} {transfer}", tone_n, transfer_n, 0) for tone, tone_n in (("clamp", 0), ("reinhard", 1))
                    for transfer, transfer_n in (("srgb", 0), ("linear", 1))] + [("clamp srgb bgra top-first", 0, 0, 3)]
        for name, tone, transfer, layout in settings:
            d = A.DisplayDesc(struct_bytes=C.sizeof(A.DisplayDesc), width=W, height=H, tone=tone, transfer=transfer, layout=layout,
                              exposure=1.0, white=4.0, color=rendered.data_ptr(), exposure_scale=scale.data_ptr(), out=out.data_ptr())
            row = f"{size} display {name}"
            rows[row] = lambda d=d: on_stream(lambda: tr._check(tr._L.rt_display(tr._h, C.byref(d), 0)))
            moved[row], yard[row] = W * H * 20, copies[20]
            if name in ("clamp srgb", "clamp linear"):
                rows[row + QUEUED] = lambda d=d: tr._check(tr._L.rt_display(tr._h, C.byref(d), 0))
                moved[row + QUEUED], yard[row + QUEUED] = W * H * 20, copies[20]
        for name, plane in (("rendered", rendered), ("one bin", one_bin)):
            m = A.AutoExposureDesc(struct_bytes=C.sizeof(A.AutoExposureDesc), width=W, height=H, low_permille=100, high_permille=950, key=0.18,
                                   min_scale=2.0 ** -10, max_scale=2.0 ** 10, rate=1.0, color=plane.data_ptr(), histogram=hist.data_ptr(),
                                   scale=scale.data_ptr())
            row = f"{size} auto_exposure {name}"
            rows[row] = lambda m=m: on_stream(lambda: tr._check(tr._L.rt_auto_exposure(tr._h, C.byref(m), 0)))
            moved[row], yard[row] = W * H * 16, copies[16]
            rows[row + QUEUED] = lambda m=m: tr._check(tr._L.rt_auto_exposure(tr._h, C.byref(m), 0))
            moved[row + QUEUED], yard[row + QUEUED] = W * H * 16, copies[16]
        keep.append((rendered, one_bin, out, scale, hist))
    res = measure(torch, rows, a.windows, a.window_seconds)
    med = {k: statistics.median(v) for k, (v, _) in res.items()}
    for k, (v, reps) in res.items():
        line = {"row": k, "ms_median": round(med[k], 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "windows": len(v),
                "calls_per_window": reps, "bytes_moved": moved[k], "gb_per_s": round(moved[k] / (med[k] * 1e-3) / 1e9, 1)}
        if k in yard:
            line["of_copy"] = round(med[yard[k]] / med[k], 3)
        emit(line)
    del rows, keep
    torch.cuda.empty_cache()

    if not a.skip_shown:
        W, H = BENCH_W, BENCH_H
        host_float, host_bytes = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.uint8)
        d = A.DisplayDesc(struct_bytes=C.sizeof(A.DisplayDesc), width=W, height=H, layout=A.DISPLAY_LAYOUT_BGRA, exposure=1.0, white=1.0)
        L, h = tr._L, tr._h

        def render(f):
            tr.render(rt.make_params(W, H, BENCH_BOUNCES, BENCH_SPP, skybox=1, frames=1 + f))

        def shown(take, read):   # bench.py's loop: frame f renders while frame f - 1 comes to the host
            tr.synchronize()
            t1 = time.perf_counter()
            render(0)
            take()
            for f in range(1, N_SHOWN):
                render(f)
                read()
                take()
            read()
            return (time.perf_counter() - t1) / N_SHOWN * 1e3

        def render_only():
            tr.synchronize()
            t1 = time.perf_counter()
            for f in range(N_SHOWN):
                render(f)
            tr.synchronize()
            return (time.perf_counter() - t1) / N_SHOWN * 1e3

        ways = {
            "render only": render_only,
            "float snapshot pair": lambda: shown(lambda: tr.snapshot_image(W, H),
                                                 lambda: tr._check(L.rt_read_snapshot(h, host_float.ctypes.data, host_float.nbytes))),
            "display snapshot pair": lambda: shown(lambda: tr._check(L.rt_snapshot_display(h, C.byref(d))),
                                                   lambda: tr._check(L.rt_read_display_snapshot(h, host_bytes.ctypes.data, host_bytes.nbytes))),
        }
        ts = {k: [] for k in ways}
        for k, fn in ways.items():
            fn()   # warm-up: buffers, events, the copy stream
        for _ in range(a.windows):
            for k, fn in ways.items():
                ts[k].append(fn())
        for k, v in ts.items():
            emit({"row": f"shown frame {W}x{H}: {k}", "ms_per_frame_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4),
                  "ms_max": round(max(v), 4), "windows": len(v), "frames_per_window": N_SHOWN,
                  "host_bytes_per_frame": {"render only": 0, "float snapshot pair": W * H * 16, "display snapshot pair": W * H * 4}[k]})
    tr.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
