#!/usr/bin/env python3
"""Time of the G-buffer-guided denoiser (rt_denoise, device path) at 1920 x 1080 with all guides: host clock around a
synchronised window of repeated calls, the median of --windows windows after a warm-up, the rows taken in turn inside
every round so that they share whatever else the machine does.

    python tools/denoise_bench.py [--iterations 1,3,5] [--windows 7] [--width 1920 --height 1080]

Rows: one per iteration count n (the prepare kernel and n passes), and `copy`, a device-to-device copy that moves the
bytes one pass moves: a pass reads 48 B and writes 16 B per texel, the copy reads and writes 32 B per texel.  Per row one
JSON line: the median, the smallest and the largest window in ms per call; for the denoiser rows the time per pass and the
bytes per second of the passes beyond the next smaller row (the first row: its passes and the prepare kernel together),
64 B x texels per pass, beside the copy's rate (`of_copy`).  The planes are the Cornell fixture's own frame (8 spp, 4 bounces) and
G-buffer; the result is checked against nothing here (tests/test_gpu_denoise.py does that)."""
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
    ap.add_argument("--iterations", default="1,3,5")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-seconds", type=float, default=0.3)
    a = ap.parse_args()
    import torch

    import ray_tracer_2_amd as rt
    from ray_tracer_2_amd import _abi as A
    if not torch.cuda.is_available():
        sys.exit("denoise_bench needs the GPU: there is no other path to time")
    dev = torch.device("cuda:0")
    W, H = a.width, a.height
    texels = W * H
    tr = rt.RayTracer(0, W, H)
    tr.load_scene(rt.SceneArrays.load(os.path.join(ROOT, "tests", "golden", "cornell_scene.npz")))
    tr.render(rt.make_params(W, H, 4, 8, skybox=1, frames=0))
    color = torch.from_numpy(tr.read_image(W, H)).to(dev)
    g = tr.render_gbuffer(rt.make_params(W, H, 1, 1), ("normal", "point", "albedo", "emission"), device=True)
    out = torch.empty_like(color)
    cur = torch.cuda.current_stream(dev)
    ext = torch.cuda.ExternalStream(tr.stream_ptr, device=dev)

    def call(n):
        d = A.DenoiseDesc(struct_bytes=C.sizeof(A.DenoiseDesc), width=W, height=H, iterations=n, sigma_color=rt.ray_tracer.DENOISE_SIGMA_COLOR,
                          sigma_normal=rt.ray_tracer.DENOISE_SIGMA_NORMAL, sigma_point=rt.ray_tracer.DENOISE_SIGMA_POINT,
                          color=color.data_ptr(), out=out.data_ptr(), **{k: v.data_ptr() for k, v in g.items()})

        def f():   # what RayTracer.denoise does around the library call, on planes allocated beforehand
            ext.wait_stream(cur)
            tr._check(tr._L.rt_denoise(tr._h, C.byref(d), 0))
            cur.wait_stream(ext)
        return f

    src = torch.empty(texels * 32, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    rows = {f"n={n}": call(n) for n in (int(v) for v in a.iterations.split(","))}
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
    pass_bytes = 64 * texels
    copy_rate = pass_bytes / (med["copy"] * 1e-3)
    ns = sorted(int(k[2:]) for k in rows if k != "copy")
    for k, v in ms.items():
        line = {"row": k, "width": W, "height": H, "ms_median": round(med[k], 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                "windows": len(v), "calls_per_window": reps[k]}
        if k == "copy":
            line["gb_per_s"] = round(copy_rate / 1e9, 1)
        else:
            n = int(k[2:])
            smaller = [m for m in ns if m < n]
            if smaller:   # the passes beyond the next smaller row
                m = smaller[-1]
                dt, passes = med[k] - med[f"n={m}"], n - m
                line["passes"] = f"{m + 1}..{n}"
            else:         # the prepare kernel and the row's passes together
                dt, passes = med[k], n
                line["passes"] = f"prepare, 1..{n}"
            rate = passes * pass_bytes / (dt * 1e-3)
            line["ms_per_pass"] = round(dt / passes, 4)
            line["gb_per_s"] = round(rate / 1e9, 1)
            line["of_copy"] = round(rate / copy_rate, 3)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
