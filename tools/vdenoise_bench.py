#!/usr/bin/env python3
"""Time of the variance-guided denoiser (rt_denoise_variance, device path) at 1920 x 1080 with all guides, beside rt_denoise
at the same iteration counts in the same run: host clock around a synchronised window of repeated calls, the median of
--windows windows after a warm-up, the rows taken in turn inside every round so that they share whatever else the machine
does.

    python tools/vdenoise_bench.py [--iterations 1,3,5] [--windows 7] [--width 1920 --height 1080]

Rows, per iteration count n:
    temporal n   rt_denoise_variance with moments and a history of 8 everywhere: every variance from the moments (prepare,
                 the window kernel's vote, n passes)
    spatial n    rt_denoise_variance without moments: every variance from the 7 x 7 window (prepare, window, n passes)
    denoise n    rt_denoise (prepare, n passes)
and `moments` (rt_luminance_moments) and `copy`, a device-to-device copy that moves the bytes one pass moves: a pass reads
48 B and writes 16 B per texel, the copy reads and writes 32 B per texel.  Per row one JSON line: the median, the smallest
and the largest window in ms per call; for the filter rows the time per pass and the bytes per second of the passes beyond
the next smaller row of the same kind (the first row: its passes and the kernels before them together), 64 B x texels per
pass, beside the copy's rate (`of_copy`).  The bytes per texel of the other kernels are in `bytes_per_texel` of the first
rows.  The planes are the Cornell fixture's own frames (8 spp, 4 bounces) and G-buffer; the moments are those of two frames
blended.  The result is checked against nothing here (tests/test_gpu_vdenoise.py does that)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# bytes per texel outside the passes, all planes given: prepare reads colour, normal, point, albedo, emission (72) -- and
# moments, history (20) -- and writes the guide record and (c_0, var_0) (48); the window kernel reads those 48 and writes 4
# (with moments everywhere: it reads 4); rt_denoise's prepare: 72 + 48; rt_luminance_moments: 72 + 16
EXTRA_BYTES = {"temporal": 72 + 20 + 48 + 4, "spatial": 72 + 48 + 48 + 4, "denoise": 72 + 48, "moments": 72 + 16}


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
    from ray_tracer_2_amd import ray_tracer as RT
    if not torch.cuda.is_available():
        sys.exit("vdenoise_bench needs the GPU: there is no other path to time")
    dev = torch.device("cuda:0")
    W, H = a.width, a.height
    texels = W * H
    tr = rt.RayTracer(0, W, H)
    tr.load_scene(rt.SceneArrays.load(os.path.join(ROOT, "tests", "golden", "cornell_scene.npz")))
    g = tr.render_gbuffer(rt.make_params(W, H, 1, 1), ("normal", "point", "albedo", "emission"), device=True)
    tr.render(rt.make_params(W, H, 4, 8, skybox=1, frames=-1))
    other = torch.from_numpy(tr.read_image(W, H)).to(dev)
    tr.render(rt.make_params(W, H, 4, 8, skybox=1, frames=0))
    color = torch.from_numpy(tr.read_image(W, H)).to(dev)
    moments = (0.5 * tr.luminance_moments(g, color) + 0.5 * tr.luminance_moments(g, other)).contiguous()
    history = torch.full((H, W), 8.0, dtype=torch.float32, device=dev)
    out = torch.empty_like(color)
    out_variance = torch.empty((H, W), dtype=torch.float32, device=dev)
    cur = torch.cuda.current_stream(dev)
    ext = torch.cuda.ExternalStream(tr.stream_ptr, device=dev)
    planes = {k: v.data_ptr() for k, v in g.items()}

    def on_stream(fn, d):   # what the RayTracer methods do around the library call, on planes allocated beforehand
        def f():
            ext.wait_stream(cur)
            tr._check(fn(tr._h, C.byref(d), 0))
            cur.wait_stream(ext)
        return f

    def variance(n, with_moments):
        d = A.VDenoiseDesc(struct_bytes=C.sizeof(A.VDenoiseDesc), width=W, height=H, iterations=n, sigma_luminance=RT.VDENOISE_SIGMA_LUMINANCE,
                           sigma_normal=RT.DENOISE_SIGMA_NORMAL, sigma_point=RT.DENOISE_SIGMA_POINT, min_history=RT.VDENOISE_MIN_HISTORY,
                           color=color.data_ptr(), out=out.data_ptr(), out_variance=out_variance.data_ptr(), **planes)
        if with_moments:
            d.moments, d.history = moments.data_ptr(), history.data_ptr()
        return on_stream(tr._L.rt_denoise_variance, d)

    def fixed(n):
        d = A.DenoiseDesc(struct_bytes=C.sizeof(A.DenoiseDesc), width=W, height=H, iterations=n, sigma_color=RT.DENOISE_SIGMA_COLOR,
                          sigma_normal=RT.DENOISE_SIGMA_NORMAL, sigma_point=RT.DENOISE_SIGMA_POINT, color=color.data_ptr(),
                          out=out.data_ptr(), **planes)
        return on_stream(tr._L.rt_denoise, d)

    ns = sorted(int(v) for v in a.iterations.split(","))
    rows = {}
    for n in ns:   # (the kinds in turn at every n: the rows to compare stand next to each other in every round)
        rows[f"temporal n={n}"] = variance(n, True)
        rows[f"spatial n={n}"] = variance(n, False)
        rows[f"denoise n={n}"] = fixed(n)
    rows["moments"] = on_stream(tr._L.rt_luminance_moments, A.VDenoiseDesc(struct_bytes=C.sizeof(A.VDenoiseDesc), width=W, height=H,
                                                                          color=color.data_ptr(), out=out.data_ptr(), **planes))
    src = torch.empty(texels * 32, dtype=torch.uint8, device=dev)
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
    pass_bytes = 64 * texels
    copy_rate = pass_bytes / (med["copy"] * 1e-3)
    for k, v in ms.items():
        line = {"row": k, "width": W, "height": H, "ms_median": round(med[k], 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                "windows": len(v), "calls_per_window": reps[k]}
        if k == "copy":
            line["gb_per_s"] = round(copy_rate / 1e9, 1)
        elif k == "moments":
            line["bytes_per_texel"] = EXTRA_BYTES[k]
            line["gb_per_s"] = round(EXTRA_BYTES[k] * texels / (med[k] * 1e-3) / 1e9, 1)
        else:
            kind, n = k.split(" n=")
            n = int(n)
            smaller = [m for m in ns if m < n]
            if smaller:   # the passes beyond the next smaller row of the same kind
                m = smaller[-1]
                dt, passes = med[k] - med[f"{kind} n={m}"], n - m
                line["passes"] = f"{m + 1}..{n}"
            else:         # the kernels before the passes and the row's passes together
                dt, passes = med[k], n
                line["passes"] = f"prepare, 1..{n}"
                line["bytes_per_texel"] = EXTRA_BYTES[kind] + 64 * n
            rate = passes * pass_bytes / (dt * 1e-3)
            line["ms_per_pass"] = round(dt / passes, 4)
            line["gb_per_s"] = round(rate / 1e9, 1)
            line["of_copy"] = round(rate / copy_rate, 3)
            line["of_denoise"] = round(med[k] / med[f"denoise n={n}"], 3)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
