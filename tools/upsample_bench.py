#!/usr/bin/env python3
"""Time of guided upsampling (rt_upsample, device path) on the Cornell fixture, and of the pipeline it is for: host clock
around a synchronised window of repeated calls, the median of --windows windows after a warm-up, the rows taken in turn
inside every round so that they share whatever else the machine does.

    python tools/upsample_bench.py [--windows 5] [--window-seconds 0.3] [--skip-pipeline]

Kernel rows, per pair of sizes (960x540 -> 1920x1080, 1920x1080 -> 3840x2160, and 1280x720 -> 1920x1080 for a ratio of
1.5): `all planes` (albedo on both sides, emission, coverage) and `required planes`; beside each a `copy` row, a
device-to-device copy that moves the bytes the call must move -- every input plane read once, every output written once, so
the copy reads and writes half of them each.  Per row one JSON line: the median, the smallest and the largest window in ms
per call, the bytes moved, the bytes per second and the fraction of the copy's rate (`of_copy`); the call's rows also give
the shares of `coverage`.
Pipeline rows, the bench line's workload (Cornell, 4 bounces, one frame per launch, seed 0) three ways in alternation:
`full 1920x1080 8 spp` (rt_render alone); `low 960x540 32 spp + upsample` and `low 960x540 8 spp + upsample` -- rt_render
at the low size, rt_render_gbuffer at the low size (point, normal, object, albedo) and at the high one (depth, point, normal,
object, albedo, emission), then rt_upsample from the handle's image with every plane.  ms per frame.
Nothing is checked against anything here (tests/test_gpu_upsample.py does that)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LO_CHANNELS = ("point", "normal", "object", "albedo")
HI_CHANNELS = ("depth", "point", "normal", "object", "albedo", "emission")
PAIRS = ((960, 540, 1920, 1080), (1920, 1080, 3840, 2160), (1280, 720, 1920, 1080))


def bytes_moved(w, h, W, H, optional):
    """Every input plane once and every output once."""
    lo = 16 + 12 + 12 + 4 + (16 if optional else 0)
    hi = 4 + 12 + 12 + 4 + (32 if optional else 0) + 16 + (1 if optional else 0)
    return w * h * lo + W * H * hi


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


def gbuffer_desc(A, torch, dev, W, H, channels):
    """A filled rt_gbuffer over new device planes, and the planes by name."""
    kinds = {"<f4": torch.float32, "<u4": torch.int32, "u1": torch.uint8}
    g, planes = A.GBuffer(struct_bytes=C.sizeof(A.GBuffer)), {}
    for c in channels:
        dt, k = A.GBUFFER_CHANNELS[c]
        planes[c] = torch.empty((H, W, k) if k else (H, W), dtype=kinds[dt], device=dev)
        setattr(g, c, planes[c].data_ptr())
    return g, planes


def upsample_desc(A, rt, w, h, W, H, lo, hi, color, out, coverage, optional):
    d = A.UpsampleDesc(struct_bytes=C.sizeof(A.UpsampleDesc), lo_width=w, lo_height=h, width=W, height=H,
                       point_tolerance=rt.ray_tracer.UPSAMPLE_POINT_TOLERANCE, normal_cos=rt.ray_tracer.UPSAMPLE_NORMAL_COS,
                       lo_color=color.data_ptr() if color is not None else None, out=out.data_ptr())
    for k in ("point", "normal", "object") + (("albedo",) if optional else ()):
        setattr(d, "lo_" + k, lo[k].data_ptr())
    for k in ("depth", "point", "normal", "object") + (("albedo", "emission") if optional else ()):
        setattr(d, k, hi[k].data_ptr())
    if optional:
        d.coverage = coverage.data_ptr()
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-seconds", type=float, default=0.3)
    ap.add_argument("--skip-pipeline", action="store_true")
    a = ap.parse_args()
    import torch

    import ray_tracer_2_amd as rt
    from ray_tracer_2_amd import _abi as A
    if not torch.cuda.is_available():
        sys.exit("upsample_bench needs the GPU: there is no other path to time")
    dev = torch.device("cuda:0")
    arrays = rt.SceneArrays.load(os.path.join(ROOT, "tests", "golden", "cornell_scene.npz"))
    tr = rt.RayTracer(0, 3840, 2160)
    tr.load_scene(arrays)
    cur = torch.cuda.current_stream(dev)
    ext = torch.cuda.ExternalStream(tr.stream_ptr, device=dev)

    def on_stream(call):   # what RayTracer.upsample does around the library call, on planes allocated beforehand
        ext.wait_stream(cur)
        call()
        cur.wait_stream(ext)

    rows, notes, moved = {}, {}, {}
    keep = []
    for w, h, W, H in PAIRS:
        tr.render(rt.make_params(w, h, 4, 8, skybox=1, frames=0))
        color = torch.from_numpy(tr.read_image(w, h)).to(dev)
        lo = tr.render_gbuffer(rt.make_params(w, h, 1, 1), LO_CHANNELS, device=True)
        hi = tr.render_gbuffer(rt.make_params(W, H, 1, 1), HI_CHANNELS, device=True)
        out = torch.empty((H, W, 4), device=dev)
        coverage = torch.empty((H, W), dtype=torch.uint8, device=dev)
        for optional, name in ((True, "all planes"), (False, "required planes")):
            d = upsample_desc(A, rt, w, h, W, H, lo, hi, color, out, coverage, optional)
            row = f"{w}x{h} -> {W}x{H}, {name}"
            rows[row] = lambda d=d: on_stream(lambda: tr._check(tr._L.rt_upsample(tr._h, C.byref(d), 0)))
            moved[row] = bytes_moved(w, h, W, H, optional)
            rows[row]()
            torch.cuda.synchronize()
            if optional:
                cov = coverage.cpu().numpy()
                notes[row] = {"ring1": round(float((cov == 2).mean()), 5), "ring2": round(float((cov == 1).mean()), 5),
                              "holes": round(float((cov == 0).mean()), 5)}
            src = torch.empty(moved[row] // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            rows[row + " (copy)"] = lambda src=src, dst=dst: dst.copy_(src)
            moved[row + " (copy)"] = moved[row]
        keep.append((color, lo, hi, out, coverage))
    res = measure(torch, rows, a.windows, a.window_seconds)
    med = {k: statistics.median(v) for k, (v, _) in res.items()}
    for k, (v, reps) in res.items():
        line = {"row": k, "ms_median": round(med[k], 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "windows": len(v),
                "calls_per_window": reps, "bytes_moved": moved[k], "gb_per_s": round(moved[k] / (med[k] * 1e-3) / 1e9, 1)}
        if not k.endswith("(copy)"):
            line["of_copy"] = round(med[k + " (copy)"] / med[k], 3)
            line.update(notes.get(k, {}))
        print(json.dumps(line), flush=True)
    del rows, keep
    if a.skip_pipeline:
        tr.close()
        return

    # the pipeline: one frame per iteration, every call queued on the handle's stream without a synchronisation between them
    w, h, W, H = 960, 540, 1920, 1080
    lo_g, lo = gbuffer_desc(A, torch, dev, w, h, LO_CHANNELS)
    hi_g, hi = gbuffer_desc(A, torch, dev, W, H, HI_CHANNELS)
    out = torch.empty((H, W, 4), device=dev)
    coverage = torch.empty((H, W), dtype=torch.uint8, device=dev)
    d = upsample_desc(A, rt, w, h, W, H, lo, hi, None, out, coverage, True)   # (lo_color NULL: the image rt_render left)
    lo_p1, hi_p1 = rt.make_params(w, h, 1, 1), rt.make_params(W, H, 1, 1)

    def full():
        tr.render(rt.make_params(W, H, 4, 8, skybox=1, frames=0))

    def low(spp):
        def run():
            tr.render(rt.make_params(w, h, 4, spp, skybox=1, frames=0))
            tr._check(tr._L.rt_render_gbuffer(tr._h, C.byref(lo_p1), C.byref(lo_g), 0))
            tr._check(tr._L.rt_render_gbuffer(tr._h, C.byref(hi_p1), C.byref(hi_g), 0))
            tr._check(tr._L.rt_upsample(tr._h, C.byref(d), 0))
        return lambda: on_stream(run)

    # ... and the low pipeline's calls one at a time, each in windows of its own
    rows = {"full 1920x1080 8 spp": full, "low 960x540 32 spp + upsample": low(32), "low 960x540 8 spp + upsample": low(8),
            "  part: rt_render 960x540 32 spp": lambda: tr.render(rt.make_params(w, h, 4, 32, skybox=1, frames=0)),
            "  part: rt_render 960x540 8 spp": lambda: tr.render(rt.make_params(w, h, 4, 8, skybox=1, frames=0)),
            "  part: rt_render_gbuffer 960x540": lambda: tr._check(tr._L.rt_render_gbuffer(tr._h, C.byref(lo_p1), C.byref(lo_g), 0)),
            "  part: rt_render_gbuffer 1920x1080": lambda: tr._check(tr._L.rt_render_gbuffer(tr._h, C.byref(hi_p1), C.byref(hi_g), 0)),
            "  part: rt_upsample": lambda: on_stream(lambda: tr._check(tr._L.rt_upsample(tr._h, C.byref(d), 0)))}
    # (rt_render is asynchronous on the handle's stream, which a window's torch.cuda.synchronize covers with the device)
    res = measure(torch, rows, a.windows, a.window_seconds)
    med = {k: statistics.median(v) for k, (v, _) in res.items()}
    for k, (v, reps) in res.items():
        line = {"row": k, "ms_per_frame_median": round(med[k], 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                "windows": len(v), "frames_per_window": reps}
        if k.startswith("low"):
            line["of_full"] = round(med[k] / med["full 1920x1080 8 spp"], 3)
        print(json.dumps(line), flush=True)
    cov = coverage.cpu().numpy()
    print(json.dumps({"pipeline_coverage": {"ring1": round(float((cov == 2).mean()), 5), "ring2": round(float((cov == 1).mean()), 5),
                                            "holes": round(float((cov == 0).mean()), 5)}}), flush=True)
    tr.close()


if __name__ == "__main__":
    main()
