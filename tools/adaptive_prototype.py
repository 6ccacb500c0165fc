"""The float64 prototype behind DESIGN.md section 2.16's quality table: is a ray budget apportioned in proportion to the
standard deviation better spent than the same budget spread evenly?  CPU only (the oracle renders every frame).

Cornell 67x45, 8 spp, 4 bounces.  For each of three pilot seeds s: a pilot of 4 accumulated frames (seeds s .. s + 3), the
variance from denoise_variance_host's out_variance, then 4 more ray records per texel on average, either n(p) in proportion
to sqrt(variance) (min 1, max 16, the rule of rt_adaptive_plan restated here in float64 and Python integers) or 4 everywhere;
sample k of a texel is the raw frame of seed s + 4 + k; the merge is a float64 running mean.  Mean squared error against the
256-frame accumulation over the filterable texels.

    python tools/adaptive_prototype.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ray_tracer_2_amd as rt  # noqa: E402
from ray_tracer_2_amd.build import build_oracle  # noqa: E402

W, H, PILOT, EXTRA, MIN, MAX = 67, 45, 4, 4, 1, 16


def apportion(variance, budget, mn, mx):
    v = variance.astype(np.float64).ravel()
    ok = np.isfinite(v) & (v > 0)
    q = np.zeros(v.size, np.int64)
    if ok.any():
        q[ok] = np.floor(np.sqrt(v[ok] / v[ok].max()) * 2.0 ** 20).astype(np.int64)
    S, R = int(q.sum()), budget - mn * v.size
    n, c = np.full(v.size, mn, np.int64), 0
    for p in range(v.size):
        if S:
            n[p] += ((c + int(q[p])) * R) // S - (c * R) // S
        c += int(q[p])
    return np.minimum(n, mx)


def main():
    build_oracle()
    from oracle import oracle
    import _denoise_reference as DR
    import _vdenoise_reference as VR
    oracle.load()
    arrays = rt.SceneArrays.load(os.path.join(ROOT, "tests", "golden", "cornell_scene.npz"))
    case = DR.cornell_case(rt, oracle, arrays)
    g = {k: case[k] for k in ("normal", "point", "albedo", "emission")}
    ok = DR.classify(case["color"], case["normal"], case["point"], case["emission"])
    truth = case["converged"][..., :3].astype(np.float64)

    def mse(img):
        d = img[..., :3][ok] - truth[ok]
        return float((d * d).mean())

    def raw(seed):
        return oracle.render(rt.make_params(W, H, 4, 8, skybox=1, frames=-seed if seed else 0), arrays)[0].copy()

    rows = []
    for s in (0, 20, 40):
        pilot = [raw(s + k) for k in range(PILOT)]
        cam = arrays.uniform.camera
        color, hist = VR.accumulate(rt, g, cam, pilot)
        moments, _ = VR.accumulate(rt, g, cam, [rt.luminance_moments_host(g, r) for r in pilot])
        _, variance = rt.denoise_variance_host(g, color, moments=moments, history=hist, out_variance=True)
        extra = [raw(s + PILOT + k).astype(np.float64) for k in range(MAX)]
        out = {}
        for name, n in (("adaptive", apportion(variance, EXTRA * W * H, MIN, MAX)), ("uniform", np.full(W * H, EXTRA, np.int64))):
            acc = color.astype(np.float64).reshape(-1, 4).copy()
            for k in range(int(n.max())):
                sel = n > k
                acc[sel] += (extra[k].reshape(-1, 4)[sel] - acc[sel]) / (PILOT + k + 1)
            out[name] = (mse(acc.reshape(H, W, 4)), int(n.sum()))
        rows.append((s, mse(color.astype(np.float64)), out["uniform"], out["adaptive"]))
        print(f"pilot seed {s:2d}: pilot {rows[-1][1]:.6f}  uniform {out['uniform'][0]:.6f} ({out['uniform'][1]} rays)  "
              f"adaptive {out['adaptive'][0]:.6f} ({out['adaptive'][1]} rays)  adaptive / uniform {out['adaptive'][0] / out['uniform'][0]:.3f}")
    u = np.array([r[2][0] for r in rows])
    a = np.array([r[3][0] for r in rows])
    print(f"uniform - adaptive: {(u - a).tolist()}; least margin {float((u - a).min()):.6f}; "
          f"spread over the seeds (max - min): uniform {float(u.max() - u.min()):.6f}, adaptive {float(a.max() - a.min()):.6f}")


if __name__ == "__main__":
    main()
