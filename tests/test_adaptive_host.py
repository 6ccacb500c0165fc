"""rt_adaptive_plan_host and rt_adaptive_merge_host (include/rt_abi.h; csrc/host/adaptive.cpp over csrc/rt_adaptive.h) against
the independent numpy restatement of tests/_adaptive_reference.py, bit for bit, on synthetic planes built to meet every rule
of the definition -- asserted from the reference's own account --; the apportionment's properties; mul_div_floor against
unsigned __int128 (tests/cpp/adaptive_mul_div_driver.cpp); the uniform consequence on the oracle; and the quality ordering of
DESIGN.md section 2.16."""
import os
import subprocess

import numpy as np
import pytest

import _adaptive_reference as R
from conftest import ROOT

F32, U32 = np.float32, np.uint32
SIZES, ORIGIN, plan_cases, assert_plan_equal = R.SIZES, R.ORIGIN, R.plan_cases, R.assert_plan_equal


def run_plan(rt, W, H, case):
    name, v, budget, mn, mx, ff = case
    st = {}
    want = R.plan(v, R.dir_plane(W, H), ORIGIN, budget, mn, mx, ff, stats=st)
    got = rt.adaptive_plan_host(v, R.dir_plane(W, H), ORIGIN, budget, mn, mx, ff)
    return want, got, st


@pytest.mark.parametrize("W,H", SIZES)
def test_plan_equals_the_reference(rt, W, H):
    for case in plan_cases(W, H):
        want, got, st = run_plan(rt, W, H, case)
        assert_plan_equal(got, want, (W, H, case[0]))
        counts, offsets, rays, totals = got
        # the apportionment's properties
        assert int(counts.sum()) == int(totals[0]) <= case[2], case[0]
        assert np.array_equal(offsets.ravel(), np.concatenate([[0], np.cumsum(counts.ravel().astype(np.int64))[:-1]]).astype(U32))
        if st["clamped"] == 0 and st["S"] != 0:
            assert int(counts.sum()) == case[2], case[0]        # (before the clamp the e(p) sum to R exactly)
        if st["S"] == 0:
            assert (counts == case[3]).all()
        assert counts.min() >= case[3] and counts.max() <= case[4]
        assert not rays[int(totals[0]):].view(np.uint8).any(), (case[0], "the tail is zeros")


def test_the_planes_meet_every_rule(rt):
    """From the reference's own account, on the 24x16 and 67x45 planes."""
    for W, H in ((24, 16), (67, 45)):
        cases = {c[0]: c for c in plan_cases(W, H)}
        st = {name: run_plan(rt, W, H, c)[2] for name, c in cases.items()}
        d = st["defaults"]
        assert d["zero"] >= 2 and d["negative"] >= 2 and d["nan"] == 1 and d["pos_inf"] == 1 and d["neg_inf"] == 1   # (-0 is a zero)
        assert d["denormal"] == 1 and d["at_max"] >= 2          # the maximum itself, twice
        assert d["S"] > 0 and 0 < d["takes"].mean() < 1
        assert st["all zero"]["S"] == 0 and st["nothing takes part"]["S"] == 0
        assert st["clamped"]["clamped"] >= 0.1 * W * H
        assert st["no clamp"]["clamped"] == 0 and st["defaults"]["clamped"] >= 0
        assert st["R = 0"]["R"] == 0 and st["min 0"]["wanted"].min() == 0      # n(p) = 0 occurs
        assert st["small budget"]["diffused"] > 0.5 * W * H                     # most e(p) are 0: the diffusion decides
        assert 0 < st["small budget"]["R"] == int((st["small budget"]["wanted"] - 1).sum())
        assert st["seed wraps"]["wrapped_seeds"] > 0
        assert st["budget beyond the plan"]["clamped"] > 0


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("albedo,moments", [(True, True), (False, True), (False, False)])
def test_merge_equals_the_reference(rt, W, H, albedo, moments):
    counts, offsets, p, bad = R.merge_inputs(W, H)
    for max_history in (np.inf, 4.0, 1.0):
        st = {}
        kw = dict(albedo=p["albedo"] if albedo else None, moments=p["moments"] if moments else None)
        want = R.merge(p["radiance"], counts, offsets, p["color"], p["history"], max_history, stats=st, **kw)
        got = rt.adaptive_merge_host(p["radiance"], counts, offsets, p["color"], p["history"], max_history, **kw)
        assert len(got) == (3 if moments else 2)
        for g, w, name in zip(got, want, ("out", "out_history", "out_moments")):
            bad_bits = ~R.same_bits(g, w)
            assert not bad_bits.any(), (W, H, max_history, name, np.argwhere(bad_bits)[:4].tolist())
        if (W, H) in ((24, 16), (67, 45)):
            assert st["no_prior"] >= 5 and st["dropped"] >= 5 and st["first"] >= 3 and st["blended"] > W * H
            assert bad["first"] >= 1 and bad["middle"] >= 1 and bad["all"] >= 1
            assert (counts == 0).any() and st["untouched"] >= 1
            if max_history != np.inf:
                assert st["capped"] > 0
    # out aliasing color (and the other outputs their inputs)
    color, hist, mom = p["color"].copy(), p["history"].copy(), p["moments"].copy()
    want = rt.adaptive_merge_host(p["radiance"], counts, offsets, p["color"], p["history"], 6.0, p["albedo"], p["moments"])
    got = rt.adaptive_merge_host(p["radiance"], counts, offsets, color, hist, 6.0, p["albedo"], mom, out=color, out_history=hist, out_moments=mom)
    assert got[0] is color and got[1] is hist and got[2] is mom
    for g, w in zip(got, want):
        assert R.same_bits(g, w).all()


def test_merge_stops_at_the_budget(rt):
    """Counts and offsets that point past the list: no read leaves it (the samples past `budget` are dropped)."""
    W, H = 8, 1
    counts = np.full((H, W), 3, U32)
    offsets = (np.arange(W, dtype=U32) * 3).reshape(H, W)
    rad = np.random.default_rng(2).uniform(0, 1, (20, 4)).astype(F32)     # 24 would be needed
    color, hist = np.zeros((H, W, 4), F32), np.zeros((H, W), F32)
    got = rt.adaptive_merge_host(rad, counts, offsets, color, hist)
    want = R.merge(rad, counts, offsets, color, hist)
    assert R.same_bits(got[0], want[0]).all() and np.array_equal(got[1], [[3, 3, 3, 3, 3, 3, 2, 0]])


def test_mul_div_floor_against_int128(tmp_path):
    exe = tmp_path / "adaptive_mul_div_driver"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall",
                    "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "adaptive_mul_div_driver.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "mul_div_floor ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_uniform_plan_is_the_shaders_accumulation(rt, oracle, cornell):
    """min = max = N = 3, budget = N W H, history 0: merge_host of the oracle's raw frames 0 .. 2 (frames = -k) is
    oracle.render's accumulation after frames 0 .. 2, bit for bit, alpha included."""
    W, H, N = 67, 45, 3
    counts, offsets, rays, totals = rt.adaptive_plan_host(R.variance_plane(W, H), R.dir_plane(W, H), ORIGIN, N * W * H, N, N, 0)
    assert (counts == N).all() and totals[0] == N * W * H and totals[1] == 0
    seeds = rays["seed"].reshape(H * W, N)
    assert np.array_equal(seeds[:, 1], rt.pixel_seeds(W, H, 1)) and np.array_equal(seeds[:, 2], rt.pixel_seeds(W, H, 2))
    acc = None
    radiance = np.zeros((N * W * H, 4), F32)
    for k in range(N):
        acc, _ = oracle.render(rt.make_params(W, H, 4, 8, skybox=1, frames=k), cornell, image=acc)
        raw, _ = oracle.render(rt.make_params(W, H, 4, 8, skybox=1, frames=-k), cornell)
        radiance[offsets.ravel() + k] = raw.reshape(-1, 4)
    out, hist = rt.adaptive_merge_host(radiance, counts, offsets, np.zeros((H, W, 4), F32), np.zeros((H, W), F32))
    assert R.same_bits(out, acc).all() and (hist == N).all()


def _mse(img, truth, ok):
    d = img[..., :3].astype(np.float64)[ok] - truth[ok]
    return float((d * d).mean())


def test_adaptive_allocation_beats_the_uniform_one(rt, oracle, cornell):
    """Cornell 67x45, 8 spp, 4 bounces: a pilot of 4 accumulated frames, the variance from denoise_variance_host's
    out_variance, 4 more ray records per texel on average (min 1, max 16) taken from the oracle's raw frames, merged; beside
    the uniform allocation of the same budget (4 per texel).  Mean squared error against the 256-frame accumulation over the
    filterable texels: adaptive <= uniform.  The float64 prototype (tools/adaptive_prototype.py) gave,
    over three pilot seeds, uniform 0.0281 / 0.0298 / 0.0266 against adaptive 0.0174 / 0.0176 / 0.0170: a least margin of
    0.0096 beside a spread over the seeds of 0.0032, so the ordering is asserted.  Measured here (binary32, pilot seed 0):
    pilot 0.059067, uniform 0.028053, adaptive 0.017354 with 10111 of the 12060 rays (121 texels clamped at 16)."""
    import _denoise_reference as DR
    import _vdenoise_reference as VR
    W, H = 67, 45
    case = DR.cornell_case(rt, oracle, cornell)
    g = {k: case[k] for k in ("normal", "point", "albedo", "emission")}
    ok = DR.classify(case["color"], case["normal"], case["point"], case["emission"])
    truth = case["converged"][..., :3].astype(np.float64)
    color, moments, hist = VR.cornell_history(rt, oracle, cornell, case, 4)
    _, variance = rt.denoise_variance_host(g, color, moments=moments, history=hist, out_variance=True)
    raws = [oracle.render(rt.make_params(W, H, 4, 8, skybox=1, frames=-(4 + k)), cornell)[0].reshape(-1, 4).copy() for k in range(16)]
    T = W * H
    res = {}
    for name, (mn, mx) in (("adaptive", (1, 16)), ("uniform", (4, 4))):
        counts, offsets, _, totals = rt.adaptive_plan_host(variance, R.dir_plane(W, H), ORIGIN, 4 * T, mn, mx, 4)
        radiance = np.zeros((4 * T, 4), F32)
        for k in range(int(counts.max())):
            sel = counts.ravel() > k
            radiance[offsets.ravel()[sel] + k] = raws[k][sel]
        out, h2 = rt.adaptive_merge_host(radiance, counts, offsets, color, hist)
        assert np.array_equal(h2, hist + counts)
        res[name] = (_mse(out, truth, ok), int(totals[0]), int(totals[2]))
    pilot = _mse(color, truth, ok)
    print(f"mean squared error over the filterable texels: pilot of 4 frames {pilot:.6f}, +4 per texel uniform {res['uniform'][0]:.6f}, "
          f"adaptive {res['adaptive'][0]:.6f} (rays {res['adaptive'][1]} of {4 * T}, clamped texels {res['adaptive'][2]})")
    assert res["uniform"][1] == 4 * T and res["adaptive"][1] <= 4 * T
    assert res["uniform"][0] < pilot and res["adaptive"][0] <= res["uniform"][0]
