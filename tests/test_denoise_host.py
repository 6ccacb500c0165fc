"""rt_denoise_host (include/rt_abi.h; csrc/host/denoise.cpp over csrc/rt_denoise.h) against the independent numpy restatement
of the definition (tests/_denoise_reference.py), bit for bit; then what the filter is for -- it brings a noisy Cornell
frame closer to the converged one -- and conditions on the reference alone that keep the comparison from passing
vacuously.  No device."""
import itertools

import numpy as np
import pytest

import _denoise_reference as R

F32 = np.float32
SIGMAS = (4.0, 0.3, 1.0)   # sigma_color, sigma_normal, sigma_point of the issue's quality condition


def _guides(case, albedo, emission):
    g = {"normal": case["normal"], "point": case["point"]}
    if albedo:
        g["albedo"] = case["albedo"]
    if emission:
        g["emission"] = case["emission"]
    return g


def _check(rt, oracle, case, n, albedo, emission, sigmas=SIGMAS, what=""):
    want = R.reference(oracle, case["color"], case["normal"], case["point"], case["albedo"] if albedo else None,
                       case["emission"] if emission else None, n, *sigmas)
    got = rt.denoise_host(_guides(case, albedo, emission), case["color"], n, *sigmas)
    bad = ~R.same_bits(got, want)
    assert not bad.any(), (what, n, albedo, emission, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    return got


@pytest.fixture(scope="module")
def cornell_frame(rt, oracle, cornell):
    return R.cornell_case(rt, oracle, cornell)


def test_synthetic_frame_meets_every_rule(oracle):
    """The 24x16 frame holds what it was built to hold (so the sweep below exercises each rule)."""
    c = R.synthetic_case()
    ok = R.classify(c["color"], c["normal"], c["point"], c["emission"])
    assert 0.5 < ok.mean() < 0.95
    assert not ok[6:8].any() and not ok[10:13, 3:6].any() and not ok[3, 20] and not ok[2, 8]
    assert ok[13, 9] and np.isnan(c["color"][13, 9, 3])   # (a NaN alpha does not make a texel unfilterable)
    assert ok[2, 15] and ok[3, 16] and ok[12, 20] and (c["albedo"][ok][:, :3] < 2.0 ** -10).sum() >= 6
    assert R.classify(c["color"], c["normal"], c["point"], None)[10:13, 3:6].all()
    n = c["normal"]
    assert ok[5, 11] and ok[5, 12] and not np.array_equal(n[5, 11], n[5, 12])   # the crease


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("albedo,emission", list(itertools.product((True, False), repeat=2)))
def test_synthetic_frame_equals_the_reference(rt, oracle, n, albedo, emission):
    """(a): iterations 1 .. 5 (step 16 on 24x16 puts most taps outside the frame), each optional plane present and absent."""
    case = R.synthetic_case()
    got = _check(rt, oracle, case, n, albedo, emission, what="synthetic")
    ok = R.classify(case["color"], case["normal"], case["point"], case["emission"] if emission else None)
    assert R.same_bits(got[~ok], case["color"][~ok]).all()          # copied through, NaN and infinity included
    assert R.same_bits(got[..., 3], case["color"][..., 3]).all()    # alpha carried
    assert (~R.same_bits(got[ok][:, :3], case["color"][ok][:, :3])).mean() > 0.9


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("albedo,emission", list(itertools.product((True, False), repeat=2)))
def test_cornell_frame_equals_the_reference(rt, oracle, cornell_frame, n, albedo, emission):
    """(b): the Cornell fixture at 67x45, albedo all ones or NULL, emission from the winning triangle's material or NULL."""
    _check(rt, oracle, cornell_frame, n, albedo, emission, what="cornell")


def test_out_may_be_color(rt, oracle):
    case = R.synthetic_case()
    for n in (1, 3, 4):
        want = rt.denoise_host(_guides(case, True, True), case["color"], n, *SIGMAS)
        buf = case["color"].copy()
        got = rt.denoise_host(_guides(case, True, True), buf, n, *SIGMAS, out=buf)
        assert got is buf and R.same_bits(buf, want).all(), n


def test_infinite_sigma_color(rt, oracle, cornell_frame):
    """sigma_color = +INF: k_c = 0, the colour term is switched off -- also where a colour difference overflows."""
    inf = (np.inf, 0.3, 1.0)
    _check(rt, oracle, R.synthetic_case(), 3, True, True, inf, "synthetic, sigma_color = inf")
    _check(rt, oracle, cornell_frame, 2, False, True, inf, "cornell, sigma_color = inf")
    big = {k: v.copy() for k, v in R.synthetic_case().items()}
    big["color"][4, 4, :3] = F32(3e38)
    big["color"][4, 5, :3] = F32(-3e38)   # (the difference is infinite, times k_c = 0 a NaN: the tap is skipped)
    _check(rt, oracle, big, 2, True, True, inf, "overflowing difference")
    _check(rt, oracle, big, 2, True, True, SIGMAS, "overflowing difference, finite sigma_color")


@pytest.mark.parametrize("W,H", [(1, 1), (8, 1), (1, 8)])
def test_small_frames(rt, oracle, W, H):
    full = R.synthetic_case()
    case = {k: np.ascontiguousarray(v[8:8 + H, 9:9 + W]) for k, v in full.items()}   # (astride the crease, all filterable)
    assert R.classify(case["color"], case["normal"], case["point"], case["emission"]).all()
    for n in (1, 2, 5):
        got = _check(rt, oracle, case, n, True, True, what=f"{W}x{H}")
        if W * H == 1:   # one texel: the centre tap alone, c / a' * a'
            a = np.maximum(case["albedo"][0, 0, :3], F32(2.0 ** -10))
            c = case["color"][0, 0, :3] / a
            w = F32(9 / 64)
            for _ in range(n):
                c = (w * c) / w
            assert R.same_bits(got[0, 0, :3], c * a).all()


def test_reference_conditions_and_quality(rt, oracle, cornell_frame):
    """On (b) with n = 3 and the sigmas above.  Coverage, on the reference alone: the share of filterable texels, of tap
    pairs that the edge terms nearly reject and that they accept, an emissive texel beside a filterable one, the share of
    texels that change.  Quality: the mean squared error against the 256-frame accumulation over the filterable texels
    falls to at most half the noisy frame's."""
    c = cornell_frame
    ok = R.classify(c["color"], c["normal"], c["point"], c["emission"])
    stats = {}
    ref = R.reference(oracle, c["color"], c["normal"], c["point"], c["albedo"], c["emission"], 3, *SIGMAS, stats=stats)
    share = ok.mean()
    rejected, accepted = stats["rejected"] / stats["pairs"], stats["accepted"] / stats["pairs"]
    changed = (~R.same_bits(ref[..., :3], c["color"][..., :3])).any(-1).mean()
    lamp = (c["emission"][..., :3] != 0).any(-1)
    beside = np.zeros_like(lamp)
    beside[:, 1:] |= lamp[:, 1:] & ok[:, :-1]
    beside[:, :-1] |= lamp[:, :-1] & ok[:, 1:]
    beside[1:] |= lamp[1:] & ok[:-1]
    beside[:-1] |= lamp[:-1] & ok[1:]
    print(f"filterable {share:.3f}, pairs {stats['pairs']}, rejected {rejected:.3f}, accepted {accepted:.3f}, changed {changed:.3f}, "
          f"lamp texels {int(lamp.sum())}, beside a filterable one {int(beside.sum())}")
    assert share >= 0.40
    assert rejected >= 0.05
    assert accepted >= 0.05
    assert beside.any()
    assert changed >= 0.40
    got = rt.denoise_host(_guides(c, True, True), c["color"], 3, *SIGMAS)
    assert R.same_bits(got, ref).all()
    truth = c["converged"][..., :3].astype(np.float64)
    noisy = float(((c["color"][..., :3] - truth)[ok] ** 2).mean())
    filtered = float(((got[..., :3] - truth)[ok] ** 2).mean())
    print(f"mean squared error over the filterable texels: noisy {noisy:.4f}, filtered {filtered:.4f}, ratio {filtered / noisy:.3f}")
    assert filtered <= 0.5 * noisy
