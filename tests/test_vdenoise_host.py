"""rt_denoise_variance_host and rt_luminance_moments_host (include/rt_abi.h; csrc/host/vdenoise.cpp over csrc/rt_vdenoise.h)
against the independent numpy restatement of the definition (tests/_vdenoise_reference.py), bit for bit; conditions on the
reference alone that keep the comparison from passing vacuously; the zero-variance consequence; and what the filter is for
-- on a lone frame and on a long history it does no worse than the fixed-width filter of the parent commit.  No device."""
import itertools

import numpy as np
import pytest

import _denoise_reference as DR
import _vdenoise_reference as R

F32 = np.float32
SIGMAS = (4.0, 0.3, 1.0)   # sigma_luminance, sigma_normal, sigma_point: the wrappers' defaults


def _guides(case, albedo=True, emission=True):
    g = {"normal": case["normal"], "point": case["point"]}
    if albedo:
        g["albedo"] = case["albedo"]
    if emission:
        g["emission"] = case["emission"]
    return g


def _check(rt, oracle, case, n, albedo=True, emission=True, moments=True, sigmas=SIGMAS, min_history=R.MIN_HISTORY, what="", stats=None):
    kw = dict(moments=case["moments"], history=case["history"]) if moments else {}
    want = R.reference(oracle, case["color"], case["normal"], case["point"], case["albedo"] if albedo else None,
                       case["emission"] if emission else None, n, *sigmas, min_history=min_history, stats=stats, **kw)
    g = _guides(case, albedo, emission)
    got = rt.denoise_variance_host(g, case["color"], n, *sigmas, min_history=min_history, out_variance=True, **kw)
    for a, b, name in zip(got, want, ("out", "out_variance")):
        bad = ~R.same_bits(a, b)
        assert not bad.any(), (what, name, n, albedo, emission, moments, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    alone = rt.denoise_variance_host(g, case["color"], n, *sigmas, min_history=min_history, **kw)   # (without out_variance)
    assert isinstance(alone, np.ndarray) and R.same_bits(alone, want[0]).all(), (what, "no out_variance")
    return got


@pytest.fixture(scope="module")
def cornell_frame(rt, oracle, cornell):
    """The Cornell fixture at 67x45: one frame and its guides (_denoise_reference.cornell_case), with the moments of four
    accumulated frames and a history that says 4 on the left half and 1 on the right: both branches in one frame."""
    c = dict(DR.cornell_case(rt, oracle, cornell))
    _, moments, hist = R.cornell_history(rt, oracle, cornell, c, 4)
    hist = hist.copy()
    hist[:, 34:] = np.minimum(hist[:, 34:], F32(1))
    c.update(moments=moments, history=hist)
    return c


def test_synthetic_frame_meets_every_rule(oracle):
    """The 24x16 frame holds what it was built to hold, by the reference's own account (so the sweep below exercises each
    rule)."""
    c, notes = R.synthetic_case()
    st = {}
    R.reference(oracle, c["color"], c["normal"], c["point"], c["albedo"], c["emission"], 3, *SIGMAS, c["moments"], c["history"],
                R.MIN_HISTORY, stats=st)
    ok, temporal, var0 = st["ok"], st["temporal"], st["var0"]
    assert 0.5 < ok.mean() < 0.95 and not (temporal & ~ok).any()
    share = temporal.sum() / ok.sum()
    print(f"filterable {ok.mean():.3f}; of those temporal {share:.3f}, spatial {1 - share:.3f}")
    assert share >= 0.20 and 1 - share >= 0.20
    # histories that do not serve, on filterable texels whose moments would
    for k in ("history_nan", "history_inf", "history_below_one", "history_short"):
        assert ok[notes[k]] and not temporal[notes[k]] and np.isfinite(c["moments"][notes[k]]).all(), k
    h = c["history"]
    assert np.isnan(h[notes["history_nan"]]) and np.isinf(h[notes["history_inf"]]) and h[notes["history_below_one"]] < 1
    assert 1 <= h[notes["history_short"]] < R.MIN_HISTORY
    # moments that do not serve, under a history that would
    for k in ("moment_nan", "moment_inf"):
        assert ok[notes[k]] and not temporal[notes[k]] and h[notes[k]] >= R.MIN_HISTORY and not np.isfinite(c["moments"][notes[k]]).all(), k
    # a second moment below the square of the first: the variance is clamped to 0
    for p in notes["negative"]:
        assert temporal[p] and c["moments"][p][1] < c["moments"][p][0] ** 2 and var0[p] == 0, p
    # a region of variance 0, and variance elsewhere on both branches
    assert temporal[notes["zero"]].all() and (var0[notes["zero"]] == 0).all()
    assert (var0[temporal] > 0).mean() > 0.8 and (var0[ok & ~temporal] > 0).mean() > 0.8
    # the window's taps off the frame and on texels that are not filterable
    print(f"window taps outside the frame {st['window_outside']}, on texels that are not filterable {st['window_unfilterable']}")
    assert st["window_outside"] >= 100 and st["window_unfilterable"] >= 100
    rejected, accepted = st["lum_rejected"] / st["pairs"], st["accepted"] / st["pairs"]
    print(f"tap pairs {st['pairs']}: nearly rejected by the luminance term {rejected:.3f}, accepted {accepted:.3f}")
    assert rejected >= 0.05 and accepted >= 0.05


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("albedo,emission,moments", list(itertools.product((True, False), repeat=3)))
def test_synthetic_frame_equals_the_reference(rt, oracle, n, albedo, emission, moments):
    """Iterations 1 .. 5 (step 16 on 24x16 puts most taps outside the frame), each optional plane present and absent,
    out_variance asked for and not."""
    case, _ = R.synthetic_case()
    out, var = _check(rt, oracle, case, n, albedo, emission, moments, what="synthetic")
    ok = R.classify(case["color"], case["normal"], case["point"], case["emission"] if emission else None)
    assert R.same_bits(out[~ok], case["color"][~ok]).all()          # copied through, NaN and infinity included
    assert R.same_bits(out[..., 3], case["color"][..., 3]).all()    # alpha carried
    assert (var[~ok] == 0).all() and (var[ok] >= 0).all()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("albedo,emission,moments", list(itertools.product((True, False), repeat=3)))
def test_cornell_frame_equals_the_reference(rt, oracle, cornell_frame, n, albedo, emission, moments):
    st = {}
    _check(rt, oracle, cornell_frame, n, albedo, emission, moments, what="cornell", stats=st)
    if moments:
        share = st["temporal"].sum() / st["ok"].sum()
        assert 0.2 < share < 0.8, share


def test_other_parameters(rt, oracle, cornell_frame):
    """Other sigmas and other thresholds of the history: every texel temporal, and none."""
    case, _ = R.synthetic_case()
    for sig in ((0.5, 0.3, 1.0), (50.0, 0.1, 0.2)):
        _check(rt, oracle, case, 3, sigmas=sig, what=sig)
    for mh in (1.0, 3.0, 9.0):
        st = {}
        _check(rt, oracle, cornell_frame, 2, min_history=mh, what=("min_history", mh), stats=st)
        assert st["temporal"].any() == (mh < 9.0)


def test_out_may_be_color(rt, oracle):
    case, _ = R.synthetic_case()
    kw = dict(moments=case["moments"], history=case["history"])
    for n in (1, 3, 4):
        want = rt.denoise_variance_host(_guides(case), case["color"], n, *SIGMAS, out_variance=True, **kw)
        buf = case["color"].copy()
        var = np.zeros(buf.shape[:2], F32)
        got = rt.denoise_variance_host(_guides(case), buf, n, *SIGMAS, out=buf, out_variance=var, **kw)
        assert got[0] is buf and got[1] is var and R.same_bits(buf, want[0]).all() and R.same_bits(var, want[1]).all(), n
    buf = case["color"].copy()
    assert rt.luminance_moments_host(_guides(case), buf, out=buf) is buf
    assert R.same_bits(buf, rt.luminance_moments_host(_guides(case), case["color"])).all()


@pytest.mark.parametrize("W,H", [(1, 1), (8, 1), (1, 8)])
def test_small_frames(rt, oracle, W, H):
    full, _ = R.synthetic_case()
    case = {k: np.ascontiguousarray(v[8:8 + H, 9:9 + W]) for k, v in full.items()}   # (astride the crease and the two histories)
    assert R.classify(case["color"], case["normal"], case["point"], case["emission"]).all()
    for n in (1, 2, 5):
        for moments in (True, False):
            out, var = _check(rt, oracle, case, n, moments=moments, what=f"{W}x{H}")
        if W * H == 1:   # one texel: the centre tap alone; its window holds itself, a variance of 0 but for rounding
            a = np.maximum(case["albedo"][0, 0, :3], F32(2.0 ** -10))
            c = case["color"][0, 0, :3] / a
            w = F32(9 / 64)
            for _ in range(n):
                c = (w * c) / w
            assert R.same_bits(out[0, 0, :3], c * a).all()


def test_luminance_moments_equal_the_reference(rt, oracle, cornell_frame):
    """(l, l l, 0, 0) on the filterable texels; lamps, misses and non-finite texels zeroed."""
    syn, _ = R.synthetic_case()
    for case, what in ((syn, "synthetic"), (cornell_frame, "cornell")):
        for albedo, emission in itertools.product((True, False), repeat=2):
            want = R.moments_reference(case["color"], case["normal"], case["point"], case["albedo"] if albedo else None,
                                       case["emission"] if emission else None)
            got = rt.luminance_moments_host(_guides(case, albedo, emission), case["color"])
            assert R.same_bits(got, want).all(), (what, albedo, emission)
            ok = R.classify(case["color"], case["normal"], case["point"], case["emission"] if emission else None)
            assert (got[~ok] == 0).all() and (got[..., 2:] == 0).all() and (got[ok][:, 0] > 0).mean() > 0.5
            lamp = (case["emission"][..., :3] != 0).any(-1)
            miss = (case["normal"] == 0).all(-1)
            assert lamp.any() and miss.any() and (got[miss] == 0).all() and ((got[lamp] == 0).all() if emission else (got[lamp][:, 0] > 0).any())


def test_zero_variance_leaves_the_frame(rt, oracle, cornell_frame):
    """With var_0 = 0 everywhere D is 2^-30 and every tap whose luminance differs is refused: out is color up to the
    roundings of / a' * a' and (w c) / w, within 1e-5 relative on every filterable texel; the variance stays 0."""
    syn, _ = R.synthetic_case()
    for case, what in ((syn, "synthetic"), (cornell_frame, "cornell")):
        H, W = case["color"].shape[:2]
        moments = np.zeros((H, W, 4), F32)
        moments[..., 0], moments[..., 1] = 2, 4
        history = np.full((H, W), 8, F32)
        ok = R.classify(case["color"], case["normal"], case["point"], case["emission"])
        for n in (1, 3, 5):
            st = {}
            ref = R.reference(oracle, case["color"], case["normal"], case["point"], case["albedo"], case["emission"], n, *SIGMAS,
                              moments, history, R.MIN_HISTORY, stats=st)
            assert st["temporal"][ok].all() and (st["var0"] == 0).all()
            out, var = rt.denoise_variance_host(_guides(case), case["color"], n, *SIGMAS, moments=moments, history=history, out_variance=True)
            assert R.same_bits(out, ref[0]).all() and R.same_bits(var, ref[1]).all()
            c = case["color"][ok][:, :3].astype(np.float64)
            assert (np.abs(out[ok][:, :3] - c) <= 1e-5 * np.abs(c)).all(), (what, n)
            assert (var == 0).all()


def _mse(img, truth, ok):
    return float(((img[..., :3] - truth)[ok] ** 2).mean())


def test_quality_on_a_lone_frame(rt, oracle, cornell_frame):
    """(a) One 8 spp frame, no moments, iterations = 3, defaults: the mean squared error against the 256-frame accumulation
    over the filterable texels is at most half the noisy frame's, and at most denoise_host's at its defaults on the same
    frame.  A float64 prototype of the definition gave 0.0090 against 0.0484 (noisy: 0.2384); measured here, in float32:
    0.00903 against 0.04839 (noisy: 0.23845)."""
    c = cornell_frame
    ok = R.classify(c["color"], c["normal"], c["point"], c["emission"])
    truth = c["converged"][..., :3].astype(np.float64)
    g = _guides(c)
    noisy = _mse(c["color"], truth, ok)
    fixed = _mse(rt.denoise_host(g, c["color"]), truth, ok)
    adaptive = _mse(rt.denoise_variance_host(g, c["color"]), truth, ok)
    print(f"mean squared error over the filterable texels, one frame: noisy {noisy:.5f}, denoise_host {fixed:.5f}, denoise_variance_host {adaptive:.5f}")
    assert adaptive <= 0.5 * noisy
    assert adaptive <= fixed


def test_quality_on_a_long_history(rt, oracle, cornell, cornell_frame):
    """(b) 64 frames, each the raw sample of its own seed, accumulated through temporal_accumulate_host under the unmoved
    camera, and the luminance_moments_host of each raw frame accumulated the same way; iterations = 3, defaults.  The error
    is at most the accumulated input's and at most denoise_host's on that input.  A float64 prototype of the definition
    gave 0.0012 against 0.0027 and 0.0017; measured here, in float32: 0.00115 against 0.00271 and 0.00172."""
    c = cornell_frame
    ok = R.classify(c["color"], c["normal"], c["point"], c["emission"])
    truth = c["converged"][..., :3].astype(np.float64)
    g = _guides(c)
    color, moments, history = R.cornell_history(rt, oracle, cornell, c, 64)
    assert (history[ok] == 64).all()
    st = {}
    R.reference(oracle, color, c["normal"], c["point"], c["albedo"], c["emission"], 1, *SIGMAS, moments, history, R.MIN_HISTORY, stats=st)
    assert st["temporal"][ok].all() and (st["var0"][ok] > 0).mean() > 0.5
    accumulated = _mse(color, truth, ok)
    fixed = _mse(rt.denoise_host(g, color), truth, ok)
    adaptive = _mse(rt.denoise_variance_host(g, color, moments=moments, history=history), truth, ok)
    print(f"mean squared error over the filterable texels, 64 frames: accumulated {accumulated:.5f}, denoise_host {fixed:.5f}, "
          f"denoise_variance_host {adaptive:.5f}")
    assert adaptive <= accumulated
    assert adaptive <= fixed
