"""rt_upsample_host (include/rt_abi.h; csrc/host/upsample.cpp over csrc/rt_upsample.h) against the independent numpy
restatement of the definition (tests/_upsample_reference.py), bit for bit; the two consequences the header states; and what
the call is for -- a frame traced at a quarter of the texels, carried up, is no worse than the full-resolution frame of the
same ray count.  No device."""
import numpy as np
import pytest

import _denoise_reference as DR
import _upsample_reference as R

F32 = np.float32
DEFAULTS = (0.02, 0.9)   # point_tolerance, normal_cos: the wrappers' defaults
SIZES = [(1, 1, 8, 8), (8, 1, 1, 8), (24, 16, 24, 16), (24, 16, 61, 37), (67, 45, 34, 23)]


def _host(rt, lo, hi, tol=DEFAULTS[0], ncos=DEFAULTS[1], coverage=True, **kw):
    return rt.upsample_host(R.without(lo, "color"), hi, lo["color"], tol, ncos, coverage=coverage, **kw)


def _check(rt, lo, hi, tol=DEFAULTS[0], ncos=DEFAULTS[1], what="", stats=None):
    want = R.reference(lo, hi, tol, ncos, stats=stats)
    got = _host(rt, lo, hi, tol, ncos)
    bad = ~R.same_bits(got[0], want[0])
    assert not bad.any(), (what, "out", int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert got[1].dtype == np.uint8 and np.array_equal(got[1], want[1]), (what, "coverage", np.argwhere(got[1] != want[1])[:4].tolist())
    alone = _host(rt, lo, hi, tol, ncos, coverage=False)
    assert isinstance(alone, np.ndarray) and R.same_bits(alone, want[0]).all(), (what, "without coverage")
    return got, want


def _variants(lo, hi):
    """The optional planes on and off."""
    yield "all", lo, hi
    yield "no emission", lo, R.without(hi, "emission")
    yield "no albedo", R.without(lo, "albedo"), R.without(hi, "albedo")
    yield "neither", R.without(lo, "albedo"), R.without(hi, "albedo", "emission")


def test_synthetic_case_meets_every_rule():
    """The synthetic pairs hold what they were built to hold, by the reference's own account of which rule fired."""
    lo, hi, notes = R.synthetic_case()
    st = {}
    out, cov = R.reference(lo, hi, *DEFAULTS, stats=st)
    for k in R.REASONS:
        assert st["fired"][k].any() and st["alone"][k].any(), k                    # each reason a tap is refused, alone
    assert (cov == 2).mean() > 0.8 and (cov == 1).sum() >= 4 and (cov == 0).sum() >= 4
    assert (st["valid_taps"] == 4).any() and (st["valid_taps"] == 3).any() and (st["valid_taps"] == 1).any()
    assert (st["valid_taps2"] > 0).any() and (st["valid_taps2"] == 0).any()       # ring 2 reached; a hole
    g = st["guided"]
    miss = hi["object"] == R.NO_OBJECT
    assert miss.any() and not g[miss].any() and (cov[miss] == 2).all()             # a miss matches a miss
    lamp = notes["lamp"]
    assert lamp.sum() >= 4 and not g[lamp].any() and (cov[lamp] == 2).any()        # a lamp matches its own lamp
    for k in ("hi_normal_nan", "hi_point_inf", "hi_depth_zero", "hi_depth_nan"):
        assert not g[notes[k]] and cov[notes[k]] == 2, k                           # a NaN texel is PLAIN and takes its object's taps
    assert g[notes["hi_alone"]] and cov[notes["hi_alone"]] == 0                    # an object the low frame does not hold
    assert not np.isfinite(lo["color"]).all() and np.isfinite(out).all()           # non-finite low colours are never carried
    al = lo["albedo"][..., :3]
    assert (al < R.FLOOR).any() and (al == R.FLOOR).any() and np.isnan(al).any()   # demodulation at the floor
    assert (out[notes["hi_black"]][:3] == 0).all() and g[notes["hi_black"]]
    # ... and what they change: without the albedo planes the guided texels differ, the PLAIN ones do not
    out2, cov2 = R.reference(R.without(lo, "albedo"), R.without(hi, "albedo"), *DEFAULTS)
    assert np.array_equal(cov, cov2) and R.same_bits(out[~g], out2[~g]).all() and (~R.same_bits(out[g], out2[g])).mean() > 0.5
    # the snap pair: both thresholds exactly, on both axes
    lo, hi = R.snap_case()
    st = {}
    R.reference(lo, hi, *DEFAULTS, stats=st)
    assert st["tx"][0, 1] == 0 and st["x0"][0, 1] == 0 and st["snap_x_down"][0, 1] and st["tx"][0, 2] == F32(2 / 64)
    assert st["tx"][0, 63] == 0 and st["x0"][0, 63] == 1 and st["snap_x_up"][0, 63] and st["tx"][0, 62] == F32(62 / 64)
    assert st["ty"][1, 0] == 0 and st["snap_y_down"][1, 0] and st["ty"][63, 0] == 0 and st["y0"][63, 0] == 1 and st["snap_y_up"][63, 0]


def test_synthetic_frames_equal_the_reference(rt):
    lo, hi, _ = R.synthetic_case()
    for what, l, h in _variants(lo, hi):
        _check(rt, l, h, what=("synthetic", what))
    for what, l, h in _variants(*R.snap_case()):
        _check(rt, l, h, what=("snap", what))


def test_tolerances_decide(rt):
    """A tolerance wide enough for the displaced point, a cosine low enough for the tilted normal: fewer refusals."""
    lo, hi, notes = R.synthetic_case()
    st, wide = {}, {}
    _check(rt, lo, hi, stats=st, what="defaults")
    _check(rt, lo, hi, 1.0, -1.0, stats=wide, what="wide")
    assert st["fired"]["plane"].any() and st["fired"]["normal"].any()
    # (the panels' own seams still fail the plane test at any tolerance below their distance; the displaced texel does not)
    for k, rule in (("plane", "plane"), ("tilt", "normal")):
        y, x = notes[k]
        Y, X = int(round(y * 36 / 15)), int(round(x * 60 / 23))   # (the high texel nearest the low one)
        assert st["fired"][rule][Y, X] and not wide["fired"][rule][Y, X], k
    assert wide["valid_taps"].sum() > st["valid_taps"].sum()


@pytest.mark.parametrize("w,h,W,H", SIZES)
def test_sizes_equal_the_reference(rt, w, h, W, H):
    lo, hi = R.pair(w, h, W, H)
    for what, l, hh in _variants(lo, hi):
        (out, cov), _ = _check(rt, l, hh, what=(w, h, W, H, what))
    assert out.shape == (H, W, 4) and cov.shape == (H, W)


@pytest.fixture(scope="module")
def cornell_pair(rt, oracle, cornell):
    """The Cornell fixture at 34x23 and 67x45 (rx = ry = 0.5 exactly): both G-buffers from the oracle, the low frame at 32
    and at 8 spp, and tests/_denoise_reference.py's full-resolution case (one 8 spp frame, the 256-frame accumulation)."""
    w, h, W, H = 34, 23, 67, 45
    lo_g, hi_g = R.cornell_planes(oracle, cornell, w, h), R.cornell_planes(oracle, cornell, W, H)
    low = {spp: oracle.render(rt.make_params(w, h, 4, spp, skybox=1, frames=0), cornell)[0].copy() for spp in (32, 8)}
    return lo_g, hi_g, low, DR.cornell_case(rt, oracle, cornell)


def test_cornell_pair_equals_the_reference(rt, cornell_pair):
    lo_g, hi_g, low, _ = cornell_pair
    lo = dict(R.without(lo_g, "depth", "emission"), color=low[8])
    for what, l, hh in _variants(lo, hi_g):
        _check(rt, l, hh, what=("cornell", what))


def test_equal_sizes_copy_the_colour(rt):
    """Consequence 1: the low planes being the high planes themselves, no albedo planes, normal_cos <= 0.99 -- every texel
    whose colour is finite takes one tap of weight 1 and `out` is the colour bit for bit."""
    lo, hi, _ = R.synthetic_case()
    W, H = 61, 37
    rng = np.random.default_rng(3)
    color = np.concatenate([rng.uniform(0, 3, (H, W, 3)), rng.uniform(0, 1, (H, W, 1))], -1).astype(F32)
    color[5, 7, 2] = np.nan
    color[9, 40, 3] = np.inf
    g = R.without(hi, "albedo")
    for guides in (g, R.without(g, "emission")):
        for ncos in (0.99, 0.9, -1.0):
            out, cov = rt.upsample_host(R.without(guides, "depth", "emission"), guides, color, 0.02, ncos, coverage=True)
            ok = np.isfinite(color).all(-1)
            assert ok.sum() == W * H - 2
            assert R.same_bits(out[ok], color[ok]).all() and (cov[ok] == 2).all(), ncos
            assert (cov[~ok] < 2).all() and np.isfinite(out[~ok]).all(), ncos


def test_even_texels_of_a_doubled_frame_are_the_low_texels(rt, cornell_pair):
    """Consequence 2: W == 2w - 1 and H == 2h - 1, both G-buffers traced through the same rays, no albedo planes -- the
    texels with X and Y even hold the low texels' colour bit for bit, wherever that is finite."""
    lo_g, hi_g, low, _ = cornell_pair
    lo = R.without(lo_g, "depth", "emission", "albedo")
    for hi in (R.without(hi_g, "albedo"), R.without(hi_g, "albedo", "emission")):
        out, cov = rt.upsample_host(lo, hi, low[8], coverage=True)
        assert np.isfinite(low[8]).all()
        assert R.same_bits(out[::2, ::2], low[8]).all() and (cov[::2, ::2] == 2).all()
        assert (~R.same_bits(out[1::2, 1::2], low[8][:-1, :-1])).mean() > 0.5     # (the others are blends, but for the sky)


def test_outputs_may_be_given(rt):
    lo, hi, _ = R.synthetic_case()
    want = _host(rt, lo, hi)
    out, cov = np.zeros((37, 61, 4), F32), np.zeros((37, 61), np.uint8)
    got = _host(rt, lo, hi, out=out, coverage=cov)
    assert got[0] is out and got[1] is cov and R.same_bits(out, want[0]).all() and np.array_equal(cov, want[1])


def test_a_quarter_of_the_texels_is_no_worse(rt, cornell_pair):
    """The Cornell pair 34x23 -> 67x45, 4 bounces, against the 256-frame accumulation at 67x45, over ALL texels that hit
    geometry and are not the lamp (holes included).  The reference is one full-resolution frame at 8 spp.  The low frame at
    32 spp -- the same number of rays -- upsampled has at most half its mean squared error (a numpy prototype of the definition measured
    0.161; the bound is the margin DESIGN.md section 2.13 gave its own 0.203), and the low frame at 8 spp -- a quarter of
    the rays -- at most the same error (prototype: 0.543; break-even is the claim).
    Measured: 32 spp 0.1611, 8 spp 0.5433 of the full-resolution frame's 0.2384; coverage over those texels: ring 1 0.9886,
    ring 2 0.0063, holes 0.0051."""
    lo_g, hi_g, low, case = cornell_pair
    lo = R.without(lo_g, "depth", "emission")
    truth = case["converged"][..., :3].astype(np.float64)
    where = (hi_g["normal"] != 0).any(-1) & (hi_g["emission"][..., :3] == 0).all(-1)
    assert 0.4 < where.mean() < 0.7
    single = float(((case["color"][..., :3] - truth)[where] ** 2).mean())
    ratios = {}
    for spp in (32, 8):
        out, cov = rt.upsample_host(lo, hi_g, low[spp], coverage=True)
        ratios[spp] = float(((out[..., :3] - truth)[where] ** 2).mean()) / single
        shares = [float((cov[where] == k).mean()) for k in (2, 1, 0)]
        print(f"{spp} spp low frame upsampled: ratio {ratios[spp]:.4f} of the full-resolution frame's {single:.4f}; "
              f"ring 1 {shares[0]:.4f}, ring 2 {shares[1]:.4f}, holes {shares[2]:.4f} of {int(where.sum())} texels")
    assert ratios[32] <= 0.5
    assert ratios[8] <= 1.0
