"""rt_temporal_accumulate_host (include/rt_abi.h; csrc/host/temporal.cpp over csrc/rt_temporal.h) against the independent
numpy restatement of the definition (tests/_temporal_reference.py), bit for bit; the unmoved camera, where the call is the
shader's own accumulation; and what the call is for -- a camera that moves every frame keeps its history.  No device."""
import itertools

import numpy as np
import pytest

import _temporal_reference as R

F32 = np.float32
DEFAULTS = (0.01, 0.9)   # point_tolerance, normal_cos: the wrappers' defaults


def _host(rt, planes, cam, cap=np.inf, tol=DEFAULTS[0], ncos=DEFAULTS[1], motion=True, **kw):
    g = {k: planes[k] for k in ("point", "normal", "object") if planes.get(k) is not None}
    pg = {k[5:]: planes[k] for k in ("prev_point", "prev_normal", "prev_object") if planes.get(k) is not None}
    return rt.temporal_accumulate_host(g, pg, cam, planes["prev_color"], planes["prev_history"], planes["color"], cap, tol, ncos,
                                       motion=motion, **kw)


def _check(rt, planes, cam, cap=np.inf, tol=DEFAULTS[0], ncos=DEFAULTS[1], motion=True, what="", stats=None):
    want = R.reference(planes, cam, cap, tol, ncos, stats=stats)
    got = _host(rt, planes, cam, cap, tol, ncos, motion)
    assert len(got) == (3 if motion else 2)
    for a, b, name in zip(got, want, ("out", "out_history", "motion")):
        bad = ~R.same_bits(a, b)
        assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    return got, want


def test_synthetic_case_meets_every_rule():
    """The 24x16 pair of frames holds what it was built to hold, by the reference's own account of which rule fired."""
    planes, cam, notes = R.synthetic_case()
    st = {}
    out, hist, motion = R.reference(planes, cam, 4.0, *DEFAULTS, stats=st)
    n, pn = planes["normal"], planes["prev_normal"]
    assert ((n == 0).all(-1)).any() and ((pn == 0).all(-1)).any()                      # a current and a previous miss
    for k in ("color", "point", "normal", "prev_color", "prev_history", "prev_point", "prev_normal"):
        assert (~np.isfinite(planes[k])).any(), k                                      # a NaN or infinity in each plane
    assert not st["reprojectable"][notes["object_says_miss"]] and not st["reprojectable"][15, 7] and not st["reprojectable"][15, 8]
    for k in ("behind", "left", "right", "below", "above", "snap_x_down", "snap_x_up", "snap_y_down", "snap_y_up", "outside",
              "prev_miss", "prev_nan", "history_low", "object", "plane", "normal", "dropped_sample", "capped"):
        assert st[k].any(), k
    assert st["behind"][notes["behind"]] and st["left"][notes["off_left"]] and st["right"][notes["off_right"]]
    assert st["below"][notes["off_below"]] and st["above"][notes["off_above"]]
    for k in ("left_edge", "right_edge", "bottom_edge", "top_edge"):
        assert st["outside"][notes[k]] and st["have"][notes[k]], k                     # a tap outside with weight, others valid
    taps = st["valid_taps"]
    assert taps[notes["one_tap_down"]] == 1 and taps[notes["one_tap_up"]] == 1
    assert taps[notes["two_taps_x"]] == 2 and taps[notes["two_taps_y"]] == 2
    assert (taps == 4).sum() > 100 and (taps == 3).any() and (taps == 0).any()
    assert np.array_equal(motion[notes["one_tap_down"]], F32([2, 1])) and np.array_equal(motion[notes["one_tap_up"]], F32([2, 1]))
    y, x = notes["dropped"]
    assert st["have"][y, x] and np.isfinite(out[y, x]).all() and not np.isfinite(planes["color"][y, x]).all()
    assert (st["capped"] & (hist == 5)).any() and (st["have"] & ~st["capped"] & (hist < 5)).any()
    # without history: the colour bit for bit, history 1; NaN motion exactly where nothing was reprojected
    none = ~st["have"]
    assert R.same_bits(out[none], planes["color"][none]).all() and (hist[none] == 1).all()
    assert np.array_equal(np.isnan(motion).all(-1), ~st["on_screen"]) and (motion.view(np.uint32)[~st["on_screen"]] == 0x7FC00000).all()
    # without the object planes the recess and the box are refused by the plane test alone
    st2 = {}
    R.reference({k: v for k, v in planes.items() if "object" not in k}, cam, 4.0, *DEFAULTS, stats=st2)
    assert not st2["object"].any() and st2["plane"].sum() > st["plane"].sum()


@pytest.mark.parametrize("objects,motion,cap", list(itertools.product((True, False), (True, False), (4.0, np.inf))))
def test_synthetic_frame_equals_the_reference(rt, objects, motion, cap):
    planes, cam, _ = R.synthetic_case()
    if not objects:
        planes = {k: v for k, v in planes.items() if "object" not in k}
    _check(rt, planes, cam, cap, motion=motion, what="synthetic")


def test_one_object_plane_alone_is_not_compared(rt):
    """`object` without `prev_object` still marks misses; `prev_object` alone does nothing."""
    planes, cam, notes = R.synthetic_case()
    a = {k: v for k, v in planes.items() if k != "prev_object"}
    (out, hist, _), _ = _check(rt, a, cam, what="object alone")
    assert hist[notes["object_says_miss"]] == 1
    b = {k: v for k, v in planes.items() if k != "object"}
    none = {k: v for k, v in planes.items() if "object" not in k}
    got, _ = _check(rt, b, cam, what="prev_object alone")
    for u, v in zip(got, _host(rt, none, cam)):
        assert R.same_bits(u, v).all()


def test_tolerances_decide(rt):
    """A tolerance wide enough for the recess and the box, a cosine low enough for the tilted normals: more history."""
    planes, cam, _ = R.synthetic_case()
    none = {k: v for k, v in planes.items() if "object" not in k}
    st, wide = {}, {}
    _check(rt, none, cam, stats=st, what="defaults")
    _check(rt, none, cam, np.inf, 1.0, -1.0, stats=wide, what="wide")
    assert st["plane"].any() and st["normal"].any() and not wide["plane"].any() and not wide["normal"].any()
    assert wide["have"].sum() > st["have"].sum()


@pytest.fixture(scope="module")
def cameras(cornell):
    """The Cornell fixture's camera and two moved ones: a fraction of a texel and several texels at 67x45."""
    cam = cornell.uniform.camera
    return cam, R.moved_camera(cam, right=0.03, up=0.01), R.moved_camera(cam, right=0.5, up=-0.12, forward=0.1)


@pytest.fixture(scope="module")
def cornell_frames(rt, oracle, cornell, cameras):
    """Per camera: guides (oracle.intersect), one 8 spp / 4 bounce frame (oracle.render, frames = 0)."""
    out = []
    for cam in cameras:
        g = R.cornell_guides(oracle, cornell, cam)
        color, _ = oracle.render(rt.make_params(67, 45, 4, 8, skybox=1, frames=0), R.with_camera(cornell, cam))
        out.append((g, color))
    return out


@pytest.mark.parametrize("move", [1, 2])
@pytest.mark.parametrize("objects", [True, False])
def test_cornell_frame_equals_the_reference(rt, cameras, cornell_frames, move, objects):
    """The Cornell fixture at 67x45: history from the fixture's camera, the current frame from a moved one."""
    (pg, prev_color), (g, color) = cornell_frames[0], cornell_frames[move]
    rng = np.random.default_rng(move)
    planes = dict(color=color, point=g["point"], normal=g["normal"], prev_color=prev_color,
                  prev_history=rng.integers(1, 7, prev_color.shape[:2]).astype(F32), prev_point=pg["point"], prev_normal=pg["normal"])
    if objects:
        planes.update(object=g["object"], prev_object=pg["object"])
    st = {}
    for cap in (3.0, np.inf):
        _, (out, hist, motion) = _check(rt, planes, cameras[0], cap, stats=st, what=("cornell", move, cap))
    size = np.linalg.norm(motion[st["have"]], axis=-1).mean()
    share = st["have"].sum() / st["reprojectable"].sum()
    print(f"move {move}: mean |motion| {size:.3f} texel, {share:.3f} of the hit texels find history, valid taps "
          f"{np.bincount(st['valid_taps'][st['on_screen']], minlength=5).tolist()}")
    assert (0.05 < size < 1.0) if move == 1 else (size > 3.0)
    assert share > (0.9 if move == 1 else 0.6)
    assert (st["valid_taps"] == 4).sum() > 0.3 * st["have"].sum() and (st["plane"] | st["object"] | st["prev_miss"]).any()


@pytest.mark.parametrize("W,H", [(1, 1), (8, 1), (1, 8)])
def test_small_frames(rt, W, H):
    planes, cam = R.small_case(W, H)
    for objects, motion in itertools.product((True, False), repeat=2):
        pl = planes if objects else {k: v for k, v in planes.items() if "object" not in k}
        st = {}
        _check(rt, pl, cam, 5.0, motion=motion, stats=st, what=(W, H, objects, motion))
        assert st["have"].all()
        assert (st["valid_taps"] == 2).sum() == max(W, H) - 1 and (st["valid_taps"] == 1).sum() == 1   # (the last texel's neighbour is outside)


def test_out_may_be_color(rt):
    planes, cam, _ = R.synthetic_case()
    want = _host(rt, planes, cam, 4.0)
    buf = planes["color"].copy()
    hist = np.zeros(buf.shape[:2], F32)
    got = _host(rt, dict(planes, color=buf), cam, 4.0, out=buf, out_history=hist)
    assert got[0] is buf and got[1] is hist
    for a, b in zip(got, want):
        assert R.same_bits(a, b).all()


def test_unmoved_camera_is_the_shaders_accumulation(rt, oracle, cornell):
    """Frames 0 .. 3 of oracle.render against: frame 0, then for k = 1 .. 3 the raw sample of frames = -k through
    temporal_accumulate_host with prev_history = k, under the same camera and G-buffer.  Bit for bit on every hit texel,
    alpha included, with motion exactly (0, 0); the other texels hold the raw sample."""
    W, H = 67, 45
    cam = cornell.uniform.camera
    g = R.cornell_guides(oracle, cornell, cam)
    hit = (g["normal"] != 0).any(-1)
    assert 0.5 < hit.mean() < 1.0
    acc, _ = oracle.render(rt.make_params(W, H, 4, 8, skybox=1, frames=0), cornell)
    mine = acc.copy()
    for k in range(1, 4):
        acc, _ = oracle.render(rt.make_params(W, H, 4, 8, skybox=1, frames=k), cornell, image=acc)
        raw, _ = oracle.render(rt.make_params(W, H, 4, 8, skybox=1, frames=-k), cornell)
        mine, hist, motion = rt.temporal_accumulate_host(g, g, cam, mine, np.full((H, W), k, F32), raw, motion=True)
        assert R.same_bits(mine[hit], acc[hit]).all(), k
        assert (~R.same_bits(mine[hit][:, :3], raw[hit][:, :3])).mean() > 0.9, k   # (the blend did something)
        assert np.array_equal(motion[hit], np.zeros_like(motion[hit])) and np.isnan(motion[~hit]).all(), k
        assert (hist[hit] == k + 1).all() and (hist[~hit] == 1).all(), k
        assert R.same_bits(mine[~hit], raw[~hit]).all(), k


STEP = 0.05   # the camera's sideways move per frame, world units: about 0.4 texel at 67x45 on the back wall


def test_a_moving_camera_keeps_its_history(rt, oracle, cornell):
    """16 frames of the Cornell fixture at 67x45, 8 spp / 4 bounces, the camera `STEP` further right each frame, every frame
    the raw sample of its own seed (frames = -k), max_history = inf and the default tolerances.  Against a 256-frame
    accumulation at the last camera, over the hit texels whose history reached 8 frames: the mean squared error is at
    most half a single frame's (a mean of eight or more independent frames has at most 1/8; the margin is for the
    bilinear resampling and the restarts).  Measured: 0.028 of the single frame's (0.0057 against 0.2076) over 0.981 of the
    hit texels, mean |motion| 0.646 texel -- below the 1/16 of sixteen independent frames because every bilinear fetch
    also averages neighbouring texels, which this smooth scene forgives.
    Two conditions on the inputs, by the numpy reference: those texels are at least 60 % of the hit texels, and their mean
    |motion| in the last step is at least 0.25 texel."""
    W, H, N = 67, 45, 16
    base = cornell.uniform.camera
    cams = [R.moved_camera(base, right=STEP * (k - (N - 1) / 2)) for k in range(N)]
    out = hist = None
    for k in range(N):
        raw, _ = oracle.render(rt.make_params(W, H, 4, 8, skybox=1, frames=-k), R.with_camera(cornell, cams[k]))
        g = R.cornell_guides(oracle, cornell, cams[k])
        if k == 0:
            out, hist = raw.copy(), np.ones((H, W), F32)
            continue
        pg = R.cornell_guides(oracle, cornell, cams[k - 1])
        planes = dict(color=raw, point=g["point"], normal=g["normal"], object=g["object"], prev_color=out, prev_history=hist,
                      prev_point=pg["point"], prev_normal=pg["normal"], prev_object=pg["object"])
        if k == N - 1:
            (out, hist, motion), ref = _check(rt, planes, cams[k - 1], what="the last step")
        else:
            out, hist, motion = _host(rt, planes, cams[k - 1])
    last = R.with_camera(cornell, cams[-1])
    truth = None
    for f in range(256):
        truth, _ = oracle.render(rt.make_params(W, H, 4, 8, skybox=1, frames=f), last, image=truth)
    hit = (g["normal"] != 0).any(-1)
    old = hit & (ref[1] >= 8)
    share = old.sum() / hit.sum()
    size = float(np.linalg.norm(ref[2][old], axis=-1).mean())
    t = truth[..., :3].astype(np.float64)
    single = float(((raw[..., :3] - t)[old] ** 2).mean())
    kept = float(((out[..., :3] - t)[old] ** 2).mean())
    print(f"history >= 8 on {share:.3f} of the hit texels, mean |motion| {size:.3f} texel; mean squared error: single frame "
          f"{single:.4f}, accumulated {kept:.4f}, ratio {kept / single:.3f}; history mean {hist[old].mean():.2f}")
    assert share >= 0.60
    assert size >= 0.25
    assert kept <= 0.5 * single
