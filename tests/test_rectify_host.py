"""rt_temporal_rectify_host (include/rt_abi.h; csrc/host/rectify.cpp over csrc/rt_rectify.h) against the independent numpy
restatement of the definition (tests/_rectify_reference.py), bit for bit; the header's consequences; and what the call is for
-- a lamp that is dimmed stops lagging, a scene that does not change loses nothing.  No device."""
import itertools

import numpy as np
import pytest

import _rectify_reference as R
import _temporal_deform_reference as TD
import _temporal_motion_reference as TM
import _temporal_reference as T

F32 = np.float32
INF = float("inf")


def test_synthetic_case_meets_every_rule():
    """The 40x20 frame holds what it was built to hold, by the reference's own account of which rule fired."""
    planes, notes = R.synthetic_case()
    kw = dict(R.variants(planes))
    st, st0 = {}, {}
    with_obj, without = kw["all"], kw["no object"]
    out, hist, mom, clip = R.reference(**with_obj, **R.DEFAULTS, stats=st)
    out0, hist0, mom0, clip0 = R.reference(**without, **R.DEFAULTS, stats=st0)
    color, history, length = planes["color"], planes["history"], planes["history_length"]
    # no history: every form, and only those texels; the colour bit for bit, length 1, the moments, byte 0
    none = np.zeros(length.shape, bool)
    for p in notes["no_history"]:
        none[p] = True
    assert len(notes["no_history"]) == 17 and np.array_equal(~st["have"], none) and np.array_equal(~st0["have"], none)
    for comp, kind in itertools.product(range(4), (np.isnan, np.isposinf, np.isneginf)):
        assert kind(history[none][:, comp]).any(), (comp, kind)
    bad = length[none]
    assert (bad == 0).any() and (bad == 0.5).any() and np.isnan(bad).any() and np.isposinf(bad).any() and np.isneginf(bad).any()
    assert R.same_bits(out[none], color[none]).all() and (hist[none] == 1).all() and (clip[none] == 0).all()
    assert R.same_bits(mom[none], planes["moments"][none]).all() and (clip[~none] > 0).all()
    # the window: corners, edges and the interior; taps that are not finite; the tap with an infinite alpha counts
    c0 = st0["count"]
    assert c0[19, 0] == 16 and c0[0, 39] == 16 and c0[0, 10] == 28 and c0[10, 39] == 28 and c0.max() == 49
    assert c0[notes["nan_sample"]] == 48 and c0[notes["alpha_sample"]] == 49 and c0[5, 27] == 47   # (3, 24) and (4, 28) are in reach
    for k in ("nan_sample", "inf_sample", "alpha_sample"):
        assert st["dropped"][notes[k]] and not np.isfinite(color[notes[k]]).all(), k
        h4 = out[notes[k]]
        assert np.isfinite(h4).all() and hist[notes[k]] <= length[notes[k]], k     # the sample was dropped: h', n'
    assert st["dropped"].sum() == 4 and (~np.isfinite(color[..., :3])).any(-1).sum() == 3
    # the object plane: another object's neighbours do not count; a lone texel has c = 1 and no box, whatever its history
    c = st["count"]
    assert c[notes["island"]] == 12 and c0[notes["island"]] == 49 and (c <= c0).all() and (c < c0).sum() > 100
    assert c[notes["lone"]] == 1 and not st["box"][notes["lone"]] and clip[notes["lone"]] == R.KEPT and clip0[notes["lone"]] == R.CLIPPED
    assert c[18, 15] == 7 and (planes["object"][18, 5:30] == 0xFFFFFFFF).all()    # misses match misses: the band's own row
    # sd = 0: the block's centre without the plane, the island with it
    for p in (notes["equal_kept"], notes["equal_above"], notes["equal_below"]):
        assert (st0["sd"][p] == 0).all() and c0[p] == 49, p
    assert (st["sd"][notes["island"]] == 0).all() and (st0["sd"][notes["island"]] > 0).all()
    assert clip0[notes["equal_kept"]] == R.KEPT and st0["at_hi"][notes["equal_above"]].all() and st0["at_lo"][notes["equal_below"]].all()
    assert st["at_lo"][notes["island"]].tolist() == [True, False, False] and st["at_hi"][notes["island"]].tolist() == [False, True, True]
    # lo in one channel and hi in another; the length cut, and too short to be cut
    for k in ("cut", "short", "edge", "corner"):
        assert st["at_lo"][notes[k]][0] and st["at_hi"][notes[k]][1] and clip[notes[k]] == R.CLIPPED, k
    assert st["cut"][notes["cut"]] and hist[notes["cut"]] == 5 and length[notes["cut"]] == 9
    assert not st["cut"][notes["short"]] and hist[notes["short"]] == 3 and length[notes["short"]] == 2
    assert 0.2 < st["clipped"].mean() < 0.8 and (st["at_lo"].any(-1) & ~st["at_hi"].any(-1)).any() and (st["at_hi"].any(-1) & ~st["at_lo"].any(-1)).any()
    # -0
    assert (color.view(np.uint32) == 0x80000000).sum() == 3 and (history.view(np.uint32) == 0x80000000).sum() == 2
    # the moments' two rules
    m, hm = planes["moments"], planes["history_moments"]
    assert R.same_bits(mom[notes["hm_bad"]], m[notes["hm_bad"]]).all() and R.same_bits(mom[notes["m_bad"]], hm[notes["m_bad"]]).all()
    assert R.same_bits(mom[notes["both_bad"]], m[notes["both_bad"]]).all()
    ok = st["have"] & np.isfinite(m).all(-1) & np.isfinite(hm).all(-1)
    assert (~R.same_bits(mom[ok], m[ok])).any(-1).all() and (~R.same_bits(mom[ok], hm[ok])).any(-1).all()
    # clip_sigma 0 clips all but a history that is the mean itself; +INF forms no box
    s0, sinf = {}, {}
    R.reference(**without, radius=3, clip_sigma=0.0, clip_history=4.0, stats=s0)
    R.reference(**without, radius=3, clip_sigma=INF, clip_history=4.0, stats=sinf)
    assert s0["clipped"].sum() >= s0["have"].sum() - 2 and not s0["clipped"][notes["equal_kept"]]
    assert not sinf["box"].any() and not sinf["clipped"].any()


@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("clip_sigma", [0.0, 1.0, INF])
def test_synthetic_frame_equals_the_reference(rt, radius, clip_sigma):
    planes, _ = R.synthetic_case()
    for (name, kw), clip_history in itertools.product(R.variants(planes), (4.0, 1.0, INF)):
        R.check(rt.temporal_rectify_host, kw, (name, radius, clip_sigma, clip_history), radius=radius, clip_sigma=clip_sigma,
                clip_history=clip_history)


@pytest.mark.parametrize("W,H", [(1, 1), (1, 8), (8, 1), (7, 5)])
def test_small_frames(rt, W, H):
    planes = R.small_case(W, H)
    for (name, kw), radius in itertools.product(R.variants(planes), (1, 2, 3)):
        out, hist, _, clip = R.check(rt.temporal_rectify_host, kw, (W, H, name, radius), radius=radius, clip_sigma=0.5, clip_history=2.0)
        assert (clip > 0).all()
        if (W, H) == (1, 1):
            assert clip[0, 0] == R.KEPT     # c = 1: no box


def test_outputs_may_be_the_history_planes(rt):
    planes, _ = R.synthetic_case()
    kw = dict(R.variants(planes))["all"]
    want = rt.temporal_rectify_host(**kw, clipped=True)
    bufs = [planes[k].copy() for k in ("history", "history_length", "history_moments")]
    given = dict(kw, history=bufs[0], history_length=bufs[1], history_moments=bufs[2])
    got = rt.temporal_rectify_host(**given, out=bufs[0], out_history=bufs[1], out_moments=bufs[2], clipped=True)
    assert all(g is b for g, b in zip(got, bufs))
    for a, b in zip(got, want):
        assert R.same_bits(a, b).all()


def test_equal_colours_clip_the_history_onto_the_colour(rt):
    """Consequence 3, seen through a dropped sample (out = h'): an infinite alpha leaves the texel's rgb in the window."""
    planes, notes = R.synthetic_case()
    color = planes["color"].copy()
    for k in ("equal_above", "equal_below", "island"):
        color[notes[k]][3] = np.inf
    for objects, names in ((False, ("equal_above", "equal_below")), (True, ("island",))):
        out, hist, clip = rt.temporal_rectify_host(color, planes["history"], planes["history_length"],
                                                   object=planes["object"] if objects else None, clipped=True)
        for k in names:
            p = notes[k]
            assert clip[p] == R.CLIPPED and R.same_bits(out[p][:3], F32(R.EQUAL)).all(), (k, out[p])
            assert R.same_bits(out[p][3], planes["history"][p][3]) and hist[p] == min(planes["history_length"][p], 4.0), k


def _consequence_1(rt, call_kw, planes, cap, what):
    """temporal_reproject_host then temporal_rectify_host at clip_sigma = +INF against temporal_accumulate_host itself; and
    consequence 4: at any clip_sigma, the texels that were not clipped."""
    g, pg, cam = call_kw.pop("guides"), call_kw.pop("prev_guides"), call_kw.pop("cam")
    args = (g, pg, cam, planes["prev_color"], planes["prev_history"])
    want = rt.temporal_accumulate_host(*args, planes["color"], cap, **call_kw)
    h, n = rt.temporal_reproject_host(*args, cap, **call_kw)
    assert np.isnan(h).all(-1).any() and np.isfinite(h).all(-1).any() and (n > 1).any(), what
    assert (~np.isfinite(planes["color"])).any(), what     # a sample that is dropped is among them
    for radius, obj in itertools.product((1, 3), (None, planes.get("object"))):
        got = rt.temporal_rectify_host(planes["color"], h, n, object=obj, radius=radius, clip_sigma=INF, clip_history=1.0)
        for a, b, name in zip(got, want, ("out", "out_history")):
            bad = ~R.same_bits(a, b)
            assert not bad.any(), (what, radius, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        out, hist, clip = rt.temporal_rectify_host(planes["color"], h, n, object=obj, radius=radius, clip_sigma=0.75, clipped=True)
        kept = clip != R.CLIPPED
        assert (clip == R.CLIPPED).any() and (clip == R.KEPT).any() and (clip == 0).any(), what
        assert R.same_bits(out[kept], want[0][kept]).all() and R.same_bits(hist[kept], want[1][kept]).all(), (what, radius, "consequence 4")


@pytest.mark.parametrize("cap", [4.0, INF])
def test_infinite_sigma_is_temporal_accumulation(rt, cap):
    """Consequence 1 on the synthetic pairs of the three temporal tests, each with a camera move."""
    planes, cam, _ = T.synthetic_case()
    g = {k: planes[k] for k in ("point", "normal", "object")}
    pg = {k[5:]: planes[k] for k in ("prev_point", "prev_normal", "prev_object")}
    _consequence_1(rt, dict(guides=g, prev_guides=pg, cam=cam), planes, cap, "plain")
    planes, cam, motions, _ = TM.synthetic_case()
    g = {k: planes[k] for k in ("point", "normal", "object")}
    pg = {k[5:]: planes[k] for k in ("prev_point", "prev_normal", "prev_object")}
    _consequence_1(rt, dict(guides=g, prev_guides=pg, cam=cam, motions=motions), planes, cap, "moving")
    planes, cam, motions, tris, _ = TD.synthetic_case()
    g, pg = TD.split(planes)
    _consequence_1(rt, dict(guides=g, prev_guides=pg, cam=cam, motions=motions, prev_triangles=tris, tri_first=TD.TRI_FIRST), planes, cap,
                   "deforming")


def test_sanitizer_driver(rt, tmp_path):
    """tests/cpp/rectify_driver.cpp with host/rectify.cpp under AddressSanitizer and UndefinedBehaviorSanitizer, a program of
    its own: frames of 1x1, 7x5 and 40x9 on exactly sized heap buffers at every radius, every optional plane on and off, the
    outputs in place and not.  The 7x5 outputs it writes are the wrapper's."""
    import os
    import subprocess
    from conftest import ROOT
    exe = tmp_path / "rectify_driver"
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "rectify_driver.cpp"),
                    os.path.join(ROOT, "ray_tracer_2_amd", "csrc", "host", "rectify.cpp"), "-o", str(exe)], check=True)
    res = tmp_path / "out.bin"
    done = subprocess.run([str(exe), str(res)], capture_output=True, text=True)
    assert done.returncode == 0, (done.stdout, done.stderr)
    for size in ("1x1", "7x5", "40x9"):
        assert f"{size} ok" in done.stdout, done.stdout
    # the driver's frame: ramp(i) = lo + span * ((37 i) % 101) / 101 in binary32, a few texels salted
    w, h = 7, 5
    n = w * h
    ramp = lambda i, lo, span: (F32(span) * ((i * 37) % 101).astype(F32) / F32(101) + F32(lo)).astype(F32)   # noqa: E731
    i4, i1 = np.arange(4 * n), np.arange(n)
    color, history = ramp(i4, 0.2, 0.8), ramp(i4 + 13, 0.3, 0.6)
    moments, hmoments = ramp(i4 + 5, 0.0, 2.0), ramp(i4 + 29, 0.0, 2.0)
    length, obj = (1 + i1 % 9).astype(F32), ((i1 // 3) % 2).astype(np.uint32)
    color[4 * 2 + 1], color[4 * 5 + 3], history[4 * 3], length[4], hmoments[4 * 6 + 2] = np.nan, np.inf, np.nan, 0.5, np.inf
    shape = lambda a: a.reshape(h, w, 4) if a.size == 4 * n else a.reshape(h, w)   # noqa: E731
    want = rt.temporal_rectify_host(shape(color), shape(history), shape(length), shape(obj), radius=2, moments=shape(moments),
                                    history_moments=shape(hmoments), clipped=True)
    raw = np.fromfile(res, np.uint8)
    assert raw.size == n * (16 + 4 + 16 + 1)
    got = (raw[:16 * n].view(F32), raw[16 * n:20 * n].view(F32), raw[20 * n:36 * n].view(F32), raw[36 * n:])
    for a, b in zip(got[:3], want[:3]):
        assert R.same_bits(a, b.ravel()).all()
    assert np.array_equal(got[3], want[3].ravel()) and set(want[3].ravel()) == {0, 1, 2}


# ---- the Cornell fixture: frames of oracle.render ----
W, H, SPP, BOUNCES, FRAMES, CHANGE = 67, 45, 8, 4, 24, 16
BRIGHT, DIM = 34.0, 8.5


def lamp_of(arrays):
    """The mesh with emission_strength > 0."""
    lit = np.flatnonzero(arrays.meshes["material"]["emission_strength"] > 0)
    assert len(lit) == 1
    return int(lit[0])


def with_lamp(arrays, strength):
    meshes = arrays.meshes.copy()
    meshes["material"]["emission_strength"][lamp_of(arrays)] = strength
    return type(arrays)(arrays.uniform, arrays.spheres, meshes, arrays.triangles, arrays.nodes, arrays.textures)


@pytest.fixture(scope="module")
def sequences(rt, oracle, cornell):
    """Per lamp strength: the raw 8 spp / 4 bounce frames of seeds 0 .. 23 (frames = -k) and a 256-frame accumulation; the
    guides; the texels the error is taken over -- hit, and not the lamp."""
    assert cornell.meshes["material"]["emission_strength"][lamp_of(cornell)] == BRIGHT
    raw, truth = {}, {}
    for s in (BRIGHT, DIM):
        a = with_lamp(cornell, s)
        raw[s] = [oracle.render(rt.make_params(W, H, BOUNCES, SPP, skybox=1, frames=-k if k else 0), a)[0] for k in range(FRAMES)]
        acc = None
        for f in range(256):
            acc, _ = oracle.render(rt.make_params(W, H, BOUNCES, SPP, skybox=1, frames=f), a, image=acc)
        truth[s] = acc
    g = T.cornell_guides(oracle, cornell, cornell.uniform.camera)
    mask = (g["normal"] != 0).any(-1) & (g["object"] != lamp_of(cornell))
    assert 0.5 < mask.mean() < 1.0
    return raw, truth, g, mask


def run(rt, cornell, frames, g, rectify):
    """The accumulated frame after each of `frames`, and with `rectify` the clipped byte of each step."""
    cam = cornell.uniform.camera
    acc, n = frames[0].copy(), np.ones((H, W), F32)
    outs, clips = [acc], [np.zeros((H, W), np.uint8)]
    for raw in frames[1:]:
        if rectify:
            h, hn = rt.temporal_reproject_host(g, g, cam, acc, n)
            acc, n, clip = rt.temporal_rectify_host(raw, h, hn, object=g["object"], clipped=True)
            clips.append(clip)
        else:
            acc, n = rt.temporal_accumulate_host(g, g, cam, acc, n, raw)
        outs.append(acc)
    return outs, clips


def mse(img, truth, mask):
    return float(((img[..., :3].astype(np.float64) - truth[..., :3].astype(np.float64))[mask] ** 2).mean())


def test_cornell_frames_equal_the_reference(rt, sequences):
    raw, _, g, _ = sequences
    history, color = raw[BRIGHT][0], raw[DIM][1]
    length = np.random.default_rng(3).integers(1, 9, (H, W)).astype(F32)
    planes = dict(color=color, history=history, history_length=length, object=g["object"],
                  moments=rt.luminance_moments_host(g, color), history_moments=rt.luminance_moments_host(g, history))
    for (name, kw), radius in itertools.product(R.variants(planes), (1, 2, 3)):
        _, _, _, clip = R.check(rt.temporal_rectify_host, kw, ("cornell", name, radius), radius=radius, clip_sigma=1.0, clip_history=4.0)
        assert (clip == R.CLIPPED).mean() > 0.05 and (clip == R.KEPT).mean() > 0.05


def test_a_dimmed_lamp_stops_lagging_and_a_still_scene_loses_nothing(rt, cornell, sequences):
    """The Cornell fixture at 67x45, 8 spp / 4 bounces, the camera still, 24 frames, frame k the raw sample of seed k;
    temporal_reproject_host then temporal_rectify_host with the defaults (radius 3, clip_sigma 1, clip_history 4, the object
    plane given) in every frame from k = 1, against plain temporal_accumulate_host.  Mean squared rgb error against a
    256-frame accumulation of the final scene over the hit texels that are not the lamp.
    DIMMED: the lamp's emission_strength goes 34 -> 8.5 from k = 16.  Asserted: rectified <= 0.5 x plain at k = 16 and k = 23,
    and at least 0.05 of those texels clipped at k = 16.
    STILL: nothing changes.  Asserted: rectified <= 1.25 x plain at k = 16, 19, 23, and at most 0.10 of those texels clipped.
    BRIGHTENED: 8.5 -> 34 from k = 16, printed and not asserted: the old, darker history lies inside the new frame's wide
    noise box and is not clipped, while the cut histories cost noise -- the method's limit.
    Measured with the binary32 host form (plain, rectified, clipped share):
      dimmed     k = 16: 0.01931, 0.00217, 0.118 (a single frame: 0.01613);  k = 23: 0.00987, 0.00071, 0.028
      still      k = 16: 0.01326, 0.00930, 0.039;  k = 19: 0.01162, 0.01003, 0.030;  k = 23: 0.00923, 0.00883, 0.047
      brightened k = 16: 0.00794, 0.00977, 0.023;  k = 19: 0.00756, 0.01023, 0.026;  k = 23: 0.00664, 0.00909, 0.042
    -- ratios 0.112 and 0.072 (dimmed), 0.70, 0.86 and 0.96 (still), 1.23, 1.35 and 1.37 (brightened)."""
    raw, truth, g, mask = sequences
    rows = {}
    for name, first, then in (("dimmed", BRIGHT, DIM), ("still", BRIGHT, BRIGHT), ("brightened", DIM, BRIGHT)):
        frames = raw[first][:CHANGE] + raw[then][CHANGE:]
        plain, _ = run(rt, cornell, frames, g, False)
        rect, clips = run(rt, cornell, frames, g, True)
        rows[name] = {k: (mse(plain[k], truth[then], mask), mse(rect[k], truth[then], mask), float((clips[k][mask] == R.CLIPPED).mean()))
                      for k in range(1, FRAMES)}
        for k in (16, 19, 23):
            p, r, share = rows[name][k]
            print(f"{name:10s} k = {k}: plain {p:.5f}, rectified {r:.5f} ({r / p:.3f}), clipped share {share:.3f}")
        if name == "dimmed":
            print(f"{name:10s} k = 16: a single frame {mse(frames[16], truth[then], mask):.5f}")
    assert rows["dimmed"][16][2] >= 0.05
    assert max(rows["still"][k][2] for k in (16, 19, 23)) <= 0.10
    for k in (16, 23):
        assert rows["dimmed"][k][1] <= 0.5 * rows["dimmed"][k][0], k
    for k in (16, 19, 23):
        assert rows["still"][k][1] <= 1.25 * rows["still"][k][0], k
