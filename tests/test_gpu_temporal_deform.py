"""rt_temporal_accumulate_deforming (include/rt_abi.h; csrc/rt_temporal.hip: rt_temporal_deform_kernel) against
rt_temporal_accumulate_deforming_host, bit for bit: the synthetic frames of the CPU tests through the host-memory path, a
table without a deformed record against rt_temporal_accumulate_moving, and a scene made with rt_scene_add_mesh_data -- a
sheet of 8 x 8 quads with smooth normals over a floor, with one sphere -- before and after its vertices ripple
(refit_triangles).  The device path (torch tensors, in place, a NULL colour) runs in a process of its own:
tests/_temporal_deform_device_path.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _temporal_deform_reference as D
import _temporal_reference as R
from ray_tracer_2_amd import _abi as A

pytestmark = pytest.mark.gpu

F32 = np.float32
NAMES = ("out", "out_history", "motion")
CHANNELS = ("point", "normal", "object", "primitive", "bary", "flags", "albedo")
W, H, K = 96, 64, 3
SHEET = 1            # the sheet's mesh index: its object word
MARK = F32(-7.25)


def _same(got, want, what):
    assert len(got) == len(want), what
    for a, b, name in zip(got, want, NAMES):
        bad = ~R.same_bits(a, b)
        assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def _both(rt, t, planes, cam, motions, tris, first, what, **kw):
    """The device (host-memory path) against the host; returns the device's outputs."""
    g, pg = D.split(planes)
    args = (g, pg, cam, planes["prev_color"], planes["prev_history"], planes["color"])
    want = rt.temporal_accumulate_host(*args, motions=motions, prev_triangles=tris, tri_first=first, **kw)
    got = t.temporal_accumulate(*args, motions=motions, prev_triangles=tris, tri_first=first, **kw)
    _same(got, want, what)
    return got


@pytest.fixture(scope="module")
def t(rt):
    tr = rt.RayTracer(device=0, max_width=W, max_height=H)
    yield tr
    tr.close()


@pytest.mark.parametrize("size", [(37, 19), (70, 21)])
def test_synthetic_frames_equal_the_host(rt, t, size):
    """37x19: partial tiles on both axes; 70x21: three tile columns, the last partial.  Staged from host memory."""
    planes, cam, motions, tris, notes = D.synthetic_case(*size)
    for objects, motion, cap in ((True, True, 4.0), (False, True, np.inf), (True, False, np.inf)):
        p = planes if objects else {k: v for k, v in planes.items() if k != "prev_object"}
        got = _both(rt, t, p, cam, motions, tris, D.TRI_FIRST, (size, objects, motion, cap), max_history=cap, motion=motion)
    for k in ("below_range", "past_range", "degenerate", "nan_bary", "inf_bary", "past_table"):
        assert got[1][notes[k]] == 1, k
    deformed = planes["object"] >= 2
    assert (got[1][deformed] > 1).mean() > 0.4
    # out = color
    want = rt.temporal_accumulate_host(*D.split(planes), cam, planes["prev_color"], planes["prev_history"], planes["color"], 4.0,
                                       motions=motions, prev_triangles=tris, tri_first=D.TRI_FIRST)
    buf, hist = planes["color"].copy(), np.zeros(planes["object"].shape, F32)
    got = t.temporal_accumulate(*D.split(dict(planes, color=buf)), cam, planes["prev_color"], planes["prev_history"], buf, 4.0, out=buf,
                                out_history=hist, motions=motions, prev_triangles=tris, tri_first=D.TRI_FIRST)
    assert got[0] is buf and got[1] is hist
    _same(got, want, (size, "out is color"))


def test_without_a_deformed_record_it_is_the_moving_call(rt, t):
    """Consequence (a) on the device: the deformed records turned into rigid ones, the three planes and the triangles filled
    with noise -- rt_temporal_accumulate_moving's planes bit for bit."""
    planes, cam, motions, tris, _ = D.synthetic_case(70, 21)
    table = motions.copy()
    table["moved"][2], table["moved"][3] = 1, 3
    rng = np.random.default_rng(3)
    junk = tris.copy()
    junk.view(np.uint32)[:] = rng.integers(0, 1 << 32, junk.view(np.uint32).shape, dtype=np.uint64).astype(np.uint32)
    noise = dict(planes, primitive=rng.integers(0, 1 << 32, planes["primitive"].shape, dtype=np.uint64).astype(np.uint32),
                 bary=np.full(planes["bary"].shape, np.nan, F32), flags=rng.integers(0, 256, planes["flags"].shape).astype(np.uint8))
    g, pg = D.split(planes)
    moving = t.temporal_accumulate({k: g[k] for k in ("point", "normal", "object")}, pg, cam, planes["prev_color"], planes["prev_history"],
                                   planes["color"], 4.0, motion=True, motions=table)
    for p, tr in ((planes, tris), (noise, junk)):
        got = t.temporal_accumulate(*D.split(p), cam, planes["prev_color"], planes["prev_history"], planes["color"], 4.0, motion=True,
                                    motions=table, prev_triangles=tr, tri_first=D.TRI_FIRST)
        _same(got, moving, "no deformed record")
    assert (moving[1] > 1).mean() > 0.3


@pytest.fixture(scope="module")
def sheet(rt, t):
    """The scene on the handle, its arrays, and the flat frame: the G-buffer, the image after frames 0 .. K - 1 (K frames
    accumulated) and after frame K, and the raw sample of seed K."""
    sc = D.sheet_scene(rt, W, H)
    arrays = rt.SceneArrays.from_scene(sc)
    t.load_scene(arrays)
    par = lambda f: rt.make_params(W, H, 3, 2, skybox=1, frames=f)   # noqa: E731
    g = t.render_gbuffer(rt.make_params(W, H, 1, 1), CHANNELS)
    for f in range(K):
        t.render(par(f))
    prev_color = t.read_image(W, H).copy()
    t.render(par(K))
    after = t.read_image(W, H).copy()
    t.render(par(-K))
    raw = t.read_image(W, H).copy()
    first = int(arrays.meshes["triangle_offset"][SHEET])
    n = int(arrays.meshes["triangles"][SHEET])
    assert n == 2 * D.SHEET_N * D.SHEET_N
    yield dict(scene=sc, arrays=arrays, g=g, prev_color=prev_color, after=after, raw=raw, first=first, n=n,
               cam=arrays.uniform.camera)
    sc.close()


def test_unchanged_triangles_are_the_renderers_accumulation(rt, t, sheet):
    """Consequence (b): prev_triangles = the uploaded triangles of the sheet (in triangle_order: the scene's own packed
    array), the sheet marked deformed, an unmoved camera, the same G-buffer on both sides, prev_color the image after frames
    0 .. K - 1 (history K = 3) and color the raw sample of seed K: `out` is the image after frame K bit for bit on every hit
    texel, out_history K + 1 and motion exactly (0, 0) there."""
    a, g = sheet["arrays"], sheet["g"]
    tris = a.triangles[sheet["first"]:sheet["first"] + sheet["n"]]
    assert tris.tobytes() == D.packed_sheet(sheet["scene"], D.sheet_vertices()).tobytes()       # the packing the tests use below
    motions = rt.object_motions(a, a, deformed=[SHEET])
    assert motions["moved"].tolist() == [0, 2, 0]
    planes = dict(g, color=sheet["raw"], prev_color=sheet["prev_color"], prev_history=np.full((H, W), K, F32),
                  prev_point=g["point"], prev_normal=g["normal"], prev_object=g["object"])
    out, hist, motion = _both(rt, t, planes, sheet["cam"], motions, tris, sheet["first"], "unchanged triangles", motion=True)
    hit = g["object"] != A.MISS
    on = g["object"] == SHEET
    assert on.mean() > 0.2 and (g["object"] == 0).any() and (g["object"] == 2).any() and not hit.all()
    assert R.same_bits(out[hit], sheet["after"][hit]).all()
    assert (hist[hit] == K + 1).all() and np.array_equal(motion[hit], np.zeros_like(motion[hit]))
    assert R.same_bits(out[~hit], sheet["raw"][~hit]).all() and (hist[~hit] == 1).all()
    plain = t.temporal_accumulate({k: g[k] for k in ("point", "normal", "object")}, {k: g[k] for k in ("point", "normal", "object")},
                                  sheet["cam"], sheet["prev_color"], planes["prev_history"], sheet["raw"], motion=True)
    _same((out, hist, motion), plain, "rt_temporal_accumulate")


def _interior(g, pg, motion):
    """The texels of the sheet whose four taps (from the call's own motion) lie in the frame on the sheet's previous texels."""
    yy, xx = np.mgrid[0:H, 0:W]
    ok = (g["object"] == SHEET) & ~np.isnan(motion).any(-1)
    px, py = xx + np.nan_to_num(motion[..., 0]), yy + np.nan_to_num(motion[..., 1])
    x0, y0 = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    for dx in (0, 1):
        for dy in (0, 1):
            qx, qy = x0 + dx, y0 + dy
            inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            ok &= inside & (pg["object"][np.clip(qy, 0, H - 1), np.clip(qx, 0, W - 1)] == SHEET)
    return ok


def test_a_rippling_sheet_keeps_its_history(rt, t, sheet):
    """The flat sheet's vertices ripple (y += RIPPLE sin(3 x + 0.7) cos(2.5 z), analytic normals), refit_triangles sends them,
    and a new G-buffer and raw sample of seed K are taken; the camera stands.  The device's planes are the host's bit for
    bit.  On the interior set -- sheet texels whose four taps' prev_object are all the sheet -- the new call leaves
    out_history == K + 1 exactly on at least 0.9, and rt_temporal_accumulate_moving with the rigid table (nothing moved
    rigidly: every record still) keeps history on at most half as many texels: the ripple lifts most of the sheet further off
    its old tangent plane than point_tolerance x depth allows (RIPPLE 0.2 against 0.01 x a depth of 2.2 .. 4.1).  The
    amplitude was chosen on the host restatement alone, over a float64 ray cast of this scene: it gives 0.96 and 0.26 (at
    0.1: 0.96 and 0.47; the texels short of 0.96 keep their history too, at K + 1 less one ulp of the weights' rounding).  Every texel off the sheet has the moving call's bits.
    Measured on an MI355X: 1503 interior texels of the sheet's 1563; history K + 1 on 0.963 of them; the moving call keeps
    history on 0.261 as many; mean |motion| 0.98 texel."""
    a, sc = sheet["arrays"], sheet["scene"]
    pg = sheet["g"]
    first, n = sheet["first"], sheet["n"]
    prev_tris = a.triangles[first:first + n].copy()
    rippled = D.packed_sheet(sc, D.sheet_vertices(phase=0.7))
    try:
        t.refit_triangles(rippled, first)
        g = t.render_gbuffer(rt.make_params(W, H, 1, 1), CHANNELS)
        t.render(rt.make_params(W, H, 3, 2, skybox=1, frames=-K))
        raw = t.read_image(W, H).copy()
    finally:
        t.refit_triangles(prev_tris, first)
    planes = dict(g, color=raw, prev_color=sheet["prev_color"], prev_history=np.full((H, W), K, F32), prev_point=pg["point"],
                  prev_normal=pg["normal"], prev_object=pg["object"])
    motions = rt.object_motions(a, a, deformed=[SHEET])
    out, hist, motion = _both(rt, t, planes, sheet["cam"], motions, prev_tris, first, "rippled", motion=True)
    rigid = rt.object_motions(a, a)
    assert not rigid["moved"].any()
    gg, pgg = D.split(planes)
    moving = t.temporal_accumulate({k: gg[k] for k in ("point", "normal", "object")}, pgg, sheet["cam"], planes["prev_color"],
                                   planes["prev_history"], raw, motion=True, motions=rigid)
    inner = _interior(g, pg, motion)
    carried = float((hist[inner] == K + 1).mean())
    restarted = float((moving[1][inner] > 1).sum() / max(int((hist[inner] == K + 1).sum()), 1))
    size = float(np.linalg.norm(motion[inner], axis=-1).mean())
    print(f"interior {int(inner.sum())} of {int((g['object'] == SHEET).sum())} sheet texels; history {K + 1} on {carried:.3f} of them with the "
          f"previous triangles; the moving call keeps history on {restarted:.3f} as many; mean |motion| {size:.2f} texels")
    assert inner.sum() > 0.2 * W * H
    assert carried >= 0.9
    assert restarted <= 0.5
    off = g["object"] != SHEET
    for x, y, name in zip((out, hist, motion), moving, NAMES):
        assert R.same_bits(x, y)[off].all(), name
    # the luminance moments as color / prev_color with the same arguments: what denoise_variance takes for a deforming object
    m_prev = t.luminance_moments(pg, sheet["prev_color"])
    m_now = t.luminance_moments(g, raw)
    got = _both(rt, t, dict(planes, color=m_now, prev_color=m_prev), sheet["cam"], motions, prev_tris, first, "moments", motion=True)
    assert R.same_bits(got[1], hist).all() and R.same_bits(got[2], motion).all()


def _raw_call(t, p, call_flags=A.TEMPORAL_HOST_MEMORY, **over):
    cam = A.CameraUniform()
    for i in range(4):
        cam.cam_to_world[i][i] = 1.0
    cam.view_params[:] = (1.2, 0.8, 1.5)
    h, w = p["object"].shape
    d = A.TemporalDeformDesc(struct_bytes=C.sizeof(A.TemporalDeformDesc), width=w, height=h, prev_camera=cam, max_history=8.0,
                             point_tolerance=0.01, normal_cos=0.9, n_objects=len(p["motions"]), tri_first=3,
                             n_prev_triangles=len(p["prev_triangles"]))
    for k, v in p.items():
        setattr(d, k, v.ctypes.data)
    for k, v in over.items():
        setattr(d, k, v)
    return t._L.rt_temporal_accumulate_deforming(t._h, C.byref(d), call_flags)


def test_errors_and_the_staging_cap(rt):
    """The triangle side's argument errors on the device entry point, the alignment rules among them (host arrays' addresses
    stand in for device pointers: the checks come before any use), with the outputs as they were; and the previous triangles
    are counted against max_device_mb."""
    import test_temporal_deform_abi as T
    tr = rt.RayTracer(device=0, max_width=16, max_height=16)
    L, h = tr._L, tr._h
    err = lambda: L.rt_last_error(h).decode()   # noqa: E731
    try:
        p = T._planes()
        aligned = {}
        for k, v in p.items():
            raw = np.zeros(v.nbytes + 16, np.uint8)
            off = (-raw.ctypes.data) % 16
            raw[off:off + v.nbytes] = v.view(np.uint8).ravel()
            aligned[k] = raw[off:off + v.nbytes]
        ptr = {k: v.ctypes.data for k, v in aligned.items()}
        assert L.rt_temporal_accumulate_deforming(None, None, 1) == -1
        assert L.rt_temporal_accumulate_deforming(h, None, 1) == -1 and "null" in err()
        assert _raw_call(tr, p, call_flags=2) == -1 and "flags" in err()
        for over, text in ((dict(struct_bytes=224), "struct_bytes"), (dict(primitive=None), "primitive"), (dict(bary=None), "bary"),
                           (dict(flags=None), "flags"), (dict(prev_triangles=None), "prev_triangles"), (dict(n_prev_triangles=0), "n_prev_triangles"),
                           (dict(tri_first=0xFFFFFFFF, n_prev_triangles=2), "2^32"), (dict(motions=None), "motions"), (dict(object=None), "object"),
                           (dict(_p1=1), "_p1"), (dict(width=0), "zero")):
            for flags in (0, 1):
                assert _raw_call(tr, p, call_flags=flags, **dict(ptr if flags == 0 else {}, **over)) == -1 and text in err(), (over, flags, err())
        need = {"primitive": 4, "bary": 4, "flags": 1, "prev_triangles": 16, "motions": 16}
        for c, al in need.items():
            for off in (1, 2, 4, 8):
                if off % al:
                    assert _raw_call(tr, p, call_flags=0, **dict(ptr, **{c: ptr[c] + off})) == -1 and f"plane {c} " in err() and "aligned" in err(), (c, off, err())
        assert T._untouched(p)
        assert _raw_call(tr, p) == 0 and np.all(p["out_history"] > 1)
        # 3 MiB of previous triangles beside 104 + 13 bytes per texel of planes (512 x 256: 14.6 MiB)
        big = 512, 256
        q = {k: (np.ascontiguousarray(np.broadcast_to(v[:1, :1], big[::-1] + v.shape[2:])) if k not in ("motions", "prev_triangles") else v)
             for k, v in p.items()}
        q["prev_triangles"] = np.zeros(32768, A.TRI_DTYPE)
        q["prev_triangles"][:2] = p["prev_triangles"]
        for k in ("out", "out_history", "motion"):
            q[k][:] = MARK
        before = tr.last_launch()["device_mb_held"]
        tr.set_option("max_device_mb", before + 16)
        assert _raw_call(tr, q) == -8 and "max_device_mb" in err()
        assert np.all(q["out_history"] == MARK)
        assert _raw_call(tr, dict(q, prev_triangles=q["prev_triangles"][:2])) == 0
        tr.set_option("max_device_mb", before + 19)
        q["out_history"][:] = MARK
        assert _raw_call(tr, q) == 0 and np.all(q["out_history"] > 1)
        assert tr.last_launch()["device_mb_held"] == before
    finally:
        tr.close()


def test_device_path():
    """Torch tensors on the device (tests/_temporal_deform_device_path.py, a process of its own that imports torch first)."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "_temporal_deform_device_path.py")],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "device path ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
