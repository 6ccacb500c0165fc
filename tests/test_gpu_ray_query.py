"""The public ray queries (include/rt_abi.h: rt_intersect_rays, rt_occluded_rays, rt_pick; rt_queries.inl: rt_query_kernel)
against the test library's per-ray probe (rt_test_intersect) and the oracle (oracle.intersect) bit for bit, on the ray
families of tests/_ray_families.py; the triangle index and barycentrics against the uploaded triangles; the tmax filter;
the occlusion contract; picking against the debug views; and that queries leave a render sequence untouched."""
import numpy as np
import pytest

import _query_helpers as QH
import _ray_families as RF
from oracle import independent_f64 as F
from ray_tracer_2_amd import _abi as A
from ray_tracer_2_amd.ray_tracer import normalize3_f32

pytestmark = pytest.mark.gpu

N_RANDOM = 20000
CONFIGS = [{}, {"lds_scene": 0}, {"tlas": 0}, {"forest": 0, "flat2": 0}]
DEFAULTS = {"lds_scene": 1, "forest": 1, "flat2": 1, "tlas": 1}
F32 = np.float32


@pytest.fixture(scope="module")
def probe(rt):
    t = rt.RayTracer(device=0, max_width=64, max_height=64, lib=rt.load_test())
    yield t
    t.close()


def _set(t, opts):
    for k, v in {**DEFAULTS, **opts}.items():
        t.set_option(k, v)


def _rays(arrays, name):
    fams = RF.families(arrays, name, n_random=N_RANDOM)
    ro = np.concatenate([v[0] for v in fams.values()])
    rd = np.concatenate([v[1] for v in fams.values()])
    # the query normalises what it is given with the kernels' normalize3; give it directions normalize3 has made once,
    # so that the probe (which normalises what IT is given) and the oracle trace the same bits
    return ro, normalize3_f32(rd)


def _check_words(got, want, what):
    # a NaN float equals any NaN (test_gpu_intersect.same_bits)
    isf = np.zeros(12, bool)
    isf[1:10] = True
    nan = ((got & 0x7fffffff) > 0x7f800000) & ((want & 0x7fffffff) > 0x7f800000) & isf[None, :]
    bad = np.flatnonzero(((got != want) & ~nan).any(1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(got)} differ, first {bad[0]}: {got[bad[0]].tolist()} vs {want[bad[0]].tolist()}"


def test_device_path():
    """Tensors on the device (tests/_query_device_path.py, a process of its own that imports torch first): the same
    records as the host path, and a pipelined render sequence with device queries between its frames is unchanged."""
    import os
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "_query_device_path.py")],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "device path ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("name", RF.LIBRARY + RF.BUILT)
def test_closest_hit_equals_probe_and_oracle(rt, oracle, probe, name):
    arrays = RF.scene(rt, name)
    ro, nd = _rays(arrays, name)
    want_o, _ = QH.filtered_probe_words(oracle.intersect(arrays, ro, normalize3_f32(nd)), np.inf)
    nm = len(arrays.meshes)
    try:
        for cfg in CONFIGS:
            _set(probe, cfg)
            probe.load_scene(arrays)
            want_p, _ = QH.filtered_probe_words(probe.intersect(ro, nd), np.inf)
            _check_words(want_p, want_o, f"{name} {cfg} probe vs oracle")
            host = probe.trace_rays(ro, nd)
            _check_words(QH.hits_as_probe_words(host), want_p, f"{name} {cfg} host path")
            for n in (1, 63, 65):   # odd counts: partial waves, fewer workgroups than the grid
                part = probe.trace_rays(ro[:n], nd[:n])
                assert np.array_equal(part.view(np.uint8), host[:n].view(np.uint8)), (name, cfg, n)
            # primitive: the sphere index for spheres, a triangle of the winning mesh for meshes
            hit = (host["flags"] & 1) != 0
            sph = hit & (host["object"] >= nm)
            assert np.array_equal(host["primitive"][sph], host["object"][sph] - nm)
            tri = hit & ~sph
            mo = arrays.meshes[host["object"][tri]]
            p = host["primitive"][tri].astype(np.int64)
            assert np.all((p >= mo["triangle_offset"]) & (p < mo["triangle_offset"] + mo["triangles"]))
            assert np.all(host["object"][~hit] == 0xFFFFFFFF) and np.all(np.isposinf(host["t"][~hit]))
    finally:
        _set(probe, {})


@pytest.mark.parametrize("name", ["cornell", "room", "items", "xforms", "glass", "ties", "tlas9"])
def test_triangle_index_and_barycentrics(rt, tracer, name):
    arrays = RF.scene(rt, name)
    ro, nd = _rays(arrays, name)
    tracer.load_scene(arrays)
    h = tracer.trace_rays(ro, nd)
    nm = len(arrays.meshes)
    tri = ((h["flags"] & 1) != 0) & (h["object"] < nm)
    assert tri.sum() > 100
    hh = h[tri]
    t = arrays.triangles[hh["primitive"]]
    tu, tv = QH.tex_uv_f32(t, hh["bary_u"], hh["bary_v"])
    assert np.array_equal(tu.view(np.uint32), hh["tex_u"].view(np.uint32)), name
    assert np.array_equal(tv.view(np.uint32), hh["tex_v"].view(np.uint32)), name
    # the float64 point of the barycentrics, against the reported point within the float32 margin
    u, v = hh["bary_u"].astype(np.float64), hh["bary_v"].astype(np.float64)
    w = 1.0 - u - v
    lp = w[:, None] * t["v1"] + u[:, None] * t["v2"] + v[:, None] * t["v3"]
    m2w = np.asarray(arrays.meshes[hh["object"]]["model_to_world"], np.float64)
    wp = np.einsum("rk,rkj->rj", lp, m2w[:, :3, :3]) + m2w[:, 3, :3]
    amb = F.ambiguity(F.Scene(arrays), ro[tri], nd[tri])
    err = np.linalg.norm(wp - hh["point"].astype(np.float64), axis=1)
    scale = np.abs(wp).max(1) + np.abs(ro[tri]).max(1) + 1.0
    tol = np.maximum(np.where(np.isfinite(amb["dst_tol"]), amb["dst_tol"], 0), 1e-5 * scale)
    # (rays whose triangle decisions may flip in float32 -- barycentric, det and EPSILON margins below 1 -- have no such
    # bound on t; equal-distance ties between primitives, the `gap` margin, do not move the point)
    ok = (amb["bary"] >= 1) & (amb["det"] >= 1) & (amb["eps"] >= 1)
    assert ok.mean() > 0.5, (name, float(ok.mean()))
    assert np.all(err[ok] <= 4 * tol[ok]), (name, float((err[ok] / tol[ok]).max()))


def _tmax_sets(closest, rng):
    c = np.where(np.isfinite(closest), closest, 1.0).astype(F32)
    return {"below": (c * F32(1 - 2.0 ** -10)).astype(F32), "at": c, "next": np.nextafter(c, F32(np.inf)),
            "random": rng.uniform(0.01, 2.0 * float(np.median(c)) + 0.1, len(c)).astype(F32),
            "inf": np.full(len(c), np.inf, F32)}


@pytest.mark.parametrize("name", ["cornell", "room", "items", "glass", "xforms", "ties", "tlas9", "cull17"])
def test_tmax_filter_and_occlusion(rt, tracer, name):
    arrays = RF.scene(rt, name)
    ro, nd = _rays(arrays, name)
    sel = np.random.default_rng(1).choice(len(ro), min(len(ro), 3000), replace=False)
    ro, nd = ro[sel], nd[sel]
    tracer.load_scene(arrays)
    full = tracer.trace_rays(ro, nd)
    hit = (full["flags"] & 1) != 0
    dists = QH.hit_distances_f64(arrays, ro, nd)
    rng = np.random.default_rng(2)
    for label, tm in _tmax_sets(np.where(hit, full["t"], np.inf), rng).items():
        got = tracer.trace_rays(ro, nd, tm)
        keep = hit & (full["t"] < tm)
        assert np.array_equal(got[keep].view(np.uint8), full[keep].view(np.uint8)), (name, label)
        assert np.all(got["flags"][~keep] == 0) and np.all(np.isposinf(got["t"][~keep])), (name, label)
        occ = tracer.occluded(ro, nd, tm)
        band = QH.near_band(dists, tm)
        bad = np.flatnonzero((occ != keep) & ~band)
        assert bad.size == 0, (name, label, bad[:5], occ[bad[:5]], keep[bad[:5]])
        assert band.sum() <= max(10, len(ro) // 20) or label in ("at", "next", "below"), (name, label, int(band.sum()))
        pr = tracer.occluded(ro, nd, tm, prune=True)
        print(f"{name} {label}: band {int(band.sum())}, occluded {int(occ.sum())}/{len(occ)}, "
              f"prune_tmax differs on {int((pr != occ).sum())}")


@pytest.mark.parametrize("name", ["cornell", "room", "texture_test", "deep_chain"])
def test_pick_equals_the_debug_views(rt, tracer, cornell, name):
    """"deep_chain": 36 levels with wide stacks, 73,728 B of dynamic LDS -- the launches of rt_pick's query kernel and of the
    debug views opt into more than 64 KiB."""
    import os
    from _deep_chain import deep_chain_scene
    from conftest import GOLDEN
    arrays = (rt.SceneArrays.load(os.path.join(GOLDEN, "texture_test_scene.npz")) if name == "texture_test"
              else deep_chain_scene(rt, cornell, levels=36) if name == "deep_chain" else RF.scene(rt, name))
    W, H = (64, 36) if name == "deep_chain" else (24, 16)
    tracer.set_option("stack_wide", 1 if name == "deep_chain" else -1)
    try:
        tracer.load_scene(arrays)
        _pick_against_the_debug_views(rt, tracer, arrays, name, W, H)
    finally:
        tracer.set_option("stack_wide", -1)


def _pick_against_the_debug_views(rt, tracer, arrays, name, W, H):
    views = {}
    for flag in (2, 1):
        tracer.render(rt.make_params(W, H, 1, 1, skybox=1, frames=0, debug_flag=flag, debug_scale=1))
        views[flag] = tracer.read_image(W, H)
    plain = [i for i, m in enumerate(arrays.meshes) if int(m["material"]["flag"]) != A.MATERIAL_TEXTURE]
    plain += [len(arrays.meshes) + i for i, s in enumerate(arrays.spheres) if int(s["material"]["flag"]) != A.MATERIAL_TEXTURE]
    p = rt.make_params(W, H, 1, 1, skybox=1, frames=0)
    n_hit = 0
    for y in range(H):
        for x in range(W):
            h = tracer.pick(p, x, y)
            d = views[2][y, x]
            if h is None:
                assert np.all(d == 0), (name, x, y)
                continue
            n_hit += 1
            assert F32(h["t"]).view(np.uint32) == d[0].view(np.uint32), (name, x, y, h["t"], d[0])
            if h["object"] in plain:
                nrm = np.asarray(h["normal"], F32) * F32(0.5) + F32(0.5)
                assert np.array_equal(nrm.view(np.uint32), views[1][y, x, :3].view(np.uint32)), (name, x, y)
    assert n_hit > 0
    with pytest.raises(rt.RtError) as e:
        tracer.pick(p, W, 0)
    assert e.value.code == -1


def test_queries_have_no_side_effects(rt, tracer, cornell):
    ro, nd = _rays(cornell, "cornell")
    ro, nd = ro[:5000], nd[:5000]
    p0 = rt.make_params(64, 48, 3, 2, skybox=1, frames=0)

    def run(queries, frame_ahead):
        tracer.set_option("frame_ahead", frame_ahead)
        tracer.load_scene(cornell)
        tracer.reset_timing()
        for f in range(12):
            tracer.render(rt.make_params(64, 48, 3, 2, skybox=1, frames=f))
            if queries:
                tracer.trace_rays(ro, nd)
                tracer.occluded(ro, nd, 1.0)
                if f % 4 == 1:
                    tracer.pick(p0, 3, 5)
                    tracer.occluded(ro[:100], nd[:100], 2.0, prune=True)
            else:
                # (host-path queries return when their results are on the host: a host that waits, which the automatic
                # frame_ahead policy sees -- the sequence without them waits at the same points; the device path, which
                # does not wait, is compared with no waits at all in tests/_query_device_path.py)
                tracer.synchronize()
        img = tracer.read_image(64, 48)
        s = tracer.stats()
        return img, (s.segments, s.paths, s.node_tests, s.triangle_tests, s.frames, s.segments_reused, s.frames_speculative)

    try:
        for fa in (-1, 8):
            a, sa = run(False, fa)
            b, sb = run(True, fa)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), fa
            # (the automatic policy, -1, renders ahead when a call finds the stream busy: how far is a matter of timing, with
            # or without queries -- there only the frames asked for are schedule-free; an explicit depth fixes every counter)
            assert (sa == sb) if fa > 0 else (sa[4] == sb[4]), (fa, sa, sb)
    finally:
        tracer.set_option("frame_ahead", -1)
    # a query after an upload of another scene sees the new scene
    room = RF.scene(rt, "room")
    tracer.load_scene(room)
    got = tracer.trace_rays(ro[:500], nd[:500])
    t = rt.RayTracer(device=0, max_width=16, max_height=16)
    try:
        t.load_scene(room)
        want = t.trace_rays(ro[:500], nd[:500])
    finally:
        t.close()
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))


def test_edges(rt, cornell):
    import ctypes as C
    t = rt.RayTracer(device=0, max_width=16, max_height=16)
    L, h = t._L, t._h
    try:
        one = np.zeros(1, A.RAY_DTYPE)
        out = np.zeros(1, A.HIT_DTYPE)
        occ = np.zeros(1, np.uint32)
        # no scene
        assert L.rt_intersect_rays(h, one.ctypes.data, 1, out.ctypes.data, A.QUERY_HOST_MEMORY) == -4
        assert L.rt_occluded_rays(h, one.ctypes.data, 1, occ.ctypes.data, A.QUERY_HOST_MEMORY) == -4
        assert L.rt_pick(h, C.byref(rt.make_params(8, 8, 1, 1)), 0, 0, C.byref(A.Hit())) == -4
        t.load_scene(cornell)
        # n = 0 is a no-op, even with null pointers
        assert L.rt_intersect_rays(h, None, 0, None, 0) == 0 and L.rt_occluded_rays(h, None, 0, None, 0) == 0
        assert len(t.trace_rays(np.zeros((0, 3), F32), np.zeros((0, 3), F32))) == 0
        # null pointers, unknown flags, a pick outside the frame
        assert L.rt_intersect_rays(h, None, 1, out.ctypes.data, A.QUERY_HOST_MEMORY) == -1
        assert L.rt_occluded_rays(h, one.ctypes.data, 1, None, A.QUERY_HOST_MEMORY) == -1
        assert L.rt_intersect_rays(h, one.ctypes.data, 1, out.ctypes.data, 8 | A.QUERY_HOST_MEMORY) == -1
        assert L.rt_intersect_rays(h, one.ctypes.data, 1, out.ctypes.data, A.QUERY_PRUNE_TMAX | A.QUERY_HOST_MEMORY) == -1
        assert L.rt_occluded_rays(h, one.ctypes.data, 1, occ.ctypes.data, 4 | A.QUERY_HOST_MEMORY) == -1
        assert L.rt_pick(h, C.byref(rt.make_params(8, 8, 1, 1)), 0, 8, C.byref(A.Hit())) == -1
        assert L.rt_pick(h, None, 0, 0, C.byref(A.Hit())) == -1
        assert L.rt_intersect_rays(h, one.ctypes.data, 1 << 31, out.ctypes.data, A.QUERY_HOST_MEMORY) == -2
        # invalid rays: miss records, no fault; valid rays around them unaffected
        cam = np.asarray(cornell.uniform.camera.cam_to_world, F32)[3, :3]
        r = np.zeros(8, A.RAY_DTYPE)
        r["origin"] = cam
        r["dir"] = [0, 0, -1]
        r["dir"][1] = [0, 0, 1]
        r["tmax"] = np.inf
        r["origin"][2] = [np.nan, 0, 0]
        r["dir"][3] = [0, 0, 0]
        r["dir"][4] = [np.inf, 0, 1]
        r["tmax"][5] = 0.0
        r["tmax"][6] = np.nan
        r["_p0"][7] = 1
        hits = np.zeros(8, A.HIT_DTYPE)
        assert L.rt_intersect_rays(h, r.ctypes.data, 8, hits.ctypes.data, A.QUERY_HOST_MEMORY) == 0
        o8 = np.ones(8, np.uint32)
        assert L.rt_occluded_rays(h, r.ctypes.data, 8, o8.ctypes.data, A.QUERY_HOST_MEMORY) == 0
        assert np.all(hits["flags"][2:] == 0) and np.all(hits["object"][2:] == 0xFFFFFFFF) and np.all(o8[2:] == 0)
        assert hits["flags"][0] & 1 or hits["flags"][1] & 1   # (the camera looks into the box one way or the other)
        # a host-path call under a tight max_device_mb: chunks, or RT_ERR_OUT_OF_MEMORY
        ro, nd = _rays(cornell, "cornell")
        want = t.trace_rays(ro, nd)
        t.set_option("max_device_mb", 1)
        try:
            try:
                got = t.trace_rays(ro, nd)
                assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
            except rt.RtError as e:
                assert e.code == -8
        finally:
            t.set_option("max_device_mb", 0)
    finally:
        t.close()
