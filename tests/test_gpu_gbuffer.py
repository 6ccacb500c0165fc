"""Whole-frame first-hit buffers (include/rt_abi.h: rt_render_gbuffer; rt_queries.inl: rt_gbuffer_kernel), pinned bit for bit
to three things that exist without it: the oracle (its debug views, which generate the rays themselves, and
oracle.intersect on the frame's own directions), the merged ray queries (rt_intersect_rays where normalising a direction
again leaves its bits alone, rt_pick on a sample everywhere) and the uploaded triangles and materials.  Then: channel
subsets, the host path in row bands, the device path (tests/_gbuffer_device_path.py), side effects, edits, errors."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _query_helpers as QH
import _ray_families as RF
from conftest import GOLDEN
from oracle import independent_f64 as F
from ray_tracer_2_amd import _abi as A
from ray_tracer_2_amd.ray_tracer import normalize3_f32

pytestmark = pytest.mark.gpu

F32 = np.float32
ALL = tuple(A.GBUFFER_CHANNELS)
CONFIGS = [{}, {"lds_scene": 0}, {"tlas": 0}, {"forest": 0, "flat2": 0}]   # test_gpu_ray_query.CONFIGS
DEFAULTS = {"lds_scene": 1, "forest": 1, "flat2": 1, "tlas": 1}
SIZES = [(24, 16), (67, 45)]
SMALL = [(8, 1), (1, 8), (1, 1)]
MIN_HIT_SHARE = 0.10


def _set(t, opts):
    for k, v in {**DEFAULTS, **opts}.items():
        t.set_option(k, v)


def look_at_bounds(arrays):
    """A camera that sees the scene: from outside its bounds along (0.45, 0.35, -0.82), written into the SceneUniform so
    that the oracle and the handle get the same one."""
    lo, hi = RF._bounds(arrays)
    c, r = 0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo))
    f = np.array([0.45, 0.35, -0.82])
    f /= np.linalg.norm(f)
    right = np.cross([0.0, 1.0, 0.0], f)
    right /= np.linalg.norm(right)
    up = np.cross(f, right)
    cam = arrays.uniform.camera
    for col, v in enumerate((right, up, f, c - 2.0 * r * f)):
        for row in range(3):
            cam.cam_to_world[col][row] = float(v[row])
        cam.cam_to_world[col][3] = 1.0 if col == 3 else 0.0
    cam.view_params[:] = [0.5, 0.5, 1.0]
    return arrays


def scene(rt, name):
    if name == "texture_test":
        return rt.SceneArrays.load(os.path.join(GOLDEN, "texture_test_scene.npz"))
    if name == "sponza_hetero":
        from ray_tracer_2_amd import scenes
        return rt.SceneArrays.from_scene(scenes.sponza_hetero())
    a = RF.scene(rt, name)
    return look_at_bounds(a) if name in RF.BUILT else a


def cam_origin(arrays):
    return np.asarray(arrays.uniform.camera.cam_to_world, F32)[3, :3].copy()


def as_hits(g):
    """The planes of a G-buffer with every rt_hit channel as rt_hit records, texel by texel in row-major order."""
    n = g["depth"].size
    h = np.zeros(n, A.HIT_DTYPE)
    h["t"] = g["depth"].ravel()
    h["object"], h["primitive"], h["flags"] = g["object"].ravel(), g["primitive"].ravel(), g["flags"].ravel()
    h["point"], h["normal"] = g["point"].reshape(n, 3), g["normal"].reshape(n, 3)
    h["bary_u"], h["bary_v"] = g["bary"].reshape(n, 2).T
    h["tex_u"], h["tex_v"] = g["texcoord"].reshape(n, 2).T
    return h


def same_bits(a, b):
    """Bit for bit; a NaN equals any NaN (test_gpu_ray_query._check_words)."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def same_planes(g, ref, what, channels=None):
    for c in channels or ref.keys():
        assert g[c].dtype == ref[c].dtype and g[c].shape == ref[c].shape, (what, c)
        assert np.array_equal(g[c].view(np.uint8), ref[c].view(np.uint8)), (what, c, int((g[c] != ref[c]).sum()))


def check_pick(t, rt, p, g, texels, what):
    h = as_hits(g)
    W = p.width
    for x, y in texels:
        hit = A.Hit()
        t._check(t._L.rt_pick(t._h, C.byref(p), int(x), int(y), C.byref(hit)))
        got = h[y * W + x]
        assert bytes(hit) == got.tobytes(), (what, x, y, np.frombuffer(bytes(hit), A.HIT_DTYPE)[0], got)


def check_against_the_oracle_views(rt, oracle, arrays, g, W, H, what):
    """Item 1: the oracle renders the debug views itself, rays included."""
    views = {flag: oracle.render(rt.make_params(W, H, 1, 1, skybox=1, frames=0, debug_flag=flag, debug_scale=1), arrays)[0]
             for flag in (2, 1, 3)}
    hit = (g["flags"] & 1) != 0
    for flag in views:
        assert np.array_equal(views[flag][..., 3] == 1.0, hit), (what, flag, "hit / miss against the view's alpha")
        assert np.all(views[flag][~hit] == 0), (what, flag)
    assert np.all(same_bits(views[2][..., 0], g["depth"])[hit]), (what, "depth")
    assert np.all(np.isposinf(g["depth"][~hit])), what
    assert np.all(same_bits(views[3][..., :2], g["texcoord"])[hit]), (what, "texcoord")
    mats = np.concatenate([arrays.meshes["material"], arrays.spheres["material"]])
    plain = hit.copy()
    plain[hit] = mats["flag"][g["object"][hit]] != A.MATERIAL_TEXTURE   # (a textured material may carry a normal map)
    nrm = g["normal"] * F32(0.5) + F32(0.5)
    assert np.all(same_bits(views[1][..., :3], nrm)[plain]), (what, "normal")


def check_against_oracle_intersect(oracle, arrays, g, what):
    """Item 2: calculate_ray_collions of the oracle on the frame's own directions."""
    n = g["depth"].size
    ro = np.broadcast_to(cam_origin(arrays), (n, 3))
    want, _ = QH.filtered_probe_words(oracle.intersect(arrays, ro, g["dir"].reshape(n, 3)), np.inf)
    got = QH.hits_as_probe_words(as_hits(g))
    isf = np.zeros(12, bool)
    isf[1:10] = True
    nan = ((got & 0x7fffffff) > 0x7f800000) & ((want & 0x7fffffff) > 0x7f800000) & isf[None, :]
    bad = np.flatnonzero(((got != want) & ~nan).any(1))
    assert bad.size == 0, f"{what}: {bad.size} of {n} texels differ from oracle.intersect, first {bad[0]}: {got[bad[0]].tolist()} vs {want[bad[0]].tolist()}"


def check_triangles(arrays, g, what, point_margin):
    """Item 3 (ii): on every hit texel the checks of test_gpu_ray_query.test_triangle_index_and_barycentrics."""
    h = as_hits(g)
    nm = len(arrays.meshes)
    hit = (h["flags"] & 1) != 0
    sph = hit & (h["object"] >= nm)
    assert np.array_equal(h["primitive"][sph], h["object"][sph] - nm), what
    assert np.all(h["bary_u"][sph] == 0) and np.all(h["bary_v"][sph] == 0), what
    assert np.all(h["object"][~hit] == A.MISS) and np.all(h["primitive"][~hit] == A.MISS), what
    tri = hit & ~sph
    hh = h[tri]
    mo = arrays.meshes[hh["object"]]
    p = hh["primitive"].astype(np.int64)
    assert np.all((p >= mo["triangle_offset"]) & (p < mo["triangle_offset"].astype(np.int64) + mo["triangles"])), what
    t = arrays.triangles[hh["primitive"]]
    tu, tv = QH.tex_uv_f32(t, hh["bary_u"], hh["bary_v"])
    assert np.array_equal(tu.view(np.uint32), hh["tex_u"].view(np.uint32)), what
    assert np.array_equal(tv.view(np.uint32), hh["tex_v"].view(np.uint32)), what
    if not point_margin or not len(hh):
        return
    n = g["depth"].size
    ro = np.broadcast_to(cam_origin(arrays), (n, 3))[tri]
    nd = g["dir"].reshape(n, 3)[tri]
    u, v = hh["bary_u"].astype(np.float64), hh["bary_v"].astype(np.float64)
    w = 1.0 - u - v
    lp = w[:, None] * t["v1"] + u[:, None] * t["v2"] + v[:, None] * t["v3"]
    m2w = np.asarray(mo["model_to_world"], np.float64)
    wp = np.einsum("rk,rkj->rj", lp, m2w[:, :3, :3]) + m2w[:, 3, :3]
    amb = F.ambiguity(F.Scene(arrays), ro, nd)
    err = np.linalg.norm(wp - hh["point"].astype(np.float64), axis=1)
    scale = np.abs(wp).max(1) + np.abs(ro).max(1) + 1.0
    tol = np.maximum(np.where(np.isfinite(amb["dst_tol"]), amb["dst_tol"], 0), 1e-5 * scale)
    ok = (amb["bary"] >= 1) & (amb["det"] >= 1) & (amb["eps"] >= 1)
    assert np.all(err[ok] <= 4 * tol[ok]), (what, float((err[ok] / tol[ok]).max()))


# the float64 brute force of the point margin runs on the scenes test_triangle_index_and_barycentrics runs it on
POINT_MARGIN = ("cornell", "room", "items", "xforms", "glass", "ties", "tlas9")


@pytest.mark.parametrize("name", RF.LIBRARY + RF.BUILT)
def test_frame_equals_oracle_queries_and_pick(rt, oracle, tracer, name):
    """Items 1, 2, 3 and 5 of the issue's list for one scene: at 24x16 and 67x45 under the default options against the
    oracle (both ways), rt_intersect_rays, the triangles and rt_pick; under every other option set the same bytes; the frames of one row, one column and one texel against rt_pick."""
    arrays = scene(rt, name)
    ro = cam_origin(arrays)
    rng = np.random.default_rng(len(name) * 1000 + sum(map(ord, name)))
    try:
        _set(tracer, {})
        tracer.load_scene(arrays)
        ref = {}
        for W, H in SIZES:
            what = f"{name} {W}x{H}"
            p = rt.make_params(W, H, 1, 1)
            g = ref[(W, H)] = tracer.render_gbuffer(p, ALL)
            hit = (g["flags"] & 1) != 0
            share = float(hit.mean())
            print(f"{what}: {share:.3f} of the texels hit")
            assert share >= MIN_HIT_SHARE, (what, share)
            check_against_the_oracle_views(rt, oracle, arrays, g, W, H, what)
            check_against_oracle_intersect(oracle, arrays, g, what)
            # 3 (i): where normalising the direction again changes no bit, rt_intersect_rays traces the same ray
            d = g["dir"].reshape(-1, 3)
            mask = (normalize3_f32(d).view(np.uint32) == d.view(np.uint32)).all(1)
            print(f"{what}: normalize3 is idempotent on {mask.mean():.3f} of the directions")
            assert mask.mean() >= 1.0 / 3.0, (what, float(mask.mean()))
            q = tracer.trace_rays(np.broadcast_to(ro, d.shape), d)
            assert np.array_equal(q[mask].view(np.uint8), as_hits(g)[mask].view(np.uint8)), what
            check_triangles(arrays, g, what, point_margin=name in POINT_MARGIN)
        # 3 (iii): rt_pick itself on a seeded sample of the larger frame, at least 100 of it outside the mask, and the corners
        W, H = SIZES[1]
        p, g = rt.make_params(W, H, 1, 1), ref[SIZES[1]]
        outside = np.flatnonzero(~mask)
        assert outside.size >= 100, (name, outside.size)
        idx = np.unique(np.concatenate([rng.choice(outside, 120, replace=False), rng.choice(W * H, 420, replace=False)]))
        assert idx.size >= 500 and np.isin(idx, outside).sum() >= 100
        texels = [(int(i % W), int(i // W)) for i in idx] + [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]
        check_pick(tracer, rt, p, g, texels, f"{name} pick")
        for W, H in SMALL:   # one row, one column, one texel: against rt_pick, every texel
            p = rt.make_params(W, H, 1, 1)
            g = tracer.render_gbuffer(p, ALL)
            check_pick(tracer, rt, p, g, [(x, y) for y in range(H) for x in range(W)], f"{name} {W}x{H}")
        # every other option set (they also move scenes between the kernels of runs and of tiles): the bytes of the default
        for cfg in CONFIGS[1:]:
            _set(tracer, cfg)
            tracer.load_scene(arrays)
            for W, H in SIZES:
                same_planes(tracer.render_gbuffer(rt.make_params(W, H, 1, 1), ALL), ref[(W, H)], f"{name} {cfg} {W}x{H}")
    finally:
        _set(tracer, {})


def check_depth_against_the_oracle_view(rt, oracle, tracer, arrays, W, H):
    tracer.load_scene(arrays)
    g = tracer.render_gbuffer(rt.make_params(W, H, 1, 1), ("depth", "flags"))
    view = oracle.render(rt.make_params(W, H, 1, 1, skybox=1, frames=0, debug_flag=2, debug_scale=1), arrays)[0]
    hit = (g["flags"] & 1) != 0
    assert hit.mean() >= MIN_HIT_SHARE
    assert np.array_equal(view[..., 3] == 1.0, hit)
    assert np.all(same_bits(view[..., 0], g["depth"])[hit]) and np.all(np.isposinf(g["depth"][~hit]))


def test_full_size_frame_against_the_oracle_depth_view(rt, oracle, tracer, cornell):
    _set(tracer, {})
    check_depth_against_the_oracle_view(rt, oracle, tracer, cornell, 1920, 1080)


def test_deep_chain_frame_against_the_oracle_depth_view(rt, oracle, tracer, cornell):
    """The same comparison on the chain BVH of 36 levels with wide stacks: 36 entries x 128 dwords x 4 B x 4 waves =
    73,728 B of dynamic LDS, so the G-buffer launch opts into more than 64 KiB."""
    from _deep_chain import deep_chain_scene
    _set(tracer, {})
    tracer.set_option("stack_wide", 1)
    try:
        check_depth_against_the_oracle_view(rt, oracle, tracer, deep_chain_scene(rt, cornell, levels=36), 64, 36)
    finally:
        tracer.set_option("stack_wide", -1)


@pytest.mark.parametrize("name", ["texture_test", "sponza_hetero"])
def test_material_channels(rt, oracle, tracer, name):
    """Item 4: albedo and emission against the uploaded materials indexed by `object`, textured hits against the oracle's
    texture filter at the texel's texcoord."""
    arrays = scene(rt, name)
    mats = np.concatenate([arrays.meshes["material"], arrays.spheres["material"]])
    try:
        for cfg in ({}, {"lds_scene": 0}):
            _set(tracer, cfg)
            tracer.load_scene(arrays)
            for W, H in SIZES:
                what = f"{name} {cfg} {W}x{H}"
                g = tracer.render_gbuffer(rt.make_params(W, H, 1, 1), ("albedo", "emission", "object", "texcoord", "flags"))
                hit = (g["flags"] & 1) != 0
                assert hit.mean() >= MIN_HIT_SHARE, (what, float(hit.mean()))
                assert np.all(g["albedo"][~hit] == 0) and np.all(g["emission"][~hit] == 0), what
                m = mats[g["object"][hit]]
                em = (m["emission_color"] * m["emission_strength"][:, None]).astype(F32)   # one binary32 product per component
                assert np.all(same_bits(g["emission"][hit], em)), what
                tex = (m["flag"] == A.MATERIAL_TEXTURE) & (m["diffuse_index"] != -1)
                assert tex.sum() > 0.05 * hit.sum(), (what, int(tex.sum()))
                alb = g["albedo"][hit]
                assert np.all(same_bits(alb[~tex], m["color"][~tex])), what
                uv = g["texcoord"][hit][tex]
                want = np.zeros((int(tex.sum()), 4), F32)
                di = m["diffuse_index"][tex]
                for i in np.unique(di):
                    if 0 <= i < len(arrays.textures):   # (an index without a texture samples zeros, as the shader's dummy)
                        want[di == i] = oracle.sample_texture(arrays.textures[i], uv[di == i])
                assert np.all(same_bits(alb[tex], want)), what
    finally:
        _set(tracer, {})


def _raw(t, p, planes, flags=A.GBUFFER_HOST_MEMORY, struct_bytes=None, p0=0):
    g = A.GBuffer(struct_bytes=C.sizeof(A.GBuffer) if struct_bytes is None else struct_bytes, _p0=p0)
    for c, arr in planes.items():
        setattr(g, c, arr.ctypes.data)
    return t._L.rt_render_gbuffer(t._h, C.byref(p) if p is not None else None, C.byref(g), flags)


def _filled(W, H, channels=ALL):
    out = {}
    for c in channels:
        dt, k = A.GBUFFER_CHANNELS[c]
        n = H * W * max(k, 1)
        out[c] = np.full(n * np.dtype(dt).itemsize, 0xA5, np.uint8).view(np.dtype(dt)).reshape((H, W, k) if k else (H, W))
    return out


def _untouched(planes):
    return all(np.all(a.view(np.uint8) == 0xA5) for a in planes.values())


def test_channel_subsets(rt, tracer):
    """Item 6, first half: any subset of planes holds the bytes the full set holds in them."""
    rng = np.random.default_rng(6)
    subsets = [(c,) for c in ALL] + [tuple(rng.choice(ALL, int(k), replace=False)) for k in rng.integers(2, 9, 3)]
    try:
        for name in ("cornell", "tlas9"):   # (the kernels of runs and of tiles)
            arrays = scene(rt, name)
            for cfg in ({}, {"lds_scene": 0}):
                _set(tracer, cfg)
                tracer.load_scene(arrays)
                p = rt.make_params(67, 45, 1, 1)
                full = tracer.render_gbuffer(p, ALL)
                for s in subsets:
                    g = tracer.render_gbuffer(p, s)
                    assert tuple(g) == s
                    same_planes(g, full, f"{name} {cfg} subset {s}", s)
    finally:
        _set(tracer, {})


def test_host_path_in_row_bands(rt, tracer, cornell):
    """Item 6, second half: a cap that forces more than ten bands gives the bytes of the unbanded call; a cap at what is
    already held leaves no room for one row."""
    W, H = 1920, 1080
    _set(tracer, {})
    tracer.load_scene(cornell)
    for f in range(2):   # (something is held afterwards: the primary table)
        tracer.render(rt.make_params(W, H, 1, 1, skybox=1, frames=f))
    tracer.synchronize()
    p = rt.make_params(W, H, 1, 1)
    want = tracer.render_gbuffer(p, ALL)
    held = tracer.last_launch()["device_mb_held"]
    assert held >= 1
    try:
        tracer.set_option("max_device_mb", held + 16)   # 201 MB of planes through at most 16 MiB: more than ten bands
        same_planes(tracer.render_gbuffer(p, ALL), want, "banded")
        tracer.set_option("max_device_mb", held)        # less than one MiB left: no row of 16384 x 97 B
        wide = rt.make_params(16384, 2, 1, 1)
        planes = _filled(16384, 2)
        assert _raw(tracer, wide, planes) == -8
        assert b"max_device_mb" in tracer._L.rt_last_error(tracer._h)
        assert _untouched(planes)
    finally:
        tracer.set_option("max_device_mb", 0)
    same_planes(tracer.render_gbuffer(p, ("depth", "object")), want, "after the cap", ("depth", "object"))


def test_device_path():
    """Torch tensors on the device (tests/_gbuffer_device_path.py, a process of its own that imports torch first): the
    bytes of the host path, and a pipelined render sequence with G-buffer calls between its frames is unchanged."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "_gbuffer_device_path.py")],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "device path ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_no_side_effects(rt, tracer, cornell):
    """Item 7: the sequence of test_gpu_ray_query.test_queries_have_no_side_effects with G-buffer calls between the frames."""
    pg = rt.make_params(67, 45, 1, 1)

    def run(gbuffers, frame_ahead):
        tracer.set_option("frame_ahead", frame_ahead)
        tracer.load_scene(cornell)
        tracer.reset_timing()
        for f in range(12):
            tracer.render(rt.make_params(64, 48, 3, 2, skybox=1, frames=f))
            if gbuffers:
                tracer.render_gbuffer(pg)
                if f % 4 == 1:
                    tracer.render_gbuffer(rt.make_params(64, 48, 1, 1), ALL)
            else:
                tracer.synchronize()   # (a host-path call returns when its data is on the host: the other sequence waits too)
        img = tracer.read_image(64, 48)
        s = tracer.stats()
        return img, (s.segments, s.paths, s.node_tests, s.triangle_tests, s.frames, s.segments_reused, s.frames_speculative), \
            tuple(tracer.last_launch().values())

    try:
        _set(tracer, {})
        for fa in (-1, 8):
            a, sa, la = run(False, fa)
            b, sb, lb = run(True, fa)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), fa
            # (the automatic policy renders ahead by what it finds on the stream: only the frames asked for are schedule-free)
            assert (sa == sb) if fa > 0 else (sa[4] == sb[4]), (fa, sa, sb)
            if fa > 0:
                assert la == lb, (la, lb)
    finally:
        tracer.set_option("frame_ahead", -1)


def test_after_edits_the_next_frame_is_a_fresh_handles(rt, tracer):
    """Item 7, second half: after update_instances, refit_triangles and a new load_scene."""
    import test_gpu_refit as R
    import test_gpu_scene_edits as E
    p = rt.make_params(67, 45, 1, 1)
    fresh = rt.RayTracer(device=0, max_width=16, max_height=16)

    def check(b, what):
        fresh.load_scene(b)
        same_planes(tracer.render_gbuffer(p, ALL), fresh.render_gbuffer(p, ALL), what)

    try:
        _set(tracer, {})
        a = E.scene(rt, "cornell")
        tracer.load_scene(a)
        tracer.render_gbuffer(p, ALL)
        _, b = E.edit_pair(rt, a, "color")
        m = b.meshes.copy()
        m[len(m) // 2] = E.translated(m[len(m) // 2], (0.0625, 0.03125, -0.125))
        b = E.clone(b, meshes=m)
        tracer.update_instances(b)
        check(b, "update_instances")
        first, n = R.mesh_range(b, 0, len(b.meshes))
        new = R.moved(b, first, n, seed=4)
        tracer.refit_triangles(new, first)
        check(R.refitted(b, first, new), "refit_triangles")
        room = RF.scene(rt, "room")
        tracer.load_scene(room)
        check(room, "load_scene")
    finally:
        fresh.close()


def test_edges(rt, cornell):
    """Item 8: every error of the contract with its code and text; pre-filled planes stay as they were."""
    t = rt.RayTracer(device=0, max_width=16, max_height=16)
    L, h = t._L, t._h
    p = rt.make_params(8, 6, 1, 1)

    def err():
        return L.rt_last_error(h).decode()

    try:
        planes = _filled(8, 6)
        assert _raw(t, p, planes) == -4 and "rt_upload_scene" in err()   # no scene
        assert _raw(t, p, {}) == 0                                       # (no plane: a no-op, scene or not)
        t.load_scene(cornell)
        g = A.GBuffer(struct_bytes=C.sizeof(A.GBuffer))
        assert L.rt_render_gbuffer(None, C.byref(p), C.byref(g), 1) == -1
        assert L.rt_render_gbuffer(h, None, C.byref(g), 1) == -1 and "null" in err()
        assert L.rt_render_gbuffer(h, C.byref(p), None, 1) == -1 and "null" in err()
        assert _raw(t, p, planes, struct_bytes=C.sizeof(A.GBuffer) - 8) == -1 and "struct_bytes" in err()
        assert _raw(t, p, planes, struct_bytes=0) == -1 and "struct_bytes" in err()
        assert _raw(t, p, planes, p0=1) == -1 and "_p0" in err()
        assert _raw(t, p, planes, flags=3) == -1 and "flags" in err()
        assert _raw(t, p, planes, flags=-2) == -1 and "flags" in err()
        assert _raw(t, rt.make_params(0, 6, 1, 1), planes) == -1 and "zero" in err()
        assert _raw(t, rt.make_params(8, 0, 1, 1), planes) == -1 and "zero" in err()
        assert _raw(t, rt.make_params(1 << 16, 1 << 15, 1, 1), planes) == -2 and "2^31" in err()
        assert _raw(t, rt.make_params(0x7fffffff, 2, 1, 1), planes) == -2
        # device planes: alignment -- 4 bytes, 16 for albedo / emission, 1 for flags (host arrays' addresses stand in for
        # device pointers: the check comes before any use) -- of every plane, alone and among aligned ones
        need = {c: (16 if c in ("albedo", "emission") else 1 if c == "flags" else 4) for c in ALL}
        for c in ALL:
            for among in (False, True):
                for off in (1, 2, 4, 8):
                    g = A.GBuffer(struct_bytes=C.sizeof(A.GBuffer))
                    if among:
                        for o in ALL:
                            setattr(g, o, planes[o].ctypes.data)
                    setattr(g, c, planes[c].ctypes.data + off)
                    if off % need[c]:
                        assert L.rt_render_gbuffer(h, C.byref(p), C.byref(g), 0) == -1 and f"plane {c} " in err() and "aligned" in err(), (c, off)
                    # (an aligned offset would pass the check and hand a host address to the device: not called)
        assert all(planes[c].ctypes.data % 16 == 0 for c in ALL)
        assert _untouched(planes)
        # and the call that is right fills every plane
        assert _raw(t, p, planes) == 0
        assert not any(np.all(a.view(np.uint8) == 0xA5) for a in planes.values())
        with pytest.raises(ValueError):
            t.render_gbuffer(p, ("depth", "nope"))
    finally:
        t.close()


def test_hits_and_misses_both_occur(rt, tracer):
    """Item 5, last sentence: over all scenes of test_frame_equals_oracle_queries_and_pick both hits and misses occur,
    counted here from the flags plane of the same frames."""
    hits = misses = 0
    _set(tracer, {})
    for name in RF.LIBRARY + RF.BUILT:
        tracer.load_scene(scene(rt, name))
        for W, H in SIZES:
            f = tracer.render_gbuffer(rt.make_params(W, H, 1, 1), ("flags",))["flags"]
            hits += int((f & 1).sum())
            misses += int(((f & 1) == 0).sum())
    assert hits > 0 and misses > 0, (hits, misses)
