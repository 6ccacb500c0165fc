"""Radiance queries (include/rt_abi.h: rt_radiance_rays; rt_queries.inl: rt_radiance_kernel; RayTracer.radiance) against the
CPU oracle, bit for bit: the rays of seeded pinhole cameras inside the scenes -- the `dir` plane of render_gbuffer, the
camera's origin, pixel_seeds -- must get the texels oracle.render writes for those cameras (tests/_radiance_cases.py).  The
yardstick is always the oracle, never another call of the library; a NaN equals any NaN, all four channels count."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _radiance_cases as RC
from ray_tracer_2_amd import _abi as A

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def T(rt):
    t = rt.RayTracer(device=0, max_width=64, max_height=48)
    yield t
    t.close()


_refs = {}


def cornell_case(rt, oracle, T, cornell):
    """Case 1 on cornell at (4 spp, 4 bounces, skybox 1): the shuffled batch of the 12 cameras' rays and the oracle's frames
    in the batch's order -- computed once, shared and left unchanged."""
    if "cornell" not in _refs:
        cams = RC.cameras(cornell)
        RC.set_options(T, {})
        T.load_scene(cornell)
        o, d, s, perm = RC.camera_batch(T, rt, cams)
        want, _ = RC.oracle_frames(rt, oracle, cornell, cams, 4, 4, 1)
        for a in (o, d, s, want):
            a.setflags(write=False)
        _refs["cornell"] = (cams, o, d, s, want[perm])
    return _refs["cornell"]


# ---- 1. oracle parity on interior cameras ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", RC.SCENES)
def test_interior_cameras_equal_the_oracle(rt, oracle, T, name):
    arrays = RC.scene(rt, name)
    cams = RC.cameras(arrays)
    cams = [c for c in cams if RC.jitter_free(c, RC.W, RC.H)]   # (the jitter-sum case: none occurs with the recipe)
    assert len(cams) == RC.N_CAMERAS
    want = {}
    for spp, nb in RC.SWEEP:
        for sky in (0, 1):
            want[spp, nb, sky], segments = RC.oracle_frames(rt, oracle, arrays, cams, spp, nb, sky)
            if name in ("cornell", "glass", "room") and (spp, nb, sky) == (4, 4, 1):
                # asserted on the oracle's own output: the comparison below cannot pass on black frames or on paths of
                # one segment
                lit = float((want[spp, nb, sky][:, :3] != 0).any(1).mean())
                per_path = segments / (len(cams) * RC.W * RC.H * spp)
                print(f"{name}: non-zero share {lit:.2f}, segments per path {per_path:.2f}")
                assert lit >= 0.5 and per_path >= 1.5, (name, lit, per_path)
    try:
        batch = None
        for cfg in RC.CONFIGS:
            RC.set_options(T, cfg)
            T.load_scene(arrays)
            if batch is None:
                batch = RC.camera_batch(T, rt, cams)
            o, d, s, perm = batch
            assert len(s) == 768
            for (spp, nb, sky), ref in want.items():
                got = T.radiance(o, d, s, nb, spp, skybox=bool(sky))
                assert got.shape == (768, 4) and got.dtype == F32
                RC.assert_same(got, ref[perm], f"{name} {cfg} spp {spp} bounces {nb} skybox {sky}")
    finally:
        RC.set_options(T, {})


# ---- 2. a whole frame, and ragged sizes ------------------------------------------------------------------------------
def test_a_whole_frame_and_ragged_counts(rt, oracle, T, cornell):
    Wf, Hf = 64, 48
    RC.set_options(T, {})
    T.load_scene(cornell)
    cam = cornell.uniform.camera
    assert RC.jitter_free(cam, Wf, Hf) and cam.defocus_strength == 0.0 and cam.diverge_strength == 0.0
    o, d, s = RC.frame_rays(T, rt, cam, 0, Wf, Hf)
    want, _ = oracle.render(rt.make_params(Wf, Hf, 4, 8, skybox=1, frames=0), cornell)
    full = T.radiance(o, d, s, 4, 8)
    RC.assert_same(full, want.reshape(-1, 4), "cornell 64x48, 8 spp, 4 bounces")
    for n in (1, 63, 64, 65, 257, 3001):   # partial waves, fewer workgroups than the grid, a ragged last claim
        RC.assert_same(T.radiance(o[:n], d[:n], s[:n], 4, 8), full[:n], f"the first {n} rays")


# ---- 3. position independence ----------------------------------------------------------------------------------------
def test_a_ray_s_result_does_not_depend_on_its_place(rt, oracle, T, cornell):
    _, o, d, s, want = cornell_case(rt, oracle, T, cornell)
    RC.set_options(T, {})
    T.load_scene(cornell)
    perm = np.random.default_rng(11).permutation(len(s))
    RC.assert_same(T.radiance(o[perm], d[perm], s[perm], 4, 4), want[perm], "permuted batch")
    for i in (0, 5, 767):
        RC.assert_same(T.radiance(o[i:i + 1], d[i:i + 1], s[i:i + 1], 4, 4), want[i:i + 1], f"ray {i} alone")


# ---- 4. state independence and no side effects -----------------------------------------------------------------------
def test_the_handle_s_state_does_not_enter(rt, oracle, T, cornell):
    cams, o, d, s, want = cornell_case(rt, oracle, T, cornell)
    RC.set_options(T, {})
    T.load_scene(cornell)
    try:
        jittered = A.CameraUniform.from_buffer_copy(bytes(cams[0]))
        jittered.defocus_strength = 0.5
        T.set_camera(jittered)
        RC.assert_same(T.radiance(o, d, s, 4, 4), want, "a jittered camera on the handle")
        T.render(rt.make_params(40, 24, 2, 3, skybox=0, frames=2))
        RC.assert_same(T.radiance(o, d, s, 4, 4), want, "after an unrelated render")
        for k, v in (("vote_eighths", 8), ("pixel_cache", 0), ("primary_table", 0)):
            T.set_option(k, v)
        T.render(rt.make_params(40, 24, 2, 3, skybox=0, frames=3))
        RC.assert_same(T.radiance(o, d, s, 4, 4), want, "vote_eighths, pixel_cache, primary_table changed")
    finally:
        for k, v in (("vote_eighths", -1), ("pixel_cache", 1), ("primary_table", 1)):
            T.set_option(k, v)
        T.set_camera(cornell.uniform.camera)


def test_calls_between_frames_leave_the_sequence_alone(rt, oracle, T, cornell):
    _, o, d, s, want = cornell_case(rt, oracle, T, cornell)
    o, d, s = o[:300], d[:300], s[:300]

    def run(calls, frame_ahead):
        RC.set_options(T, {})
        T.set_option("frame_ahead", frame_ahead)
        T.load_scene(cornell)
        T.reset_timing()
        for f in range(6):
            T.render(rt.make_params(64, 48, 3, 2, skybox=1, frames=f))
            if calls:
                before = T.last_launch()
                RC.assert_same(T.radiance(o, d, s, 4, 4), want[:300], f"between frames {f} and {f + 1}")
                assert T.last_launch() == before
            else:
                T.synchronize()   # (a host-path call returns when its results are on the host: the same waits)
        img = T.read_image(64, 48)
        st = T.stats()
        return img, (st.segments, st.paths, st.node_tests, st.triangle_tests, st.frames, st.segments_reused, st.frames_speculative,
                     st.launches), T.last_launch()

    try:
        # (-1: the automatic policy and the pipelined single frames; it renders ahead when a call finds the stream busy, a
        # matter of timing with or without the calls -- there only the image and the frames asked for are schedule-free; an
        # explicit depth fixes every counter and the launch shape: tests/test_gpu_ray_query.py)
        for fa in (-1, 8):
            a, sa, la = run(False, fa)
            b, sb, lb = run(True, fa)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), fa
            assert (sa == sb and la == lb) if fa > 0 else (sa[4] == sb[4]), (fa, sa, sb, la, lb)
    finally:
        T.set_option("frame_ahead", -1)


# ---- 5. invalid rays -------------------------------------------------------------------------------------------------
def test_invalid_rays_get_zeros_and_disturb_nobody(rt, oracle, T, cornell):
    _, o, d, s, want = cornell_case(rt, oracle, T, cornell)
    RC.set_options(T, {})
    T.load_scene(cornell)
    n = 300
    rays = np.zeros(n, A.PATH_RAY_DTYPE)
    rays["origin"], rays["dir"], rays["seed"] = o[:n], d[:n], s[:n]
    bad = {3: ("origin", [np.nan, 0, 0]), 64: ("origin", [0, np.inf, 0]), 65: ("dir", [0, 0, 0]), 130: ("dir", [np.inf, 0, 1]),
           131: ("dir", [0, -np.inf, 0]), 255: ("origin", [0, 0, -np.inf]), 299: ("dir", [np.nan, 1, 0])}
    for i, (f, v) in bad.items():
        rays[f][i] = v
    rays["_p0"][200] = 1
    invalid = sorted(list(bad) + [200])
    out = np.full((n, 4), 7.0, F32)
    p = rt.make_params(0, 0, 4, 4, skybox=1)
    assert T._L.rt_radiance_rays(T._h, C.byref(p), rays.ctypes.data, n, out.ctypes.data, A.RADIANCE_HOST_MEMORY) == 0
    assert np.all(out[invalid].view(np.uint32) == 0)
    valid = np.setdiff1d(np.arange(n), invalid)
    RC.assert_same(out[valid], want[:n][valid], "the valid rays around the invalid ones")


# ---- 6. errors -------------------------------------------------------------------------------------------------------
def test_errors_write_nothing(rt, cornell):
    t = rt.RayTracer(device=0, max_width=16, max_height=16)
    L, h = t._L, t._h
    try:
        rays = np.zeros(4, A.PATH_RAY_DTYPE)
        rays["dir"] = [0, 0, -1]
        out = np.full((4, 4), 7.0, F32)
        p = rt.make_params(0, 0, 2, 2, skybox=1)
        HOST = A.RADIANCE_HOST_MEMORY

        def call(params, r, n, o, flags):
            rc = L.rt_radiance_rays(h, None if params is None else C.byref(params), r, n, o, flags)
            assert np.all(out == 7.0), "an error wrote to the output"
            return rc

        assert call(p, rays.ctypes.data, 4, out.ctypes.data, HOST) == -4                         # no scene
        t.load_scene(cornell)
        assert L.rt_radiance_rays(None, C.byref(p), rays.ctypes.data, 4, out.ctypes.data, HOST) == -1
        assert call(None, rays.ctypes.data, 4, out.ctypes.data, HOST) == -1                      # null arguments
        assert call(p, None, 4, out.ctypes.data, HOST) == -1
        assert call(p, rays.ctypes.data, 4, None, HOST) == -1
        assert call(p, rays.ctypes.data, 4, out.ctypes.data, HOST | 2) == -1                     # unknown flag
        assert call(p, rays.ctypes.data, 4, out.ctypes.data, 8) == -1
        assert call(rt.make_params(0, 0, 2, 0), rays.ctypes.data, 4, out.ctypes.data, HOST) == -1    # rays_per_pixel = 0
        assert call(rt.make_params(0, 0, -1, 2), rays.ctypes.data, 4, out.ctypes.data, HOST) == -1   # number_of_bounces = -1
        assert call(p, rays.ctypes.data, 1 << 31, out.ctypes.data, HOST) == -2                   # n = 2^31
        assert call(p, None, 0, None, 0) == 0                                                    # n = 0: a no-op
        assert t.radiance(np.zeros((0, 3), F32), np.zeros((0, 3), F32), np.zeros(0, np.uint32), 1, 1).shape == (0, 4)
        # misaligned device pointers: the addresses are checked, never read
        base = int(t.device_image_ptr)
        assert base % 16 == 0
        assert call(p, base + 4, 4, base + 1024, 0) == -1
        assert call(p, base, 4, base + 1024 + 8, 0) == -1
    finally:
        t.close()


# ---- 7. host staging in chunks ---------------------------------------------------------------------------------------
def test_host_staging_in_chunks(rt, cornell):
    t = rt.RayTracer(device=0, max_width=256, max_height=256)
    try:
        t.load_scene(cornell)
        for f in range(2):   # (something is held afterwards: the primary table, 64 B per texel)
            t.render(rt.make_params(256, 256, 1, 1, skybox=1, frames=f))
        t.synchronize()
        n = 50000
        rng = np.random.default_rng(5)
        lo, hi = RC.RF._bounds(cornell)
        o = (lo + (hi - lo) * rng.uniform(0.1, 0.9, (n, 3))).astype(F32)
        d = rng.normal(size=(n, 3)).astype(F32)
        s = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
        want = t.radiance(o, d, s, 1, 1)
        assert (want[:, :3] != 0).any()
        held = t.last_launch()["device_mb_held"]   # (MiB, rounded up)
        assert held >= 2
        try:
            t.set_option("max_device_mb", held + 1)   # between 1 and 2 MiB of room at 48 bytes per ray: 2 or 3 chunks
            got = t.radiance(o, d, s, 1, 1)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
            t.set_option("max_device_mb", held - 1)   # less than the handle holds already: not one ray fits
            out = np.full((n, 4), 7.0, F32)
            rays = np.zeros(n, A.PATH_RAY_DTYPE)
            rays["origin"], rays["dir"], rays["seed"] = o, d, s
            p = rt.make_params(0, 0, 1, 1)
            assert t._L.rt_radiance_rays(t._h, C.byref(p), rays.ctypes.data, n, out.ctypes.data, A.RADIANCE_HOST_MEMORY) == -8
            assert b"max_device_mb" in t._L.rt_last_error(t._h) and np.all(out == 7.0)
        finally:
            t.set_option("max_device_mb", 0)
        assert np.array_equal(t.radiance(o[:100], d[:100], s[:100], 1, 1).view(np.uint32), want[:100].view(np.uint32))
    finally:
        t.close()


# ---- 8. after edits --------------------------------------------------------------------------------------------------
def test_after_instance_edits_and_a_refit(rt, oracle, T):
    a = RC.scene(rt, "items")
    cams = RC.cameras(a)
    RC.set_options(T, {})
    T.load_scene(a)
    o, d, s, perm = RC.camera_batch(T, rt, cams)

    def copy(x):
        u = A.SceneUniform.from_buffer_copy(bytes(x.uniform))
        return type(x)(u, x.spheres.copy(), x.meshes.copy(), x.triangles.copy(), x.nodes.copy(), x.textures)

    b = copy(a)   # a material's colour and a transform
    b.meshes[1]["material"]["color"] = (0.9, 0.2, 0.1, 1.0)
    b.meshes[1]["material"]["emission_color"] = (1.0, 0.8, 0.6, 1.0)
    b.meshes[1]["material"]["emission_strength"] = 2.0
    b.meshes[4]["world_to_model"], b.meshes[4]["model_to_world"] = RC.RF._matrices(RC.RF.trs(pos=(0.1, 0.8, 0.2), axis=(1, 0, 1), angle=0.4))
    T.update_instances(b)
    want, _ = RC.oracle_frames(rt, oracle, b, cams, 4, 4, 1)
    RC.assert_same(T.radiance(o, d, s, 4, 4), want[perm], "after update_instances")
    m = b.meshes[2]   # then moved vertices of one mesh
    first, n = int(m["triangle_offset"]), int(m["triangles"])
    new = b.triangles[first:first + n].copy()
    rng = np.random.default_rng(3)
    for k in ("v1", "v2", "v3"):
        new[k] = (new[k] + rng.normal(0, 0.03, new[k].shape) + [0.05, -0.02, 0.04]).astype(F32)
    c = copy(b).refit_bvh(first, n, new)
    T.refit_triangles(new, first)
    want, _ = RC.oracle_frames(rt, oracle, c, cams, 4, 4, 1)
    RC.assert_same(T.radiance(o, d, s, 4, 4), want[perm], "after refit_triangles")


# ---- 9. device path --------------------------------------------------------------------------------------------------
def test_device_path():
    """Tensors on the device (tests/_radiance_device_path.py, a process of its own that imports torch first): the host
    path's bits."""
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "_radiance_device_path.py")],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "device path ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
