"""The recipe tests/test_gpu_radiance.py and tests/_radiance_device_path.py share: seeded cameras inside a scene's bounds, the
rays of their 8 x 8 frames as inputs of RayTracer.radiance, and the oracle's frames of the same cameras.

A radiance call is pinned to the oracle through the pinhole camera: with origin = cam_to_world[3], dir = texel (x, y) of
render_gbuffer's `dir` plane and seed = pixel_seeds(...)[y * width + x], ray (x, y) gets the bits oracle.render writes to
that texel for frames <= 0 under a camera without jitter (include/rt_abi.h: rt_radiance_rays)."""
import os

import numpy as np

import _ray_families as RF
from ray_tracer_2_amd import _abi as A
from ray_tracer_2_amd.ray_tracer import pixel_seeds

F32 = np.float32
W = H = 8
N_CAMERAS = 12
SCENES = ["cornell", "glass", "items", "xforms", "ties", "room", "texture_test", "tlas9", "cull16", "height33"]
SWEEP = [(1, 0), (4, 4), (3, 1)]   # (spp, bounces)
CONFIGS = [{}, {"lds_scene": 0}, {"tlas": 0}, {"forest": 0, "flat2": 0}]
DEFAULTS = {"lds_scene": 1, "forest": 1, "flat2": 1, "tlas": 1}


def scene(rt, name):
    if name == "texture_test":
        return rt.SceneArrays.load(os.path.join(RF.GOLDEN, "texture_test_scene.npz"))
    return RF.scene(rt, name)


def set_options(t, opts):
    for k, v in {**DEFAULTS, **opts}.items():
        t.set_option(k, v)


def with_camera(arrays, cam):
    """`arrays` with another camera in its SceneUniform (what the oracle renders with); the arrays are shared."""
    u = A.SceneUniform.from_buffer_copy(bytes(arrays.uniform))
    u.camera = cam
    return type(arrays)(u, arrays.spheres, arrays.meshes, arrays.triangles, arrays.nodes, arrays.textures)


def focus_points(cam, w, h):
    """focus_point_of (wgsl:479-482) of every texel in binary32, the kernels' order of operations: (h, w, 3)."""
    m = np.asarray(cam.cam_to_world, F32)   # [column][row]
    vp = np.asarray(cam.view_params, F32)
    x, y = np.meshgrid(np.arange(w, dtype=F32), np.arange(h, dtype=F32))
    lx = (x / F32(w - 1) - F32(0.5)) * vp[0]
    ly = (y / F32(h - 1) - F32(0.5)) * vp[1]
    lz = np.full_like(lx, F32(1.0) * vp[2])
    return np.stack([((m[0, r] * lx + m[1, r] * ly) + m[2, r] * lz) + m[3, r] * F32(1.0) for r in range(3)], -1).astype(F32)


def jitter_free(cam, w, h):
    """No component of the camera origin or of a texel's focus point is -0 (memo_ray_of's condition): the G-buffer's
    direction is then `frag`'s direction under zero jitter strengths."""
    neg0 = lambda v: bool(np.any((np.ascontiguousarray(v, F32).view(np.uint32) == 0x80000000)))
    return not neg0(np.asarray(cam.cam_to_world, F32)[3, :3]) and not neg0(focus_points(cam, w, h))


def cameras(arrays, n=N_CAMERAS, seed=1):
    """n seeded cameras inside the scene's bounds: origin lo + (hi - lo) * U(0.1, 0.9)^3, orientation the Q of a seeded 3 x 3
    normal matrix with determinant +1, view_params (1.2, 1.2, 1), both jitter strengths +0."""
    rng = np.random.default_rng(seed)
    lo, hi = RF._bounds(arrays)
    out = []
    for _ in range(n):
        origin = lo + (hi - lo) * rng.uniform(0.1, 0.9, 3)
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        cam = A.CameraUniform()
        for col in range(3):
            for row in range(3):
                cam.cam_to_world[col][row] = float(q[row, col])
        for row in range(3):
            cam.cam_to_world[3][row] = float(origin[row])
        cam.cam_to_world[3][3] = 1.0
        cam.view_params[:] = [1.2, 1.2, 1.0]
        cam.defocus_strength = cam.diverge_strength = 0.0
        out.append(cam)
    return out


def frame_rays(t, rt, cam, frames, w=W, h=H):
    """(origins, dirs, seeds) of the w x h frame of `cam`, row-major: the `dir` plane of render_gbuffer (a merged call, used
    only to produce inputs), the camera's origin, the frame's pixel seeds."""
    t.set_camera(cam)
    d = t.render_gbuffer(rt.make_params(w, h, 1, 1), channels=("dir",))["dir"].reshape(-1, 3)
    o = np.broadcast_to(np.asarray(cam.cam_to_world, F32)[3, :3], d.shape).copy()
    return o, d, pixel_seeds(w, h, frames)


def camera_batch(t, rt, cams, perm_seed=7):
    """The rays of all cameras' 8 x 8 frames (camera k: frames = -(k + 1)), concatenated and shuffled: (origins, dirs,
    seeds, perm) with ray j of the batch = ray perm[j] of the concatenation."""
    parts = [frame_rays(t, rt, cam, -(k + 1)) for k, cam in enumerate(cams)]
    o, d, s = (np.concatenate([p[i] for p in parts]) for i in range(3))
    perm = np.random.default_rng(perm_seed).permutation(len(s))
    return o[perm], d[perm], s[perm], perm


def oracle_frames(rt, oracle, arrays, cams, spp, bounces, skybox):
    """(the cameras' frames as (n_cameras * 64, 4) in the concatenation's order, segments traced)"""
    out, segments = [], 0
    for k, cam in enumerate(cams):
        img, st = oracle.render(rt.make_params(W, H, bounces, spp, skybox=skybox, frames=-(k + 1)), with_camera(arrays, cam))
        out.append(img.reshape(-1, 4))
        segments += int(st.segments)
    return np.concatenate(out), segments


def same_bits(a, b):
    """Bit for bit, all four channels; a NaN equals any NaN."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def assert_same(got, want, what):
    ok = same_bits(got, want).all(-1)
    bad = np.flatnonzero(~ok.ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {ok.size} rays differ, first {bad[0]}: {got.reshape(-1, 4)[bad[0]].tolist()} vs {want.reshape(-1, 4)[bad[0]].tolist()}"
