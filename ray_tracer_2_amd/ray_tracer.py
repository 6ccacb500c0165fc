"""`RayTracer`: Python face of the device-side C ABI, with the reference's
method names (src/rendering/ray_tracer.rs:48-435).

    rt = RayTracer(device=0, max_width=1920, max_height=1080)   # new + create_gpu_resources
    rt.load_scene_gpu_resources(arrays)                        # textures
    rt.update_buffers(arrays)                                  # scene arrays (on change)
    rt.render(params)                                          # one frame (async)
    img = rt.read_image(w, h)                                  # RGBA32F, row 0 = bottom

The render path is the HIP library only; nothing here computes pixels.
"""
import ctypes as C
import os

import numpy as np

from . import _abi as A
from .lib import RtError, load
from .scene import Scene, SceneArrays

# The denoiser's default widths (RayTracer.denoise, denoise_host): sigma_color in demodulated radiance (colour / albedo) --
# wide, because the fireflies of a few samples per pixel are many units away from their neighbours, and halved per pass --,
# sigma_normal in units of the difference of two unit normals, sigma_point in world units (the Cornell box is 2 across).
DENOISE_SIGMA_COLOR, DENOISE_SIGMA_NORMAL, DENOISE_SIGMA_POINT = 4.0, 0.3, 1.0


# ---- the planes of the frame passes (denoise, denoise_variance / luminance_moments, temporal_accumulate, adaptive_plan /
# adaptive_merge): one set of helpers over the tables of _abi, plane -> (numpy dtype, components per texel) ----
def _plane_shape(table, k, W, H):
    """(H, W, n), (H, W) for n = 0, or the shape itself where a call's own table names one (a plane that is not frame-shaped)."""
    n = table[k][1]
    return n if isinstance(n, tuple) else (H, W, n) if n else (H, W)


def _numpy_inputs(d, table, W, H, planes):
    """Points the desc at contiguous copies of the numpy inputs (or the arrays themselves); returns what must stay alive."""
    keep = {}
    for k, v in planes.items():
        a = np.ascontiguousarray(v, np.dtype(table[k][0]))
        if a.shape != _plane_shape(table, k, W, H):
            raise ValueError(f"plane {k} must have shape {_plane_shape(table, k, W, H)}, not {a.shape}")
        keep[k] = a
        setattr(d, k, a.ctypes.data)
    return keep


def _numpy_outputs(d, table, W, H, outs):
    """Points the desc at the numpy outputs -- outs: name -> None or False (not asked for), True (a new array) or the array to
    fill -- and returns them by name (None: not asked for)."""
    res = {}
    for k, v in outs.items():
        if v is None or v is False:
            res[k] = None
            continue
        shape, dt = _plane_shape(table, k, W, H), np.dtype(table[k][0])
        if v is True:
            v = np.zeros(shape, dt)
        elif not (isinstance(v, np.ndarray) and v.dtype == dt and v.shape == shape and v.flags.c_contiguous and v.flags.writeable):
            raise ValueError(f"{k} must be a writeable contiguous {dt} array of shape {shape}")
        res[k] = v
        setattr(d, k, v.ctypes.data)
    return res


def _tensor_planes(d, device, table, W, H, planes, outs):
    """The same for torch tensors on cuda:`device`: checks the inputs and the outputs that are given (device, dtype -- a
    uint32 plane is an int32 tensor holding the bits, or uint32; a byte plane uint8 --, layout, shape), makes the outputs asked for with True,
    points the desc at all of them and returns the outputs by name (None: not asked for)."""
    import torch
    dev = torch.device("cuda", device)
    given = dict(planes, **{k: v for k, v in outs.items() if v is not None and v is not True and v is not False})
    for k, v in given.items():
        if not isinstance(v, torch.Tensor):
            raise ValueError("mix of device tensors and host arrays")
        if v.device.type != "cuda" or v.device.index != device:
            raise ValueError(f"plane {k} must be on cuda:{device}, not {v.device}")
        kinds = ((torch.float32,) if table[k][0] == "<f4" else (torch.uint8,) if table[k][0] == "u1" else
                 (torch.int32, getattr(torch, "uint32", torch.int32)))
        if v.dtype not in kinds or not v.is_contiguous() or tuple(v.shape) != _plane_shape(table, k, W, H):
            name = str(kinds[0]).replace("torch.", "")
            raise ValueError(f"plane {k} must be a contiguous {name} tensor of shape {_plane_shape(table, k, W, H)}")
    res = {}
    for k, v in outs.items():
        if v is True:
            kind = torch.float32 if table[k][0] == "<f4" else torch.uint8 if table[k][0] == "u1" else torch.int32
            v = given[k] = torch.empty(_plane_shape(table, k, W, H), dtype=kind, device=dev)
        res[k] = None if v is None or v is False else v
    for k, v in given.items():
        setattr(d, k, v.data_ptr())
    return res


def _host_call(name, d):
    """A *_host entry point of the library on a filled desc."""
    L = load()
    rc = getattr(L, name)(C.byref(d))
    if rc < 0:
        raise RtError(rc, L.rt_last_error(None).decode())


def _host_frame_call(name, d, table, W, H, planes, outs):
    """A *_host entry point on numpy planes; returns the outputs by name."""
    keep = _numpy_inputs(d, table, W, H, planes)
    res = _numpy_outputs(d, table, W, H, outs)
    _host_call(name, d)
    del keep
    return res


def _new_or(out):
    return True if out is None else out


def _frame_size(plane):
    """(W, H) of an (H, W) or (H, W, n) plane."""
    H, W = (int(v) for v in np.shape(plane)[:2])
    return W, H


def _denoise_desc(W, H, iterations, sigma_color, sigma_normal, sigma_point):
    return A.DenoiseDesc(struct_bytes=C.sizeof(A.DenoiseDesc), width=W, height=H, iterations=int(iterations),
                         sigma_color=float(sigma_color), sigma_normal=float(sigma_normal), sigma_point=float(sigma_point))


def _denoise_inputs(guides, color):
    """The desc's input planes by name and the frame's size."""
    planes = {k: guides[k] for k in ("normal", "point", "albedo", "emission") if k in guides}
    if "normal" not in planes or "point" not in planes:
        raise ValueError("guides must hold the normal and point planes of render_gbuffer")
    if color is not None:
        planes["color"] = color
    return (planes, *_frame_size(planes["normal"]))


def denoise_host(guides, color, iterations=3, sigma_color=DENOISE_SIGMA_COLOR, sigma_normal=DENOISE_SIGMA_NORMAL,
                 sigma_point=DENOISE_SIGMA_POINT, out=None):
    """rt_denoise_host: the denoiser's definition on the CPU (no device), with RayTracer.denoise's arguments for numpy
    planes.  RayTracer.denoise computes the same bits on the GPU."""
    planes, W, H = _denoise_inputs(guides, color)
    d = _denoise_desc(W, H, iterations, sigma_color, sigma_normal, sigma_point)
    return _host_frame_call("rt_denoise_host", d, A.DENOISE_PLANES, W, H, planes, {"out": _new_or(out)})["out"]


# Temporal accumulation's default thresholds (RayTracer.temporal_accumulate, temporal_accumulate_host): a tap's hit point
# may lie 1 % of the view depth off the current texel's tangent plane -- under the Cornell camera a fifth of a texel's
# footprint at 67 x 45 and five footprints at 1920 x 1080; the distance is along the normal, so on a flat wall it is zero
# but for rounding, and what the test refuses is another surface behind or in front --, and
# the two normals may be up to acos(0.9) = 26 degrees apart.  DESIGN.md section 2.14 has what the quality test measured
# with them.
TEMPORAL_POINT_TOLERANCE, TEMPORAL_NORMAL_COS = 0.01, 0.9


def _temporal_desc(W, H, prev_camera, max_history, point_tolerance, normal_cos):
    if not isinstance(prev_camera, A.CameraUniform):
        raise ValueError("prev_camera must be a CameraUniform")
    return A.TemporalDesc(struct_bytes=C.sizeof(A.TemporalDesc), width=W, height=H,
                          prev_camera=A.CameraUniform.from_buffer_copy(bytes(prev_camera)), max_history=float(max_history),
                          point_tolerance=float(point_tolerance), normal_cos=float(normal_cos))


def _temporal_inputs(guides, prev_guides, prev_color, prev_history, color):
    """The desc's input planes by name, from the two guide dicts (render_gbuffer's; each side's `object` plane is
    optional), and the frame's size."""
    for g, what in ((guides, "guides"), (prev_guides, "prev_guides")):
        if "normal" not in g or "point" not in g:
            raise ValueError(f"{what} must hold the normal and point planes of render_gbuffer")
    planes = {"point": guides["point"], "normal": guides["normal"], "prev_color": prev_color, "prev_history": prev_history,
              "prev_point": prev_guides["point"], "prev_normal": prev_guides["normal"]}
    if "object" in guides:
        planes["object"] = guides["object"]
    if "object" in prev_guides:
        planes["prev_object"] = prev_guides["object"]
    if color is not None:
        planes["color"] = color
    return (planes, *_frame_size(planes["normal"]))


def _temporal_result(res):
    return (res["out"], res["out_history"]) if res["motion"] is None else (res["out"], res["out_history"], res["motion"])


def _temporal_call(guides, prev_guides, prev_camera, prev_color, prev_history, color, max_history, point_tolerance, normal_cos,
                   motions, prev_triangles=None, tri_first=0):
    """The entry point's name stem, its desc, its plane table, the inputs by name and the frame's size: rt_temporal_accumulate
    without a motion table, rt_temporal_accumulate_moving with one (`motions`: (n,) OBJECT_MOTION_DTYPE, or an (n, 24) int32
    tensor of the records' words), rt_temporal_accumulate_deforming with the previous triangles too (`prev_triangles`: n
    TRI_DTYPE records, or an (n, 24) float32 tensor; `guides` then holds primitive, bary and flags)."""
    planes, W, H = _temporal_inputs(guides, prev_guides, prev_color, prev_history, color)
    d = _temporal_desc(W, H, prev_camera, max_history, point_tolerance, normal_cos)
    if prev_triangles is not None and motions is None:
        raise ValueError("prev_triangles needs the motion table that marks the deformed meshes (object_motions(..., deformed=))")
    if motions is None:
        return "rt_temporal_accumulate", d, A.TEMPORAL_PLANES, planes, W, H
    if "object" not in planes:
        raise ValueError("guides must hold the object plane of render_gbuffer: the motion table is indexed by it")
    if hasattr(motions, "data_ptr"):
        if motions.dim() != 2 or motions.shape[1] != 24 or motions.shape[0] < 1:
            raise ValueError("a motion table on the device is an (n_objects, 24) int32 tensor of the records' words")
        entry = ("<u4", (int(motions.shape[0]), 24))
    else:
        motions = np.asarray(motions)
        if motions.dtype != A.OBJECT_MOTION_DTYPE or motions.ndim != 1 or motions.shape[0] < 1:
            raise ValueError("a motion table is a one-dimensional OBJECT_MOTION_DTYPE array (object_motions) with a record or more")
        entry = (A.OBJECT_MOTION_DTYPE, (int(motions.shape[0]),))
    md = A.TemporalMotionDesc.from_buffer_copy(bytes(d) + bytes(C.sizeof(A.TemporalMotionDesc) - C.sizeof(A.TemporalDesc)))
    md.struct_bytes, md.n_objects = C.sizeof(A.TemporalMotionDesc), entry[1][0]
    planes["motions"] = motions
    if prev_triangles is None:
        return "rt_temporal_accumulate_moving", md, dict(A.TEMPORAL_MOTION_PLANES, motions=entry), planes, W, H
    for k in ("primitive", "bary", "flags"):
        if k not in guides:
            raise ValueError(f"guides must hold the {k} plane of render_gbuffer: a deformed texel's previous triangle is named by it")
        planes[k] = guides[k]
    if hasattr(prev_triangles, "data_ptr"):
        if prev_triangles.dim() != 2 or prev_triangles.shape[1] != 24 or prev_triangles.shape[0] < 1:
            raise ValueError("previous triangles on the device are an (n, 24) float32 tensor, as refit_triangles takes them")
        tri_entry = ("<f4", (int(prev_triangles.shape[0]), 24))
    else:
        prev_triangles = np.ascontiguousarray(prev_triangles)
        if prev_triangles.dtype != A.TRI_DTYPE or prev_triangles.ndim != 1 or prev_triangles.shape[0] < 1:
            raise ValueError("previous triangles are a one-dimensional TRI_DTYPE array with a record or more")
        tri_entry = (A.TRI_DTYPE, (int(prev_triangles.shape[0]),))
    tri_first = int(tri_first)
    if tri_first < 0 or tri_first + tri_entry[1][0] > 1 << 32:
        raise ValueError("tri_first must be >= 0 and tri_first + the number of previous triangles at most 2^32")
    dd = A.TemporalDeformDesc.from_buffer_copy(bytes(md) + bytes(C.sizeof(A.TemporalDeformDesc) - C.sizeof(A.TemporalMotionDesc)))
    dd.struct_bytes, dd.tri_first, dd.n_prev_triangles = C.sizeof(A.TemporalDeformDesc), tri_first, tri_entry[1][0]
    planes["prev_triangles"] = prev_triangles
    return ("rt_temporal_accumulate_deforming", dd, dict(A.TEMPORAL_DEFORM_PLANES, motions=entry, prev_triangles=tri_entry), planes,
            W, H)


def temporal_accumulate_host(guides, prev_guides, prev_camera, prev_color, prev_history, color, max_history=float("inf"),
                             point_tolerance=TEMPORAL_POINT_TOLERANCE, normal_cos=TEMPORAL_NORMAL_COS, out=None, out_history=None,
                             motion=False, motions=None, prev_triangles=None, tri_first=0):
    """rt_temporal_accumulate_host (with `motions`, a table of object_motions: rt_temporal_accumulate_moving_host; with
    `prev_triangles` / `tri_first` too: rt_temporal_accumulate_deforming_host): temporal accumulation's definition on the CPU
    (no device), with RayTracer.temporal_accumulate's arguments for numpy planes.  RayTracer.temporal_accumulate computes the
    same bits on the GPU."""
    fn, d, table, planes, W, H = _temporal_call(guides, prev_guides, prev_camera, prev_color, prev_history, color, max_history,
                                                point_tolerance, normal_cos, motions, prev_triangles, tri_first)
    if color is None:
        raise ValueError("color is required on the host")
    outs = {"out": _new_or(out), "out_history": _new_or(out_history), "motion": motion}
    return _temporal_result(_host_frame_call(fn + "_host", d, table, W, H, planes, outs))


def object_motions(prev_arrays, arrays, deformed=None):
    """rt_object_motions: the motion table that temporal_accumulate(..., motions=) takes, from two SceneArrays of one scene --
    before and after its meshes' transforms and its spheres were edited (the same topology: ValueError when the mesh or
    sphere counts differ).  Returns an (n_meshes + n_spheres,) OBJECT_MOTION_DTYPE array, indexed by the G-buffer's object
    word: per object whether it moved, and the map that carries its points and normals from the current frame's world to
    the previous frame's.
    `deformed` (rt_object_motions_deforming): the meshes whose vertices moved between the two states (refit_triangles) -- a
    sequence of mesh indices, or a boolean array with an entry per mesh.  Their records say DEFORMED (moved == 2) and hold
    the previous model_to_world; temporal_accumulate(..., motions=, prev_triangles=) carries their texels by the previous
    frame's triangles."""
    def records(x, dtype):
        a = np.ascontiguousarray(x)
        if a.nbytes % dtype.itemsize:
            raise ValueError(f"an array of {a.nbytes} bytes does not hold whole {dtype.itemsize}-byte records")
        return a, a.nbytes // dtype.itemsize
    (pm, npm), (m, nm) = records(prev_arrays.meshes, A.MESH_DTYPE), records(arrays.meshes, A.MESH_DTYPE)
    (ps, nps), (s, ns) = records(prev_arrays.spheres, A.SPHERE_DTYPE), records(arrays.spheres, A.SPHERE_DTYPE)
    if npm != nm or nps != ns:
        raise ValueError(f"the two scene states differ in topology: {npm} and {nm} meshes, {nps} and {ns} spheres")
    out = np.zeros(nm + ns, A.OBJECT_MOTION_DTYPE)
    L = load()
    args = (pm.ctypes.data if nm else None, m.ctypes.data if nm else None, nm, ps.ctypes.data if ns else None,
            s.ctypes.data if ns else None, ns)
    if deformed is None:
        rc = L.rt_object_motions(*args, out.ctypes.data if nm + ns else None)
    else:
        marks = np.asarray(deformed)
        if marks.dtype == np.bool_:
            if marks.shape != (nm,):
                raise ValueError(f"a boolean `deformed` has an entry per mesh: shape ({nm},), not {marks.shape}")
            marks = marks.astype(np.uint8)
        else:
            which = marks.astype(np.int64).reshape(-1)
            if which.size and (which.min() < 0 or which.max() >= nm):
                raise ValueError(f"`deformed` names a mesh outside [0, {nm})")
            marks = np.zeros(nm, np.uint8)
            marks[which] = 1
        marks = np.ascontiguousarray(np.append(marks, np.uint8(0)))   # (never empty: the pointer is not NULL)
        rc = L.rt_object_motions_deforming(*args, marks.ctypes.data, out.ctypes.data if nm + ns else None)
    if rc < 0:
        raise RtError(rc, "rt_object_motions refused its arguments")
    return out


# Guided upsampling's default thresholds (RayTracer.upsample, upsample_host): temporal accumulation's, with twice its plane
# distance -- a low texel's hit point lies up to a low texel's footprint away from the high texel's, not a fraction of
# one, and on a surface seen at a grazing angle that is further off the tangent plane.  DESIGN.md section 2.18 has what
# the quality test measured with them, and that (0.01, 0.95) .. (0.05, 0.8) measure the same.
UPSAMPLE_POINT_TOLERANCE, UPSAMPLE_NORMAL_COS = 0.02, 0.9


def _upsample_call(lo_guides, guides, color, point_tolerance, normal_cos):
    """rt_upsample's desc, its plane table with the low frame's shapes put in, the inputs by name and the high frame's size."""
    for g, what, need in ((lo_guides, "lo_guides", ("point", "normal", "object")), (guides, "guides", ("depth", "point", "normal", "object"))):
        for k in need:
            if k not in g:
                raise ValueError(f"{what} must hold the {k} plane of render_gbuffer")
    if ("albedo" in lo_guides) != ("albedo" in guides):
        raise ValueError("the albedo planes come together or not at all: lo_guides and guides must both hold `albedo`, or neither")
    planes = {"lo_point": lo_guides["point"], "lo_normal": lo_guides["normal"], "lo_object": lo_guides["object"]}
    planes.update({k: guides[k] for k in ("depth", "point", "normal", "object", "albedo", "emission") if k in guides})
    if "albedo" in lo_guides:
        planes["lo_albedo"] = lo_guides["albedo"]
    if color is not None:
        planes["lo_color"] = color
    w, h = _frame_size(planes["lo_normal"])
    W, H = _frame_size(planes["normal"])
    table = dict(A.UPSAMPLE_PLANES, **{k: (A.UPSAMPLE_PLANES[k][0], (h, w, n) if n else (h, w)) for k, n in A.UPSAMPLE_LO_COMPONENTS.items()})
    d = A.UpsampleDesc(struct_bytes=C.sizeof(A.UpsampleDesc), lo_width=w, lo_height=h, width=W, height=H,
                       point_tolerance=float(point_tolerance), normal_cos=float(normal_cos))
    return d, table, planes, W, H


def _upsample_result(res):
    return res["out"] if res["coverage"] is None else (res["out"], res["coverage"])


def upsample_host(lo_guides, guides, color, point_tolerance=UPSAMPLE_POINT_TOLERANCE, normal_cos=UPSAMPLE_NORMAL_COS, out=None,
                  coverage=False):
    """rt_upsample_host: guided upsampling's definition on the CPU (no device), with RayTracer.upsample's arguments for numpy
    planes.  RayTracer.upsample computes the same bits on the GPU."""
    if color is None:
        raise ValueError("color is required on the host")
    d, table, planes, W, H = _upsample_call(lo_guides, guides, color, point_tolerance, normal_cos)
    return _upsample_result(_host_frame_call("rt_upsample_host", d, table, W, H, planes, {"out": _new_or(out), "coverage": coverage}))


# ---- history rectification (RayTracer.temporal_reproject, .temporal_rectify; temporal_reproject_host, temporal_rectify_host) ----
# The defaults: a 7 x 7 window -- at 8 samples per pixel a 3 x 3 one is too few samples for a standard deviation, and the
# box then clips a converged history into noise --, a box of one standard deviation of a single frame's noise either way,
# which a converged history (noise / sqrt(n) off the mean) stays inside, and four frames kept of a clipped history.
# DESIGN.md section 2.20 has what the quality test measured with them.
RECTIFY_RADIUS, RECTIFY_CLIP_SIGMA, RECTIFY_CLIP_HISTORY = 3, 1.0, 4.0


def _nan_plane(guides):
    """The (H, W, 4) float32 plane of quiet NaNs that stands for `color` in a reprojection."""
    if "normal" not in guides:
        raise ValueError("guides must hold the normal and point planes of render_gbuffer")
    W, H = _frame_size(guides["normal"])
    return np.full((H, W, 4), np.nan, np.float32)


def temporal_reproject_host(guides, prev_guides, prev_camera, prev_color, prev_history, max_history=float("inf"),
                            point_tolerance=TEMPORAL_POINT_TOLERANCE, normal_cos=TEMPORAL_NORMAL_COS, out=None, out_history=None,
                            motion=False, motions=None, prev_triangles=None, tri_first=0):
    """The reprojected history alone, on the CPU: temporal_accumulate_host with a plane of quiet NaNs for `color`, which it
    drops -- `out` is prev_color fetched from where each texel lay (NaN where there is no history), out_history the
    fetched, capped history length (1 there).  What temporal_rectify_host takes as history / history_length."""
    return temporal_accumulate_host(guides, prev_guides, prev_camera, prev_color, prev_history, _nan_plane(guides), max_history,
                                    point_tolerance, normal_cos, out, out_history, motion, motions, prev_triangles, tri_first)


def _rectify_call(color, history, history_length, object, radius, clip_sigma, clip_history, moments, history_moments, out, out_history,
                  out_moments, clipped):
    """rt_temporal_rectify's desc, the inputs and the outputs by name and the frame's size."""
    if (moments is None) != (history_moments is None):
        raise ValueError("moments and history_moments come together or not at all")
    if moments is None and out_moments is not None:
        raise ValueError("out_moments needs moments and history_moments")
    planes = {"history": history, "history_length": history_length}
    for k, v in (("color", color), ("object", object), ("moments", moments), ("history_moments", history_moments)):
        if v is not None:
            planes[k] = v
    W, H = _frame_size(history)
    d = A.RectifyDesc(struct_bytes=C.sizeof(A.RectifyDesc), width=W, height=H, radius=int(radius), clip_sigma=float(clip_sigma),
                      clip_history=float(clip_history))
    outs = {"out": _new_or(out), "out_history": _new_or(out_history),
            "out_moments": None if moments is None else _new_or(out_moments), "out_clipped": clipped}
    return d, planes, outs, W, H


def _rectify_result(res):
    return tuple(res[k] for k in ("out", "out_history", "out_moments", "out_clipped") if res[k] is not None)


def temporal_rectify_host(color, history, history_length, object=None, radius=RECTIFY_RADIUS, clip_sigma=RECTIFY_CLIP_SIGMA,
                          clip_history=RECTIFY_CLIP_HISTORY, moments=None, history_moments=None, out=None, out_history=None,
                          out_moments=None, clipped=False):
    """rt_temporal_rectify_host: history rectification's definition on the CPU (no device), with RayTracer.temporal_rectify's
    arguments for numpy planes.  RayTracer.temporal_rectify computes the same bits on the GPU."""
    if color is None:
        raise ValueError("color is required on the host")
    d, planes, outs, W, H = _rectify_call(color, history, history_length, object, radius, clip_sigma, clip_history, moments,
                                          history_moments, out, out_history, out_moments, clipped)
    return _rectify_result(_host_frame_call("rt_temporal_rectify_host", d, A.RECTIFY_PLANES, W, H, planes, outs))


# ---- display frames (RayTracer.display, .auto_exposure, .snapshot_display; display_host, auto_exposure_host) ----
_DISPLAY_TONES = {"clamp": A.DISPLAY_TONE_CLAMP, "reinhard": A.DISPLAY_TONE_REINHARD}
_DISPLAY_TRANSFERS = {"srgb": A.DISPLAY_SRGB, "linear": A.DISPLAY_LINEAR}
# The meter's defaults: the darkest tenth and the brightest twentieth of the counted texels are left out (shadows that no
# exposure lifts, lamps that any exposure clips), the rest is brought to middle grey, within ten stops either way.
AUTO_EXPOSURE_LOW, AUTO_EXPOSURE_HIGH, AUTO_EXPOSURE_KEY, AUTO_EXPOSURE_MIN, AUTO_EXPOSURE_MAX = 100, 950, 0.18, 2.0 ** -10, 2.0 ** 10


def _one_float(v):
    """A one-float plane as the calls take it: a (1,) tensor as it is, anything else as a (1,) float32 array."""
    return v if hasattr(v, "data_ptr") else np.asarray(v, np.float32).reshape(-1)


def _display_desc(W, H, tone, transfer, bgra, top_first, exposure, white):
    tone, transfer = _DISPLAY_TONES.get(tone, tone), _DISPLAY_TRANSFERS.get(transfer, transfer)
    if tone not in _DISPLAY_TONES.values() or transfer not in _DISPLAY_TRANSFERS.values():
        raise ValueError("tone must be 'clamp' or 'reinhard' and transfer 'srgb' or 'linear' (or the ABI's numbers)")
    layout = (A.DISPLAY_LAYOUT_BGRA if bgra else 0) | (A.DISPLAY_LAYOUT_TOP_FIRST if top_first else 0)
    return A.DisplayDesc(struct_bytes=C.sizeof(A.DisplayDesc), width=W, height=H, tone=tone, transfer=transfer, layout=layout,
                         exposure=float(exposure), white=float(white))


def _display_call(color, width, height, out, exposure_scale, settings):
    """rt_display's desc, its inputs by name and the frame's size: that of `color`, of a given `out`, or width x height."""
    sized = color if color is not None else out if out is not None and out is not True else None
    W, H = _frame_size(sized) if sized is not None else (int(width or 0), int(height or 0))
    if W <= 0 or H <= 0:
        raise ValueError("without color (and out) the frame's width and height must be given")
    planes = {} if color is None else {"color": color}
    if exposure_scale is not None:
        planes["exposure_scale"] = _one_float(exposure_scale)
    return _display_desc(W, H, **settings), planes, W, H


def display_host(color, *, tone="clamp", transfer="srgb", bgra=False, top_first=False, exposure=1.0, white=float("inf"),
                 exposure_scale=None, out=None):
    """rt_display_host: the display pass's definition on the CPU (no device), with RayTracer.display's arguments for numpy
    planes.  RayTracer.display computes the same bytes on the GPU."""
    if color is None:
        raise ValueError("color is required on the host")
    d, planes, W, H = _display_call(color, None, None, out, exposure_scale, dict(tone=tone, transfer=transfer, bgra=bgra, top_first=top_first,
                                                                                 exposure=exposure, white=white))
    return _host_frame_call("rt_display_host", d, A.DISPLAY_PLANES, W, H, planes, {"out": _new_or(out)})["out"]


def _auto_exposure_call(color, width, height, low_permille, high_permille, key, min_scale, max_scale, rate, prev_scale):
    W, H = _frame_size(color) if color is not None else (int(width or 0), int(height or 0))
    if W <= 0 or H <= 0:
        raise ValueError("without color the frame's width and height must be given")
    low_permille, high_permille = int(low_permille), int(high_permille)
    if not 0 <= low_permille < high_permille <= 1000:
        raise ValueError("0 <= low_permille < high_permille <= 1000")
    d = A.AutoExposureDesc(struct_bytes=C.sizeof(A.AutoExposureDesc), width=W, height=H, low_permille=low_permille,
                           high_permille=high_permille, key=float(key), min_scale=float(min_scale), max_scale=float(max_scale), rate=float(rate))
    planes = {} if color is None else {"color": color}
    if prev_scale is not None:
        planes["prev_scale"] = _one_float(prev_scale)
    return d, planes, W, H


def _auto_exposure_result(res):
    return res["scale"] if res["histogram"] is None else (res["scale"], res["histogram"])


def auto_exposure_host(color, *, low_permille=AUTO_EXPOSURE_LOW, high_permille=AUTO_EXPOSURE_HIGH, key=AUTO_EXPOSURE_KEY,
                       min_scale=AUTO_EXPOSURE_MIN, max_scale=AUTO_EXPOSURE_MAX, rate=1.0, prev_scale=None, histogram=False, scale=None):
    """rt_auto_exposure_host: the exposure meter's definition on the CPU (no device), with RayTracer.auto_exposure's arguments
    for numpy planes.  RayTracer.auto_exposure computes the same bits on the GPU."""
    if color is None:
        raise ValueError("color is required on the host")
    d, planes, W, H = _auto_exposure_call(color, None, None, low_permille, high_permille, key, min_scale, max_scale, rate, prev_scale)
    return _auto_exposure_result(_host_frame_call("rt_auto_exposure_host", d, A.AUTO_EXPOSURE_PLANES, W, H, planes,
                                                  {"scale": _new_or(scale), "histogram": histogram}))


# The variance-guided denoiser's defaults (RayTracer.denoise_variance, denoise_variance_host): a luminance difference of
# sigma_luminance standard deviations of the local noise costs a factor e; a texel's accumulated moments give its variance
# once min_history frames stand behind them, and the 7 x 7 window does before that.
VDENOISE_SIGMA_LUMINANCE, VDENOISE_MIN_HISTORY = 4.0, 4.0


def _vdenoise_inputs(guides, color, moments, history):
    """The desc's input planes by name and the frame's size."""
    planes, W, H = _denoise_inputs(guides, color)
    if (moments is None) != (history is None):
        raise ValueError("moments and history go together")
    if moments is not None:
        planes.update(moments=moments, history=history)
    return planes, W, H


def _vdenoise_desc(W, H, iterations=1, sigma_luminance=VDENOISE_SIGMA_LUMINANCE, sigma_normal=DENOISE_SIGMA_NORMAL,
                   sigma_point=DENOISE_SIGMA_POINT, min_history=VDENOISE_MIN_HISTORY):
    return A.VDenoiseDesc(struct_bytes=C.sizeof(A.VDenoiseDesc), width=W, height=H, iterations=int(iterations),
                          sigma_luminance=float(sigma_luminance), sigma_normal=float(sigma_normal), sigma_point=float(sigma_point),
                          min_history=float(min_history))


def _vdenoise_result(res):
    return res["out"] if res.get("out_variance") is None else (res["out"], res["out_variance"])


def denoise_variance_host(guides, color, iterations=3, sigma_luminance=VDENOISE_SIGMA_LUMINANCE, sigma_normal=DENOISE_SIGMA_NORMAL,
                          sigma_point=DENOISE_SIGMA_POINT, moments=None, history=None, min_history=VDENOISE_MIN_HISTORY, out=None,
                          out_variance=None):
    """rt_denoise_variance_host: the variance-guided denoiser's definition on the CPU (no device), with
    RayTracer.denoise_variance's arguments for numpy planes.  RayTracer.denoise_variance computes the same bits on the GPU."""
    if color is None:
        raise ValueError("color is required on the host")
    planes, W, H = _vdenoise_inputs(guides, color, moments, history)
    d = _vdenoise_desc(W, H, iterations, sigma_luminance, sigma_normal, sigma_point, min_history)
    outs = {"out": _new_or(out), "out_variance": out_variance}
    return _vdenoise_result(_host_frame_call("rt_denoise_variance_host", d, A.VDENOISE_PLANES, W, H, planes, outs))


def luminance_moments_host(guides, color, out=None):
    """rt_luminance_moments_host: RayTracer.luminance_moments on the CPU (no device), for numpy planes."""
    if color is None:
        raise ValueError("color is required on the host")
    planes, W, H = _vdenoise_inputs(guides, color, None, None)
    return _host_frame_call("rt_luminance_moments_host", _vdenoise_desc(W, H), A.VDENOISE_PLANES, W, H, planes, {"out": _new_or(out)})["out"]


# Adaptive sampling's defaults (RayTracer.adaptive_plan / adaptive_samples, adaptive_plan_host): every texel gets at least
# one new sample, so that its variance estimate keeps moving, and at most 16, so that one firefly cannot take the budget.
ADAPTIVE_MIN_SAMPLES, ADAPTIVE_MAX_SAMPLES = 1, 16


def _adaptive_plan_desc(W, H, budget, origin, min_samples, max_samples, first_frame):
    budget, min_samples, max_samples, first_frame = int(budget), int(min_samples), int(max_samples), int(first_frame)
    if not 1 <= budget <= 0x7fffffff:
        raise ValueError("budget must be 1 .. 2^31 - 1")
    if min_samples < 0 or max_samples < 0 or not 0 <= first_frame <= 0xffffffff:
        raise ValueError("min_samples, max_samples and first_frame must fit a uint32")
    o = np.asarray(origin, np.float32).reshape(-1)
    if o.shape != (3,):
        raise ValueError("origin must have three components")
    return A.AdaptivePlanDesc(struct_bytes=C.sizeof(A.AdaptivePlanDesc), width=W, height=H, budget=budget, min_samples=min_samples,
                              max_samples=max_samples, first_frame=first_frame, origin=(C.c_float * 3)(*o.tolist()))


def _adaptive_merge_desc(W, H, budget, max_history):
    budget = int(budget)
    if not 1 <= budget <= 0x7fffffff:
        raise ValueError("budget must be 1 .. 2^31 - 1")
    return A.AdaptiveMergeDesc(struct_bytes=C.sizeof(A.AdaptiveMergeDesc), width=W, height=H, budget=budget, max_history=float(max_history))


def _adaptive_plan_call(variance, dirs, origin, budget, min_samples, max_samples, first_frame, tensors):
    """The plan's desc, its plane table -- _abi's and the two planes that are not frame-shaped: the packed records, as
    PATH_RAY_DTYPE on the host and as (budget, 8) float32 in a tensor, and the totals --, its inputs and its outputs."""
    H, W = (int(v) for v in np.shape(variance)) if np.ndim(variance) == 2 else (0, 0)
    d = _adaptive_plan_desc(W, H, budget, origin, min_samples, max_samples, first_frame)
    rays = ("<f4", (d.budget, 8)) if tensors else (A.PATH_RAY_DTYPE, (d.budget,))
    table = dict(A.ADAPTIVE_PLAN_PLANES, rays=rays, totals=("<u4", (4,)))
    return d, table, W, H, {"variance": variance, "dir": dirs}, {"counts": True, "offsets": True, "rays": True, "totals": True}


def _adaptive_plan_result(res):
    return res["counts"], res["offsets"], res["rays"], res["totals"]


def _adaptive_merge_call(radiance, counts, offsets, color, history, max_history, albedo, moments, out, out_history, out_moments):
    """The merge's desc, its plane table -- _abi's and `radiance`, which is not frame-shaped --, its inputs and its outputs;
    the frame's size is that of `counts`."""
    if moments is None and out_moments is not None:
        raise ValueError("out_moments needs moments")
    planes = {"radiance": radiance, "counts": counts, "offsets": offsets, "history": history}
    for k, v in (("color", color), ("albedo", albedo), ("moments", moments)):
        if v is not None:
            planes[k] = v
    outs = {"out": _new_or(out), "out_history": _new_or(out_history)}
    if moments is not None:
        outs["out_moments"] = _new_or(out_moments)
    H, W = (int(v) for v in np.shape(counts)[:2]) if np.ndim(counts) == 2 else (0, 0)
    if W == 0 or H == 0:
        raise ValueError("counts must have shape (H, W)")
    d = _adaptive_merge_desc(W, H, np.shape(radiance)[0] if np.ndim(radiance) == 2 else 0, max_history)
    return d, dict(A.ADAPTIVE_MERGE_PLANES, radiance=("<f4", (d.budget, 4))), W, H, planes, outs


def _adaptive_merge_result(res):
    return (res["out"], res["out_history"]) + ((res["out_moments"],) if "out_moments" in res else ())


def adaptive_plan_host(variance, dirs, origin, budget, min_samples=ADAPTIVE_MIN_SAMPLES, max_samples=ADAPTIVE_MAX_SAMPLES, first_frame=0):
    """rt_adaptive_plan_host: the plan's definition on the CPU (no device), with RayTracer.adaptive_plan's arguments for numpy
    planes.  RayTracer.adaptive_plan computes the same bits on the GPU."""
    d, table, W, H, planes, outs = _adaptive_plan_call(variance, dirs, origin, budget, min_samples, max_samples, first_frame, False)
    return _adaptive_plan_result(_host_frame_call("rt_adaptive_plan_host", d, table, W, H, planes, outs))


def adaptive_merge_host(radiance, counts, offsets, color, history, max_history=float("inf"), albedo=None, moments=None, out=None,
                        out_history=None, out_moments=None):
    """rt_adaptive_merge_host: the merge's definition on the CPU (no device), with RayTracer.adaptive_merge's arguments for
    numpy planes.  RayTracer.adaptive_merge computes the same bits on the GPU."""
    if color is None:
        raise ValueError("color is required on the host")
    d, table, W, H, planes, outs = _adaptive_merge_call(radiance, counts, offsets, color, history, max_history, albedo, moments, out,
                                                        out_history, out_moments)
    return _adaptive_merge_result(_host_frame_call("rt_adaptive_merge_host", d, table, W, H, planes, outs))


class RayTracer:
    def __init__(self, device=0, max_width=1920, max_height=1080, lib=None):
        self._L = lib or load()   # (lib=load_test(): a handle of the test library, for the rt_test_* entry points)
        self._h = C.c_void_p()
        rc = self._L.rt_create(device, max_width, max_height, C.byref(self._h))
        if rc < 0:
            msg = self._L.rt_last_error(self._h).decode()
            if self._h:
                self._L.rt_destroy(self._h)
                self._h = None
            raise RtError(rc, msg)
        self.max_width, self.max_height = max_width, max_height
        self.device = device
        # tuning knobs for experiments (results never depend on them): RT2_OPTIONS="forest=0,vote_eighths=5"
        for kv in os.environ.get("RT2_OPTIONS", "").split(","):
            if kv.strip():
                k, v = kv.split("=")
                self.set_option(k.strip(), int(v))

    def _check(self, rc):
        if rc < 0:
            raise RtError(rc, self._L.rt_last_error(self._h).decode())
        return rc

    def close(self):
        if getattr(self, "_h", None):
            self._L.rt_destroy(self._h)
            self._h = None

    __del__ = close

    # ---- reference-named methods --------------------------------------
    def load_scene_gpu_resources(self, arrays):
        descs, n = arrays.texture_descs()
        self._check(self._L.rt_upload_textures(self._h, descs, n))

    def update_buffers(self, arrays):
        a = arrays
        u = a.uniform
        self._check(self._L.rt_upload_scene(
            self._h, C.byref(u), a.spheres.ctypes.data, a.spheres.shape[0], a.meshes.ctypes.data,
            a.meshes.shape[0], a.triangles.ctypes.data, a.triangles.shape[0], a.nodes.ctypes.data,
            a.nodes.shape[0]))

    def update_instances(self, arrays):
        """The per-instance part of update_buffers (rt_update_instances): the SceneUniform, spheres and mesh uniforms of
        `arrays` over the triangles and nodes of the last update_buffers -- whose mesh count and per-mesh offsets `arrays`
        must keep.  Only the blob's head is rebuilt and sent."""
        a = arrays
        self._check(self._L.rt_update_instances(self._h, C.byref(a.uniform), a.spheres.ctypes.data, a.spheres.shape[0],
                                                a.meshes.ctypes.data, a.meshes.shape[0]))

    def update_built_scene(self, scene):
        """update_instances from a built Scene (C++ object) after its setters (rt_update_built_scene)."""
        self._check(self._L.rt_update_built_scene(self._h, scene._p))

    def refit_triangles(self, triangles, first):
        """Moved vertices, same topology (rt_refit_triangles): uploaded triangles [first, first + n) become `triangles` and
        the BVH is refitted on the device; the handle then equals a fresh update_buffers of the arrays with those triangles
        and SceneArrays.refit_bvh(first, n)'s nodes.  `triangles`: n TRI_DTYPE records (numpy), or a float32 tensor of
        shape (n, 24) on this handle's device -- read in order after the current torch stream's work, as trace_rays is."""
        if hasattr(triangles, "data_ptr"):
            import torch
            t = triangles
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
                raise ValueError("device triangles must be a float32 tensor")
            if t.device.type != "cuda" or t.device.index != self.device:
                raise ValueError(f"device triangles must be on cuda:{self.device}, not {t.device}")
            if t.dim() != 2 or t.shape[1] != 24:
                raise ValueError("device triangles must have shape (n, 24)")
            t = t.contiguous()
            n = t.shape[0]
            # (the call has read t when it returns; later work on the stream follows the refit)
            self._on_handle_stream(lambda: self._check(self._L.rt_refit_triangles(self._h, t.data_ptr() if n else None, int(first), n, 0)))
            return
        t = np.ascontiguousarray(triangles).view(A.TRI_DTYPE).reshape(-1)
        self._check(self._L.rt_refit_triangles(self._h, t.ctypes.data if t.shape[0] else None, int(first), t.shape[0],
                                               A.REFIT_HOST_MEMORY))

    def refit_built_scene(self, scene, first_mesh=0, n_meshes=None):
        """refit_triangles with the packed triangles of mesh instances [first_mesh, first_mesh + n_meshes) of a built Scene
        (C++ object) after its set_mesh_vertices (rt_refit_built_scene); n_meshes None: the rest of them."""
        if n_meshes is None:
            n_meshes = self._L.rt_scene_num_meshes(scene._p) - int(first_mesh)
        self._check(self._L.rt_refit_built_scene(self._h, scene._p, int(first_mesh), int(n_meshes)))

    def load_built_scene(self, scene):
        """A built Scene (C++ object) straight to the device: textures + arrays, without the round trip through numpy
        (rt_upload_built_scene: what the C++ mirror's load_scene_gpu_resources + update_buffers do)."""
        self._check(self._L.rt_upload_built_scene(self._h, scene._p))

    def load_scene(self, scene):
        """Scene (C++ object) or SceneArrays -> device."""
        arrays = SceneArrays.from_scene(scene) if isinstance(scene, Scene) else scene
        self.load_scene_gpu_resources(arrays)
        self.update_buffers(arrays)
        return arrays

    def set_camera(self, camera_uniform):
        self._check(self._L.rt_set_camera(self._h, C.byref(camera_uniform)))

    def render(self, params):
        self._check(self._L.rt_render(self._h, C.byref(params)))

    def render_frames(self, params, n_frames):
        """n_frames consecutive frames (Params.frames advancing), sampled in batches of overlapped frames."""
        self._check(self._L.rt_render_frames(self._h, C.byref(params), n_frames))

    def render_strips(self, params, rank, world):
        self._check(self._L.rt_render_strips(self._h, C.byref(params), rank, world))

    def render_strips_frames(self, params, n_frames, rank, world):
        self._check(self._L.rt_render_strips_frames(self._h, C.byref(params), n_frames, rank, world))

    # ---- data movement / bookkeeping ----------------------------------
    def synchronize(self):
        self._check(self._L.rt_synchronize(self._h))

    def read_image(self, width, height):
        out = np.empty((height, width, 4), dtype=np.float32)
        self._check(self._L.rt_read_image(self._h, out.ctypes.data, out.nbytes))
        return out

    def read_texels(self, n_texels):
        out = np.empty((n_texels, 4), dtype=np.float32)
        self._check(self._L.rt_read_image(self._h, out.ctypes.data, out.nbytes))
        return out

    def snapshot_image(self, width, height):
        """Keep the image as it is now aside (stream-ordered device copy; does not block)."""
        self._check(self._L.rt_snapshot_image(self._h, width * height * 16))

    def read_snapshot(self, width, height):
        """The last snapshot, read on a stream of its own: later frames are not waited for."""
        out = np.empty((height, width, 4), dtype=np.float32)
        self._check(self._L.rt_read_snapshot(self._h, out.ctypes.data, out.nbytes))
        return out

    def snapshot_display(self, width, height, *, tone="clamp", transfer="srgb", bgra=False, top_first=False, exposure=1.0,
                         white=float("inf"), exposure_scale=None):
        """Keep the picture of the image as it is now aside: snapshot_image with the display pass (display's arguments) in the
        place of the copy -- four bytes per texel in a buffer of the handle's own; does not block.  `exposure_scale`: a (1,)
        float32 tensor on this handle's device (auto_exposure's), read in stream order."""
        d = _display_desc(int(width), int(height), tone, transfer, bgra, top_first, exposure, white)
        if exposure_scale is None:
            return self._check(self._L.rt_snapshot_display(self._h, C.byref(d)))
        if not hasattr(exposure_scale, "data_ptr"):
            raise ValueError("exposure_scale must be a (1,) float32 tensor on the device (a number goes into `exposure`)")
        _tensor_planes(d, self.device, A.DISPLAY_PLANES, d.width, d.height, {"exposure_scale": exposure_scale}, {})
        self._on_handle_stream(lambda: self._check(self._L.rt_snapshot_display(self._h, C.byref(d))))

    def read_display_snapshot(self, width, height):
        """The last display snapshot as (height, width, 4) uint8, read on a stream of its own: later frames are not waited for."""
        out = np.empty((height, width, 4), dtype=np.uint8)
        self._check(self._L.rt_read_display_snapshot(self._h, out.ctypes.data, out.nbytes))
        return out

    def write_image(self, img):
        img = np.ascontiguousarray(img, dtype=np.float32)
        self._check(self._L.rt_write_image(self._h, img.ctypes.data, img.nbytes))

    def assemble_strips(self, gathered_device_ptr, width, height, world):
        self._check(self._L.rt_assemble_strips(self._h, gathered_device_ptr, width, height, world))

    def set_counters(self, enabled):
        self._check(self._L.rt_set_counters(self._h, int(enabled)))

    def set_option(self, name, value):
        self._check(self._L.rt_set_option(self._h, name.encode(), int(value)))

    def reset_timing(self):
        self._check(self._L.rt_reset_timing(self._h))

    def set_stream(self, hip_stream_ptr):
        self._check(self._L.rt_set_stream(self._h, hip_stream_ptr))

    def bind_image(self, device_ptr, texels):
        self._check(self._L.rt_bind_image(self._h, device_ptr, texels))

    # ---- test-only: the device's arithmetic building blocks (tests/test_gpu_device_units.py) ----
    def sweep(self, which):
        """(floats checked, mismatches, a mismatching bit pattern) of the kernels' short reciprocal (which = 0) / square root
        (1) against the compiler's IEEE 1.0f / x / sqrt on the device, over every float the short form serves."""
        out = (C.c_uint64 * 3)()
        self._check(self._L.rt_test_sweep(self._h, which, out))
        return int(out[0]), int(out[1]), int(out[2])

    def device_units(self, fn, x, y=None):
        x = np.ascontiguousarray(x).view(np.float32).ravel()
        y = np.zeros_like(x) if y is None else np.ascontiguousarray(y).view(np.float32).ravel()
        out = np.empty_like(x)
        self._check(self._L.rt_test_device_units(self._h, fn, x.ctypes.data, y.ctypes.data, out.ctypes.data, x.size))
        return out

    def device_sample_texture(self, tex_rgba8, uv):
        tex = np.ascontiguousarray(tex_rgba8, dtype=np.uint8)
        uv = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
        d = A.TextureDesc(tex.ctypes.data, tex.shape[1], tex.shape[0])
        out = np.empty((uv.shape[0], 4), np.float32)
        self._check(self._L.rt_test_device_sample_texture(self._h, C.byref(d), uv.ctypes.data, out.ctypes.data, uv.shape[0]))
        return out

    # ---- test-only: the kernels' ray-scene intersection for chosen rays (tests/test_gpu_intersect.py) ----
    def intersect(self, ro, rd, active=None, general=False, simple=False, stats=False):
        """intersect_scene on the uploaded scene for rays (ro[i], normalize3(rd[i])), one lane per ray, in the instantiation
        a render would take (general / simple force one; stats: the counter instantiation).  Returns the (n, 16) u32
        records of include/rt_test_abi.h (rt_test_intersect); inactive rays (active[i] == 0) are not traced and stay zero."""
        ro = np.ascontiguousarray(ro, np.float32).reshape(-1, 3)
        rd = normalize3_f32(rd)
        if ro.shape != rd.shape or not (np.isfinite(ro).all() and np.isfinite(rd).all()):
            raise ValueError("rays must be finite, with non-zero directions of finite length")
        n = ro.shape[0]
        act = None
        if active is not None:
            act = np.ascontiguousarray(active, np.uint8).ravel()
            if act.size != n:
                raise ValueError("one active flag per ray")
        out = np.zeros((n, 16), np.uint32)
        flags = (1 if general else 0) | (2 if stats else 0) | (4 if simple else 0)
        self._check(self._L.rt_test_intersect(self._h, ro.ctypes.data, rd.ctypes.data, None if act is None else act.ctypes.data,
                                              n, flags, out.ctypes.data))
        return out

    # ---- test-only: the kernels' shading step for chosen lane states and hits (tests/test_gpu_shade.py) ----
    def shade(self, cases, number_of_bounces, rays_per_pixel, skybox=1, active=None, roulette_skip=False, general=False,
              simple=False, fast_miss=True, total_regs=False):
        """path_end (roulette_skip=True: the pre-step's roulette skip) on the uploaded scene's materials for the (n, 32) u32
        case records of include/rt_test_abi.h (rt_test_shade), one lane per case, in the instantiation a render would take
        (general / simple force one; fast_miss=False: the counter builds' path_end; total_regs: the pixel sum in
        registers).  Returns the (n, 32) u32 records; inactive cases (active[i] == 0) stay out and stay zero."""
        cases = np.ascontiguousarray(cases, np.uint32)
        if cases.ndim != 2 or cases.shape[1] != 32:
            raise ValueError("cases are (n, 32) u32 records")
        n = cases.shape[0]
        act = None
        if active is not None:
            act = np.ascontiguousarray(active, np.uint8).ravel()
            if act.size != n:
                raise ValueError("one active flag per case")
        out = np.zeros((n, 32), np.uint32)
        flags = (1 if general else 0) | (0 if fast_miss else 2) | (4 if simple else 0) | (8 if total_regs else 0)
        self._check(self._L.rt_test_shade(self._h, 1 if roulette_skip else 0, cases.ctypes.data, None if act is None else act.ctypes.data,
                                          n, int(number_of_bounces), int(rays_per_pixel), int(skybox), flags, out.ctypes.data))
        return out

    # ---- test-only: the scene blob (tests/test_gpu_scene_edits.py) ----
    def scene_blob(self):
        """(blob bytes as uint8, SceneLayout as 12 uint32 -- A.SCENE_LAYOUT_FIELDS --, device address) of the uploaded scene
        (rt_test_scene_blob; waits for the handle's streams)."""
        lay, ptr = (C.c_uint32 * 12)(), C.c_uint64()
        self._check(self._L.rt_test_scene_blob(self._h, None, 0, C.byref(lay), C.byref(ptr)))
        out = np.empty(lay[9], np.uint8)
        self._check(self._L.rt_test_scene_blob(self._h, out.ctypes.data, out.nbytes, C.byref(lay), C.byref(ptr)))
        return out, np.array(lay, np.uint32), int(ptr.value)

    PACK_OPTIONS = dict(tlas=1, forest=1, flat2=1, tlas_min=8, defer_min_nodes=1024)   # (the handle's defaults)

    @staticmethod
    def pack_scene(arrays, **options):
        """(blob bytes as uint8, SceneLayout as 12 uint32, fact words as RT_TEST_PACK_FACTS uint32 -- A.PACK_FACT_FIELDS) of
        `arrays` as the host packer lays them out under `options` (PACK_OPTIONS: what set_option would have set before
        update_buffers): rt_test_pack_scene, no device and no handle."""
        from .lib import load_test
        L, a = load_test(), arrays
        opt = dict(RayTracer.PACK_OPTIONS)
        if set(options) - set(opt):
            raise ValueError(f"unknown packer options {sorted(set(options) - set(opt))}")
        opt.update(options)
        o = (C.c_int32 * 5)(*(int(opt[k]) for k in RayTracer.PACK_OPTIONS))
        lay, facts = (C.c_uint32 * 12)(), (C.c_uint32 * 18)()
        args = (a.spheres.ctypes.data, a.spheres.shape[0], a.meshes.ctypes.data, a.meshes.shape[0], a.triangles.ctypes.data,
                a.triangles.shape[0], a.nodes.ctypes.data, a.nodes.shape[0], C.byref(o))
        out = None
        for _ in range(2):
            rc = L.rt_test_pack_scene(*args, None if out is None else out.ctypes.data, 0 if out is None else out.nbytes,
                                      C.byref(lay), C.byref(facts))
            if rc < 0:
                raise RtError(rc, L.rt_last_error(None).decode())
            if out is None:
                out = np.empty(lay[9], np.uint8)
        return out, np.array(lay, np.uint32), np.array(facts, np.uint32)

    # ---- ray queries (rt_intersect_rays, rt_occluded_rays, rt_pick), frame-wide first hits (rt_render_gbuffer), radiance (rt_radiance_rays) ----
    def trace_rays(self, origins, dirs, tmax=None):
        """Closest hit of rays (origins[i], dirs[i]) on the uploaded scene, as a render's walk computes it; a hit at
        t >= tmax[i] is reported as a miss (tmax None: unbounded).  numpy inputs: a synchronous call that returns a
        numpy structured array of HIT_DTYPE (rt_hit).  Tensors on this handle's device (anything with data_ptr()):
        an asynchronous call ordered after the current stream's work; returns an (n, 16) int32 tensor of rt_hit records
        (hits_to_numpy converts it).  Invalid rays get miss records."""
        rays, dev = self._query_rays(origins, dirs, tmax)
        n = rays.shape[0]
        if not dev:
            hits = np.zeros(n, A.HIT_DTYPE)
            if n:
                self._check(self._L.rt_intersect_rays(self._h, rays.ctypes.data, n, hits.ctypes.data, A.QUERY_HOST_MEMORY))
            return hits
        import torch
        hits = torch.empty((n, 16), dtype=torch.int32, device=rays.device)
        self._device_query(self._L.rt_intersect_rays, rays, hits, 0)
        return hits

    def occluded(self, origins, dirs, tmax, prune=False):
        """Is there a hit closer than tmax on each ray (shadow rays)?  numpy inputs: a numpy bool array; tensors on this
        handle's device: a bool tensor (asynchronous).  prune: RT_QUERY_PRUNE_TMAX, the faster walk that is not exact
        (include/rt_abi.h)."""
        if tmax is None:
            raise ValueError("occluded needs tmax")
        rays, dev = self._query_rays(origins, dirs, tmax)
        n = rays.shape[0]
        flags = A.QUERY_PRUNE_TMAX if prune else 0
        if not dev:
            occ = np.zeros(n, np.uint32)
            if n:
                self._check(self._L.rt_occluded_rays(self._h, rays.ctypes.data, n, occ.ctypes.data, flags | A.QUERY_HOST_MEMORY))
            return occ != 0
        import torch
        occ = torch.empty(n, dtype=torch.int32, device=rays.device)
        self._device_query(self._L.rt_occluded_rays, rays, occ, flags)
        return occ != 0

    def pick(self, params, x, y):
        """The closest hit under texel (x, y) of a params.width x params.height frame (row 0 = bottom), as the debug
        views trace it: a dict of the rt_hit fields, or None for a miss."""
        hit = A.Hit()
        self._check(self._L.rt_pick(self._h, C.byref(params), int(x), int(y), C.byref(hit)))
        if not hit.flags & A.HIT_HIT:
            return None
        return {"t": hit.t, "object": hit.object, "primitive": hit.primitive, "backface": bool(hit.flags & A.HIT_BACKFACE),
                "point": tuple(hit.point), "normal": tuple(hit.normal), "bary": (hit.bary_u, hit.bary_v),
                "uv": (hit.tex_u, hit.tex_v)}

    def render_gbuffer(self, params, channels=("depth", "normal", "albedo", "object"), device=False):
        """First-hit buffers of the params.width x params.height frame for the camera currently set (rt_render_gbuffer): per
        texel the closest hit of the ray the debug views and pick trace for it, row 0 = bottom.  `channels`: names of
        rt_gbuffer's planes (_abi.GBUFFER_CHANNELS); a channel that is not asked for costs nothing.  Returns a dict of
        numpy arrays of shape (H, W) or (H, W, C) (synchronous), or with device=True of torch tensors on this handle's
        device, produced asynchronously after the current torch stream's work, as trace_rays orders itself."""
        if not isinstance(params, A.Params):
            raise ValueError("params must be a Params (make_params)")
        channels = tuple(channels)
        for c in channels:
            if c not in A.GBUFFER_CHANNELS:
                raise ValueError(f"unknown G-buffer channel {c!r}: one of {', '.join(A.GBUFFER_CHANNELS)}")
        if len(set(channels)) != len(channels):
            raise ValueError("a G-buffer channel is named twice")
        H, W = int(params.height), int(params.width)
        g = A.GBuffer(struct_bytes=C.sizeof(A.GBuffer))
        out = {}
        if not device:
            for c in channels:
                dt, k = A.GBUFFER_CHANNELS[c]
                out[c] = np.zeros((H, W, k) if k else (H, W), np.dtype(dt))
                setattr(g, c, out[c].ctypes.data)
            self._check(self._L.rt_render_gbuffer(self._h, C.byref(params), C.byref(g), A.GBUFFER_HOST_MEMORY))
            return out
        import torch
        dev = torch.device("cuda", self.device)
        kinds = {"<f4": torch.float32, "<u4": torch.int32, "u1": torch.uint8}   # (object / primitive: the u32 bits as int32)
        for c in channels:
            dt, k = A.GBUFFER_CHANNELS[c]
            out[c] = torch.empty((H, W, k) if k else (H, W), dtype=kinds[dt], device=dev)
            setattr(g, c, out[c].data_ptr() if out[c].numel() else None)
        self._on_handle_stream(lambda: self._check(self._L.rt_render_gbuffer(self._h, C.byref(params), C.byref(g), 0)))
        return out

    def denoise(self, guides, color=None, iterations=3, sigma_color=DENOISE_SIGMA_COLOR, sigma_normal=DENOISE_SIGMA_NORMAL,
                sigma_point=DENOISE_SIGMA_POINT, out=None):
        """The G-buffer-guided a-trous filter (rt_denoise; include/rt_abi.h has the definition) of the (H, W, 4) float32
        frame `color`.  `guides`: the dict render_gbuffer returns for the same frame; it must hold `normal` and `point`,
        and `albedo` (demodulation) and `emission` (lamps are left alone) are used when present.  `iterations`: 1 .. 8
        passes with steps 1, 2, 4, ...  The sigmas' units: `sigma_color` demodulated radiance (colour / albedo; halved
        per pass, inf switches the term off), `sigma_normal` the length of the difference of two unit normals,
        `sigma_point` world units (scale it with the scene).
        numpy planes: a synchronous call that returns a numpy array (`out`, when given: it may be `color`).  Torch tensors
        on this handle's device: an asynchronous call ordered after the current torch stream's work, as
        render_gbuffer(device=True) orders itself; returns a tensor; there color=None denoises the handle's image, into
        `out` or a new tensor."""
        planes, W, H = _denoise_inputs(guides, color)
        d = _denoise_desc(W, H, iterations, sigma_color, sigma_normal, sigma_point)
        return self._frame_call("rt_denoise", A.DENOISE_HOST_MEMORY, d, A.DENOISE_PLANES, W, H, planes, {"out": _new_or(out)})["out"]

    def _frame_call(self, fn, host_flag, d, table, W, H, planes, outs):
        """A frame pass (`fn`: the entry point's name) on numpy planes (synchronous, under `host_flag`) or on torch tensors of
        this handle's device (asynchronous, ordered after the current torch stream's work).  planes: the inputs by name,
        where a pass with a colour plane takes the handle's image when tensors come without one; outs: name -> None or
        False (not asked for), True (a new one) or the array / tensor to fill.  Returns the outputs by name."""
        if not any(hasattr(v, "data_ptr") for v in (*planes.values(), *outs.values())):
            if "color" in table and "color" not in planes:
                raise ValueError("color is required with numpy planes (color=None names the device image)")
            keep = _numpy_inputs(d, table, W, H, planes)
            res = _numpy_outputs(d, table, W, H, outs)
            self._check(getattr(self._L, fn)(self._h, C.byref(d), host_flag))
            del keep
            return res
        res = _tensor_planes(d, self.device, table, W, H, planes, outs)
        self._on_handle_stream(lambda: self._check(getattr(self._L, fn)(self._h, C.byref(d), 0)))
        return res

    def denoise_variance(self, guides, color=None, iterations=3, sigma_luminance=VDENOISE_SIGMA_LUMINANCE,
                         sigma_normal=DENOISE_SIGMA_NORMAL, sigma_point=DENOISE_SIGMA_POINT, moments=None, history=None,
                         min_history=VDENOISE_MIN_HISTORY, out=None, out_variance=None):
        """The variance-guided a-trous filter (rt_denoise_variance; include/rt_abi.h has the definition) of the (H, W, 4)
        float32 frame `color`: denoise's filter with the luminance edge term measured in standard deviations of each
        texel's own noise, so that a frame with a long history is blurred less than a lone one.  `guides`: as for denoise.
        `moments` (H, W, 4) / `history` (H, W): the luminance moments of the frames behind `color` -- luminance_moments
        of each raw frame, accumulated by a temporal_accumulate call of their own -- and the frames accumulated in them;
        where history < min_history, or without them, the variance comes from a 7 x 7 window of the frame itself.
        `sigma_luminance`: the luminance difference, in standard deviations, that costs a tap a factor e.
        `out_variance`: True, or an (H, W) array / tensor to fill, for the variance left in the filtered frame; the call then
        returns (out, out_variance).
        numpy planes: a synchronous call that returns numpy (`out`, when given: it may be `color`).  Torch tensors on this
        handle's device: an asynchronous call ordered after the current torch stream's work; returns tensors; there
        color=None denoises the handle's image."""
        planes, W, H = _vdenoise_inputs(guides, color, moments, history)
        d = _vdenoise_desc(W, H, iterations, sigma_luminance, sigma_normal, sigma_point, min_history)
        res = self._frame_call("rt_denoise_variance", A.VDENOISE_HOST_MEMORY, d, A.VDENOISE_PLANES, W, H, planes,
                               {"out": _new_or(out), "out_variance": out_variance})
        return _vdenoise_result(res)

    def luminance_moments(self, guides, color=None, out=None):
        """The per-frame sample of the luminance moments (rt_luminance_moments): (l, l l, 0, 0) per filterable texel of
        the frame `color`, l the luminance of colour / albedo, and zeros elsewhere, as an (H, W, 4) float32 array or
        tensor.  Accumulated over frames by temporal_accumulate (color = this, prev_color = the accumulated moments), it
        is what denoise_variance takes as `moments`.  numpy planes or torch tensors, as denoise_variance."""
        planes, W, H = _vdenoise_inputs(guides, color, None, None)
        res = self._frame_call("rt_luminance_moments", A.VDENOISE_HOST_MEMORY, _vdenoise_desc(W, H), A.VDENOISE_PLANES, W, H, planes,
                               {"out": _new_or(out)})
        return res["out"]

    def _on_handle_stream(self, call):
        """Runs call() on the handle's stream, ordered after the current torch stream's work and before what follows on it."""
        import torch
        dev = torch.device("cuda", self.device)
        cur = torch.cuda.current_stream(dev)
        ext = torch.cuda.ExternalStream(self._L.rt_stream(self._h), device=dev)
        ext.wait_stream(cur)
        call()
        # (the call's tensors belong to the current stream, which now waits for the launches: a later reuse of their memory is
        # ordered after them -- no record_stream on the handle's stream, which rt_destroy may destroy before they are freed)
        cur.wait_stream(ext)

    def adaptive_plan(self, variance, dirs, origin, budget, min_samples=ADAPTIVE_MIN_SAMPLES, max_samples=ADAPTIVE_MAX_SAMPLES,
                      first_frame=0):
        """Apportions `budget` rays over the texels of a frame in proportion to their standard deviation (rt_adaptive_plan;
        include/rt_abi.h has the definition).  `variance`: (H, W) float32, denoise_variance's out_variance; `dirs`: (H, W, 3),
        the `dir` plane of render_gbuffer; `origin`: the camera position, the origin of every ray.  Every texel gets between
        `min_samples` and `max_samples` rays; texel p's sample k has the seed of pixel p in frame first_frame + k.  Returns
        (counts, offsets, rays, totals): (H, W) uint32 each, the `budget` rt_path_ray records (those past totals[0] are
        zeros, which radiance answers with zeros) and (rays planned, texels above min_samples, texels clamped by
        max_samples, 0).
        numpy planes: a synchronous call that returns numpy (rays: PATH_RAY_DTYPE).  Torch tensors on this handle's device:
        an asynchronous call ordered after the current torch stream's work; counts, offsets and totals are int32 tensors
        holding the u32 bits, rays a (budget, 8) float32 tensor of the packed records."""
        tensors = hasattr(variance, "data_ptr") or hasattr(dirs, "data_ptr")
        d, table, W, H, planes, outs = _adaptive_plan_call(variance, dirs, origin, budget, min_samples, max_samples, first_frame, tensors)
        return _adaptive_plan_result(self._frame_call("rt_adaptive_plan", A.ADAPTIVE_HOST_MEMORY, d, table, W, H, planes, outs))

    def adaptive_merge(self, radiance, counts, offsets, color, history, max_history=float("inf"), albedo=None, moments=None, out=None,
                       out_history=None, out_moments=None):
        """Blends the samples traced for a plan into the accumulation (rt_adaptive_merge; include/rt_abi.h has the definition):
        texel p takes radiance[offsets[p] + k], k < counts[p], one at a time, each as one more unit of its history --
        `color` (H, W, 4) and `history` (H, W; 0 or anything below 1: no prior) are the accumulation so far, `max_history`
        caps the history length.  With `moments` (H, W, 4) the luminance moments of each sample (of radiance / albedo, with
        `albedo` (H, W, 4) given) are accumulated the same way.  Returns (out, out_history) or (out, out_history,
        out_moments); the outputs may be the inputs.
        numpy planes: a synchronous call that returns numpy.  Torch tensors on this handle's device: an asynchronous call
        ordered after the current torch stream's work; returns tensors; there color=None names the handle's image."""
        d, table, W, H, planes, outs = _adaptive_merge_call(radiance, counts, offsets, color, history, max_history, albedo, moments, out,
                                                            out_history, out_moments)
        return _adaptive_merge_result(self._frame_call("rt_adaptive_merge", A.ADAPTIVE_HOST_MEMORY, d, table, W, H, planes, outs))

    def adaptive_samples(self, guides, variance, color, history, budget, bounces, samples, origin, min_samples=ADAPTIVE_MIN_SAMPLES,
                         max_samples=ADAPTIVE_MAX_SAMPLES, first_frame=0, max_history=float("inf"), moments=None, skybox=True,
                         out=None, out_history=None, out_moments=None):
        """One round of adaptive sampling: adaptive_plan on `variance` and guides["dir"], the planned rays traced by
        rt_radiance_rays (`bounces`, `samples` per ray record, `skybox`: as radiance) straight from the packed record
        buffer, and adaptive_merge of the result into `color` / `history` (and `moments`, demodulated by guides["albedo"]
        when present).  `origin`: the camera position.  Returns (out, out_history[, out_moments], counts, totals).
        numpy planes: three synchronous calls.  Torch tensors on this handle's device: the three calls are queued on the
        handle's stream with no host synchronisation between them -- the list's tail past the planned total is zero
        records, so nothing is read back --, ordered after the current torch stream's work; color=None names the handle's
        image."""
        bounces, samples = int(bounces), int(samples)
        if bounces < 0:
            raise ValueError("bounces must be >= 0")
        if samples < 1:
            raise ValueError("samples must be >= 1")
        if "dir" not in guides:
            raise ValueError("guides must hold the dir plane of render_gbuffer")
        params = A.make_params(0, 0, bounces, samples, skybox=1 if skybox else 0)
        albedo = guides.get("albedo") if moments is not None else None
        counts, offsets, rays, totals = self.adaptive_plan(variance, guides["dir"], origin, budget, min_samples, max_samples, first_frame)
        n = int(rays.shape[0])
        if hasattr(rays, "data_ptr"):
            import torch
            radiance = torch.empty((n, 4), dtype=torch.float32, device=rays.device)
            self._device_query(lambda h, r, m, o, f: self._L.rt_radiance_rays(h, C.byref(params), r, m, o, f), rays, radiance, 0)
        else:
            radiance = np.zeros((n, 4), np.float32)
            self._check(self._L.rt_radiance_rays(self._h, C.byref(params), rays.ctypes.data, n, radiance.ctypes.data, A.RADIANCE_HOST_MEMORY))
        res = self.adaptive_merge(radiance, counts, offsets, color, history, max_history, albedo, moments, out, out_history, out_moments)
        return (*res, counts, totals)

    def temporal_accumulate(self, guides, prev_guides, prev_camera, prev_color, prev_history, color=None, max_history=float("inf"),
                            point_tolerance=TEMPORAL_POINT_TOLERANCE, normal_cos=TEMPORAL_NORMAL_COS, out=None, out_history=None,
                            motion=False, motions=None, prev_triangles=None, tri_first=0):
        """Temporal accumulation across a camera move (rt_temporal_accumulate; include/rt_abi.h has the definition): every
        texel of the current frame `color` (H, W, 4) fetches the history `prev_color` (H, W, 4) / `prev_history` (H, W;
        frames accumulated, as float32 >= 1) from where its hit point lay under `prev_camera` (a CameraUniform), through
        bilinear taps validated against the two G-buffers, and blends itself in with the shader's accumulation at its own
        weight.  `guides`, `prev_guides`: the dicts render_gbuffer returns for the two frames; each must hold `point` and
        `normal`, and `object` is compared when both hold it.  `max_history` caps the history length (inf: a plain
        running mean); `point_tolerance` is the distance off the texel's tangent plane a tap may lie, per unit of view
        depth; `normal_cos` the least cosine between the two normals.  Returns (out, out_history), or with motion=True (or
        an array / tensor to fill) (out, out_history, motion): motion is the screen-space offset, in texels, to the
        position the history came from (NaN where nothing was reprojected).  out / out_history must not be any prev_*
        plane; `out` may be `color`.
        `motions` (rt_temporal_accumulate_moving): the table of object_motions(prev_arrays, arrays) for a scene whose
        meshes or spheres moved between the two frames -- `guides` must then hold `object`.  A moved object's texels fetch
        the history of their own surface point, and `motion` is what the camera and the object produce together; an object
        the table marks as still is worked as without a table.  What is kept is the object's own history, not the lighting
        that changed around it: `max_history` bounds how long that lags, and temporal_reproject + temporal_rectify cut the
        history where the new frame contradicts it.  A second call with the luminance moments as
        color / prev_color and the same `motions` accumulates the moments denoise_variance takes for a moving object, as it
        does for a moving camera.
        `prev_triangles`, `tri_first` (rt_temporal_accumulate_deforming): for a mesh whose vertices moved between the two
        frames (refit_triangles) -- `motions` is then object_motions(prev_arrays, arrays, deformed=...), `guides` must also
        hold `primitive`, `bary` and `flags`, and `prev_triangles` are the uploaded triangles [tri_first, tri_first + n) as
        they were in the previous frame: n TRI_DTYPE records, or an (n, 24) float32 tensor on the device, the forms
        refit_triangles takes.  A deformed mesh's texels fetch the history of their own surface point on the previous
        triangle; a texel whose triangle lies outside the range restarts, as does a mesh whose topology changed.
        numpy planes: a synchronous call that returns numpy arrays.  Torch tensors on this handle's device: an asynchronous
        call ordered after the current torch stream's work, as render_gbuffer(device=True) orders itself; returns tensors;
        there color=None takes the handle's image as the current frame, and `motions` is an (n_objects, 24) int32 tensor of
        the records' words (torch.from_numpy(table.view(np.int32).reshape(-1, 24)) moved to the device)."""
        fn, d, table, planes, W, H = _temporal_call(guides, prev_guides, prev_camera, prev_color, prev_history, color, max_history,
                                                    point_tolerance, normal_cos, motions, prev_triangles, tri_first)
        outs = {"out": _new_or(out), "out_history": _new_or(out_history), "motion": motion}
        return _temporal_result(self._frame_call(fn, A.TEMPORAL_HOST_MEMORY, d, table, W, H, planes, outs))

    def temporal_reproject(self, guides, prev_guides, prev_camera, prev_color, prev_history, max_history=float("inf"),
                           point_tolerance=TEMPORAL_POINT_TOLERANCE, normal_cos=TEMPORAL_NORMAL_COS, out=None, out_history=None,
                           motion=False, motions=None, prev_triangles=None, tri_first=0):
        """The reprojected history alone: temporal_accumulate (any of its three forms) with a plane of quiet NaNs for `color`,
        which the call drops -- `out` is prev_color fetched from where each texel lay under prev_camera (NaN where there is
        no history), out_history the fetched, capped history length (1 there).  What temporal_rectify takes as history /
        history_length; the luminance moments go through a call of their own, as with temporal_accumulate.
        numpy planes or torch tensors on this handle's device, as temporal_accumulate; for tensors the NaN plane is one
        tensor per frame size that the handle keeps."""
        given = (prev_color, prev_history, out, out_history, motion, *guides.values(), *prev_guides.values())
        if any(hasattr(v, "data_ptr") for v in given):
            import torch
            W, H = _frame_size(guides["normal"])
            cache = self.__dict__.setdefault("_nan_planes", {})
            if (H, W) not in cache:
                cache[(H, W)] = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device=torch.device("cuda", self.device))
            color = cache[(H, W)]
        else:
            color = _nan_plane(guides)
        return self.temporal_accumulate(guides, prev_guides, prev_camera, prev_color, prev_history, color, max_history, point_tolerance,
                                        normal_cos, out, out_history, motion, motions, prev_triangles, tri_first)

    def temporal_rectify(self, color, history, history_length, object=None, radius=RECTIFY_RADIUS, clip_sigma=RECTIFY_CLIP_SIGMA,
                         clip_history=RECTIFY_CLIP_HISTORY, moments=None, history_moments=None, out=None, out_history=None,
                         out_moments=None, clipped=False):
        """History rectification (rt_temporal_rectify; include/rt_abi.h has the definition): temporal_accumulate's blend with
        variance clipping in front, for lighting that changes.  `history` (H, W, 4) / `history_length` (H, W) are what
        temporal_reproject returned for this frame, `color` (H, W, 4) the frame itself.  Each texel's history is clamped,
        per colour channel, into mean +- `clip_sigma` standard deviations of the colours of `color` in the (2 radius + 1)^2
        window around it (`radius` 1 .. 3; with `object`, the G-buffer's (H, W) object words, only the window's texels of
        the texel's own object), and a texel that was clamped keeps at most `clip_history` frames of its history; then the
        frame is blended in at 1 / (length + 1).  clip_sigma=inf is temporal_accumulate itself, bit for bit.
        `moments` / `history_moments` (H, W, 4; both or neither): this frame's luminance_moments and their reprojection,
        blended with the texel's weight, never clipped.
        Returns (out, out_history), then out_moments with the moments, then with clipped=True (or an (H, W) uint8 array /
        tensor to fill) the plane that says 0 = no history, 1 = kept, 2 = clipped.  out may be history, out_history
        history_length and out_moments history_moments; out must not be color.
        What it cannot see: a change that stays inside the new frame's noise -- a lamp that gets brighter widens the box
        with its own noise.
        numpy planes: a synchronous call that returns numpy.  Torch tensors on this handle's device: an asynchronous call
        ordered after the current torch stream's work, as render_gbuffer(device=True) orders itself; returns tensors; there
        color=None takes the handle's image as the frame (read only: out must not be the image)."""
        d, planes, outs, W, H = _rectify_call(color, history, history_length, object, radius, clip_sigma, clip_history, moments,
                                              history_moments, out, out_history, out_moments, clipped)
        return _rectify_result(self._frame_call("rt_temporal_rectify", A.RECTIFY_HOST_MEMORY, d, A.RECTIFY_PLANES, W, H, planes, outs))

    def upsample(self, lo_guides, guides, color=None, point_tolerance=UPSAMPLE_POINT_TOLERANCE, normal_cos=UPSAMPLE_NORMAL_COS,
                 out=None, coverage=False):
        """Guided upsampling (rt_upsample; include/rt_abi.h has the definition): the (h, w, 4) float32 frame `color`, traced at
        a low resolution, carried onto the G-buffer of a higher one by a joint bilateral filter -- every high texel takes the
        bilinear taps of the low frame that lie on its own surface (same object, near its tangent plane, a similar normal),
        a wider ring of sixteen where none of the four does, and the nearest low texel where that fails too.
        `lo_guides`, `guides`: the dicts render_gbuffer returns at the two sizes under the same camera; lo_guides must hold
        `point`, `normal` and `object`, guides also `depth`; `albedo` (in both or in neither: the radiance is carried
        demodulated and takes the high texel's albedo) and guides' `emission` (lamps are not guided) are used when
        present.  `point_tolerance` is the distance off the high texel's tangent plane a tap may lie, per unit of depth;
        `normal_cos` the least cosine between the two normals.  Any pair of sizes is allowed.
        Returns the (H, W, 4) frame, or with coverage=True (or an (H, W) uint8 array / tensor to fill) (out, coverage): 2
        where the four taps served, 1 where the wider ring did, 0 for a hole -- texels a caller may want to trace itself
        (radiance, with guides["dir"] and pixel_seeds).
        numpy planes: a synchronous call that returns numpy.  Torch tensors on this handle's device: an asynchronous call
        ordered after the current torch stream's work, as render_gbuffer(device=True) orders itself; returns tensors; there
        color=None takes the handle's image -- what render left at the low size -- as the low frame."""
        d, table, planes, W, H = _upsample_call(lo_guides, guides, color, point_tolerance, normal_cos)
        tensors = any(hasattr(v, "data_ptr") for v in (*planes.values(), out, coverage))
        if not tensors and color is None:
            raise ValueError("color is required with numpy planes (color=None names the device image)")
        return _upsample_result(self._frame_call("rt_upsample", A.UPSAMPLE_HOST_MEMORY, d, table, W, H, planes,
                                                 {"out": _new_or(out), "coverage": coverage}))

    def _image_call_tensor(self, shape, dtype):
        """An output tensor of a call that takes the handle's image and was given no tensor: it makes the call a device call."""
        import torch
        return torch.empty(shape, dtype=dtype, device=torch.device("cuda", self.device))

    def display(self, color=None, *, tone="clamp", transfer="srgb", bgra=False, top_first=False, exposure=1.0, white=float("inf"),
                exposure_scale=None, out=None, width=None, height=None):
        """The display pass (rt_display; include/rt_abi.h has the definition): the (H, W, 4) float32 frame `color` as
        (H, W, 4) uint8 -- each colour channel times `exposure` (times `exposure_scale`, the one float auto_exposure
        returns), through the tone curve (`tone`: "clamp", or "reinhard" with the luminance `white` that maps to 1) and
        the transfer (`transfer`: "srgb" for the exact 8-bit sRGB encoding, "linear" for a surface that encodes itself);
        alpha is quantised as it is.  `bgra` stores B, G, R, A; `top_first` stores the top row of the view first (the
        image's row 0 is the bottom).  The defaults with bgra=True are what the reference's window shows.
        numpy planes: a synchronous call that returns numpy.  Torch tensors on this handle's device: an asynchronous call
        ordered after the current torch stream's work; returns a tensor; there color=None takes the handle's image
        (width x height texels of it, or the size of a given `out`), and an exposure_scale tensor is read on the device."""
        d, planes, W, H = _display_call(color, width, height, out, exposure_scale,
                                        dict(tone=tone, transfer=transfer, bgra=bgra, top_first=top_first, exposure=exposure, white=white))
        if color is None and out is None:
            import torch
            out = self._image_call_tensor((H, W, 4), torch.uint8)
        if color is None and "exposure_scale" in planes and not hasattr(planes["exposure_scale"], "data_ptr"):
            raise ValueError("with color=None (the device image) exposure_scale must be a tensor; a number goes into `exposure`")
        return self._frame_call("rt_display", A.DISPLAY_HOST_MEMORY, d, A.DISPLAY_PLANES, W, H, planes, {"out": _new_or(out)})["out"]

    def auto_exposure(self, color=None, *, low_permille=AUTO_EXPOSURE_LOW, high_permille=AUTO_EXPOSURE_HIGH, key=AUTO_EXPOSURE_KEY,
                      min_scale=AUTO_EXPOSURE_MIN, max_scale=AUTO_EXPOSURE_MAX, rate=1.0, prev_scale=None, histogram=False, scale=None,
                      width=None, height=None):
        """The exposure meter (rt_auto_exposure; include/rt_abi.h has the definition): a histogram of the frame's luminance
        over 256 logarithmic bins (eight per octave, 2^-16 .. 2^16), trimmed to the ranks [low_permille, high_permille) per
        thousand, and from its mean the one float that, as display's exposure_scale, brings that mean to `key` -- clamped to
        [min_scale, max_scale], and with `prev_scale` (the last frame's) moved only `rate` of the way from it.  Returns the
        scale as a (1,) float32 array or tensor, or with histogram=True (or a (256,) uint32 array / int32 tensor to fill)
        (scale, histogram) with the untrimmed counts.
        numpy planes: a synchronous call.  Torch tensors on this handle's device: asynchronous, nothing comes to the host --
        display(exposure_scale=...) reads the float in stream order; there color=None meters the handle's image (width x
        height texels of it).  `scale` may be the prev_scale tensor."""
        d, planes, W, H = _auto_exposure_call(color, width, height, low_permille, high_permille, key, min_scale, max_scale, rate, prev_scale)
        if color is None and scale is None:
            import torch
            scale = self._image_call_tensor((1,), torch.float32)
        if color is None and "prev_scale" in planes and not hasattr(planes["prev_scale"], "data_ptr"):
            raise ValueError("with color=None (the device image) prev_scale must be a tensor")
        return _auto_exposure_result(self._frame_call("rt_auto_exposure", A.AUTO_EXPOSURE_HOST_MEMORY, d, A.AUTO_EXPOSURE_PLANES, W, H, planes,
                                                      {"scale": _new_or(scale), "histogram": histogram}))

    def radiance(self, origins, dirs, seeds, bounces, samples, skybox=True):
        """Radiance along rays of the caller's (rt_radiance_rays): for ray i `frag`'s sample loop with the ray held fixed --
        state = seeds[i]; per sample four draws (the camera jitter's) and total += trace(ray); total / samples -- as an
        (n, 4) float32 array.  With origin = cam_to_world[3], dirs = the `dir` plane of render_gbuffer and
        seeds = pixel_seeds(width, height, frames) that is the frame render writes for frames <= 0 under a jitter-free
        camera, bit for bit.  numpy inputs (origins, dirs: (n, 3) floats; seeds: (n,) uint32): a synchronous call that
        returns numpy.  Tensors on this handle's device (origins, dirs: (n, 3) float32; seeds: (n,) int32 holding the
        u32 bits, or uint32): an asynchronous call ordered after the current torch stream's work, returns a tensor.
        Invalid rays (non-finite components, a direction that cannot be normalised) get zeros."""
        bounces, samples = int(bounces), int(samples)
        if bounces < 0:
            raise ValueError("bounces must be >= 0")
        if samples < 1:
            raise ValueError("samples must be >= 1")
        params = A.make_params(0, 0, bounces, samples, skybox=1 if skybox else 0)
        if any(hasattr(v, "data_ptr") for v in (origins, dirs, seeds)):
            import torch
            if not all(isinstance(v, torch.Tensor) for v in (origins, dirs, seeds)):
                raise ValueError("mix of device tensors and host arrays")
            for v in (origins, dirs, seeds):
                if v.device.type != "cuda" or v.device.index != self.device:
                    raise ValueError(f"ray tensors must be on cuda:{self.device}, not {v.device}")
            if origins.dtype != torch.float32 or dirs.dtype != torch.float32:
                raise ValueError("origins and dirs must be float32 tensors")
            if seeds.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
                raise ValueError(f"seeds must be an int32 (the u32 bits) or uint32 tensor, not {seeds.dtype}")
            if origins.dim() != 2 or origins.shape[1] != 3 or tuple(dirs.shape) != tuple(origins.shape):
                raise ValueError("origins and dirs must both have shape (n, 3)")
            n = origins.shape[0]
            if tuple(seeds.shape) != (n,):
                raise ValueError("seeds must have shape (n,)")
            bits = seeds.view(torch.int32).reshape(n, 1).view(torch.float32)
            pad = torch.zeros((n, 1), dtype=torch.float32, device=origins.device)   # (_p0 = 0)
            rays = torch.cat([origins, bits, dirs, pad], dim=1).contiguous()
            out = torch.empty((n, 4), dtype=torch.float32, device=origins.device)
            self._device_query(lambda h, r, m, o, f: self._L.rt_radiance_rays(h, C.byref(params), r, m, o, f), rays, out, 0)
            return out
        o, d, sd = np.asarray(origins), np.asarray(dirs), np.asarray(seeds)
        for name, v in (("origins", o), ("dirs", d)):
            if v.dtype.kind != "f":
                raise ValueError(f"{name} must be a floating-point array, not {v.dtype}")
        if sd.dtype != np.uint32:
            raise ValueError(f"seeds must be a uint32 array, not {sd.dtype}")
        if o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape:
            raise ValueError("origins and dirs must both have shape (n, 3)")
        n = o.shape[0]
        if sd.shape != (n,):
            raise ValueError("seeds must have shape (n,)")
        rays = np.zeros(n, A.PATH_RAY_DTYPE)
        rays["origin"] = o
        rays["dir"] = d
        rays["seed"] = sd
        out = np.zeros((n, 4), np.float32)
        if n:
            self._check(self._L.rt_radiance_rays(self._h, C.byref(params), rays.ctypes.data, n, out.ctypes.data,
                                                 A.RADIANCE_HOST_MEMORY))
        return out

    @staticmethod
    def hits_to_numpy(hits):
        """rt_hit records of trace_rays' device path -> numpy structured array of HIT_DTYPE (synchronises)."""
        return np.ascontiguousarray(hits.cpu().numpy()).view(A.HIT_DTYPE).reshape(-1)

    def _query_rays(self, origins, dirs, tmax):
        """Packs rt_ray records: (numpy (n, 8) f32 view, False) or (torch (n, 8) f32 tensor on this device, True)."""
        dev = hasattr(origins, "data_ptr") or hasattr(dirs, "data_ptr") or hasattr(tmax, "data_ptr")
        if dev:
            import torch
            ts = [t for t in (origins, dirs, tmax) if t is not None]
            if not all(isinstance(t, torch.Tensor) for t in ts if not np.isscalar(t)) or any(isinstance(t, np.ndarray) for t in ts):
                raise ValueError("mix of device tensors and host arrays")
            for t in ts:
                if isinstance(t, torch.Tensor):
                    if t.dtype != torch.float32:
                        raise ValueError(f"ray tensors must be float32, not {t.dtype}")
                    if t.device.type != "cuda" or t.device.index != self.device:
                        raise ValueError(f"ray tensors must be on cuda:{self.device}, not {t.device}")
            if origins.dim() != 2 or origins.shape[1] != 3 or tuple(dirs.shape) != tuple(origins.shape):
                raise ValueError("origins and dirs must both have shape (n, 3)")
            n = origins.shape[0]
            if tmax is None:
                tm = torch.full((n, 1), float("inf"), dtype=torch.float32, device=origins.device)
            elif isinstance(tmax, torch.Tensor):
                if tmax.dim() == 0:
                    tm = tmax.reshape(1, 1).expand(n, 1)
                elif tuple(tmax.shape) == (n,):
                    tm = tmax.reshape(n, 1)
                else:
                    raise ValueError("tmax must be a scalar or have shape (n,)")
            else:
                tm = torch.full((n, 1), float(tmax), dtype=torch.float32, device=origins.device)
            pad = torch.zeros((n, 1), dtype=torch.float32, device=origins.device)   # (_p0 = 0: +0.0 bits)
            return torch.cat([origins, tm, dirs, pad], dim=1).contiguous(), True
        o, d = np.asarray(origins), np.asarray(dirs)
        for name, v in (("origins", o), ("dirs", d)):
            if v.dtype.kind != "f":
                raise ValueError(f"{name} must be a floating-point array, not {v.dtype}")
        if o.ndim != 2 or o.shape[1] != 3 or d.shape != o.shape:
            raise ValueError("origins and dirs must both have shape (n, 3)")
        n = o.shape[0]
        rays = np.zeros(n, A.RAY_DTYPE)
        rays["origin"] = o
        rays["dir"] = d
        if tmax is None:
            rays["tmax"] = np.inf
        else:
            t = np.asarray(tmax)
            if t.dtype.kind not in "fiu":
                raise ValueError(f"tmax must be numeric, not {t.dtype}")
            if t.ndim != 0 and t.shape != (n,):
                raise ValueError("tmax must be a scalar or have shape (n,)")
            rays["tmax"] = t
        return rays, False

    def _device_query(self, fn, rays, out, flags):
        """Runs fn on the handle's stream, ordered after the current torch stream's work and before what follows on it."""
        n = rays.shape[0]
        if n:
            self._on_handle_stream(lambda: self._check(fn(self._h, rays.data_ptr(), n, out.data_ptr(), flags)))

    def stats(self):
        s = A.Stats()
        self._check(self._L.rt_get_stats(self._h, C.byref(s)))
        return s

    def last_launch(self):
        """Shape of the last render launch: dynamic LDS bytes per workgroup, workgroups, scene staged in LDS, kernel flags."""
        out = (C.c_uint32 * 6)()
        self._check(self._L.rt_last_launch(self._h, C.byref(out)))
        return {"lds_bytes_per_workgroup": out[0], "workgroups": out[1], "scene_in_lds": bool(out[2]),
                "many_mesh": bool(out[3] & 1), "specialised": bool(out[3] & 2), "one_wave_per_tile": bool(out[3] & 4),
                "deferred_walks": bool(out[3] & 8), "wavefront": bool(out[3] & 16), "fixed_switches": bool(out[3] & 32),
                "device_mb_held": out[4], "device_mb_cap": out[5]}

    @property
    def device_image_ptr(self):
        return self._L.rt_device_image(self._h)

    @property
    def stream_ptr(self):
        return self._L.rt_stream(self._h)

    def strip_texels(self, width, height, rank, world):
        return int(self._L.rt_strip_texels(width, height, rank, world))


def pixel_seeds(width, height, frames):
    """The RNG seeds of a width x height frame's pixels (wgsl:475: y * width + x + |frames| * 719393 in u32 arithmetic),
    row-major, as a (width * height,) uint32 array: RayTracer.radiance's `seeds` for the rays of that frame."""
    width, height, frames = int(width), int(height), int(frames)
    i = np.arange(width * height, dtype=np.uint64)
    return ((i + np.uint64(abs(frames)) * np.uint64(719393)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def normalize3_f32(v):
    """The kernels' normalize3 in binary32: v * (1 / sqrt((x*x + y*y) + z*z)), every operation rounded.
    The directions a render traces are outputs of it; a zero or non-finite vector gives non-finite components."""
    v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = np.float32(1.0) / np.sqrt((x * x + y * y) + z * z)
        return (v * r[:, None]).astype(np.float32)


def render_multi(tracers, params, read_back=True, n_frames=1):
    """rt_render_multi(_frames) over a list of RayTracer (one per device, same scene on each):
    returns the assembled frame (H, W, 4) f32 when read_back, else None (non-blocking)."""
    L = load()
    arr = (C.c_void_p * len(tracers))(*[t._h for t in tracers])
    out = np.empty((params.height, params.width, 4), np.float32) if read_back else None
    rc = L.rt_render_multi_frames(arr, len(tracers), C.byref(params), n_frames, out.ctypes.data if read_back else None)
    if rc < 0:
        raise RtError(rc, L.rt_last_error(tracers[0]._h).decode())
    return out


def read_multi_frame(root, width, height):
    """The frame the last render_multi call assembled on the root (blocking)."""
    L = load()
    out = np.empty((height, width, 4), np.float32)
    rc = L.rt_read_multi_frame(root._h, out.ctypes.data, out.nbytes)
    if rc < 0:
        raise RtError(rc, L.rt_last_error(root._h).decode())
    return out
