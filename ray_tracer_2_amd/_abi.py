"""ctypes / numpy mirror of include/rt_abi.h (section 1: the data contract).

Every structure is byte-identical to the `#[repr(C)]` struct the reference
uploads to its shader (citations in rt_abi.h).  `check_sizes()` compares these
against the sizes the loaded C library reports (rt_abi_sizes).
"""
import ctypes as C

import numpy as np

f32, u32, i32 = C.c_float, C.c_uint32, C.c_int32


class Params(C.Structure):  # src/core/app.rs:27-40
    _fields_ = [("width", u32), ("height", u32), ("number_of_bounces", i32),
                ("rays_per_pixel", i32), ("skybox", i32), ("frames", i32),
                ("accumulate", i32), ("debug_flag", i32), ("debug_scale", i32),
                ("_p1", f32 * 3)]


class Material(C.Structure):  # src/scene/components/material.rs:3-18
    _fields_ = [("color", f32 * 4), ("emission_color", f32 * 4), ("specular_color", f32 * 4),
                ("absorption", f32 * 4), ("absorption_strength", f32),
                ("emission_strength", f32), ("smoothness", f32), ("specular", f32),
                ("ior", f32), ("flag", i32), ("diffuse_index", i32), ("normal_index", i32)]


class Sphere(C.Structure):  # geometry/sphere.rs:4-10
    _fields_ = [("pos", f32 * 3), ("radius", f32), ("material", Material)]


class MeshUniform(C.Structure):  # geometry/mesh.rs:52-62
    _fields_ = [("world_to_model", (f32 * 4) * 4), ("model_to_world", (f32 * 4) * 4),
                ("node_offset", u32), ("triangles", u32), ("triangle_offset", u32),
                ("_p1", f32), ("material", Material)]


class Node(C.Structure):  # src/core/bvh.rs:55-66
    _fields_ = [("left", u32), ("right", u32), ("first", u32), ("count", u32),
                ("aabb_min", f32 * 3), ("_p1", f32), ("aabb_max", f32 * 3), ("_p2", f32)]


class PackedTriangle(C.Structure):  # src/core/bvh.rs:19-34
    _fields_ = [("v1", f32 * 3), ("uv10", f32), ("v2", f32 * 3), ("uv11", f32),
                ("v3", f32 * 3), ("uv20", f32), ("n1", f32 * 3), ("uv21", f32),
                ("n2", f32 * 3), ("uv30", f32), ("n3", f32 * 3), ("uv31", f32)]


class CameraUniform(C.Structure):  # src/scene/camera.rs:15-22
    _fields_ = [("cam_to_world", (f32 * 4) * 4), ("view_params", f32 * 3),
                ("defocus_strength", f32), ("diverge_strength", f32)]


class SceneUniform(C.Structure):  # src/scene/scene.rs:1016-1026
    _fields_ = [("spheres", u32), ("n_vertices", u32), ("n_indices", u32), ("meshes", u32),
                ("camera", CameraUniform), ("nodes", u32), ("padding", f32 * 6)]


class TextureDesc(C.Structure):
    _fields_ = [("rgba8", C.c_void_p), ("width", u32), ("height", u32)]


class Transform(C.Structure):  # components/transform.rs:3-8
    _fields_ = [("pos", f32 * 3), ("rot", f32 * 4), ("scale", f32 * 3)]

    @staticmethod
    def identity():
        return Transform((f32 * 3)(0, 0, 0), (f32 * 4)(0, 0, 0, 1), (f32 * 3)(1, 1, 1))


class CameraDesc(C.Structure):  # CameraDescriptor, camera.rs:38-66
    _fields_ = [("transform", Transform), ("fov", f32), ("aspect", f32), ("near_plane", f32),
                ("far_plane", f32), ("focus_dist", f32), ("defocus_strength", f32),
                ("diverge_strength", f32)]


class Stats(C.Structure):
    _fields_ = [("segments", C.c_uint64), ("paths", C.c_uint64), ("node_tests", C.c_uint64),
                ("triangle_tests", C.c_uint64), ("kernel_ms", f32), ("launches", u32), ("frames", u32), ("segments_reused", C.c_uint64),
                ("frames_speculative", u32), ("_reserved", u32)]


class Ray(C.Structure):  # rt_ray: a ray query's input
    _fields_ = [("origin", f32 * 3), ("tmax", f32), ("dir", f32 * 3), ("_p0", u32)]


class Hit(C.Structure):  # rt_hit: a ray query's closest-hit record
    _fields_ = [("t", f32), ("object", u32), ("primitive", u32), ("flags", u32), ("point", f32 * 3), ("bary_u", f32),
                ("normal", f32 * 3), ("bary_v", f32), ("tex_u", f32), ("tex_v", f32), ("_p1", f32 * 2)]


class PathRay(C.Structure):  # rt_path_ray: a radiance query's input
    _fields_ = [("origin", f32 * 3), ("seed", u32), ("dir", f32 * 3), ("_p0", u32)]


class GBuffer(C.Structure):  # rt_gbuffer: the planes rt_render_gbuffer writes (a NULL plane is not produced)
    _fields_ = [("struct_bytes", u32), ("_p0", u32), ("depth", C.c_void_p), ("dir", C.c_void_p), ("point", C.c_void_p),
                ("normal", C.c_void_p), ("bary", C.c_void_p), ("texcoord", C.c_void_p), ("albedo", C.c_void_p),
                ("emission", C.c_void_p), ("object", C.c_void_p), ("primitive", C.c_void_p), ("flags", C.c_void_p)]


# channel of rt_gbuffer -> (numpy dtype, components per texel; 0: a plane of shape (H, W))
GBUFFER_CHANNELS = {"depth": ("<f4", 0), "dir": ("<f4", 3), "point": ("<f4", 3), "normal": ("<f4", 3), "bary": ("<f4", 2),
                    "texcoord": ("<f4", 2), "albedo": ("<f4", 4), "emission": ("<f4", 4), "object": ("<u4", 0),
                    "primitive": ("<u4", 0), "flags": ("u1", 0)}
GBUFFER_HOST_MEMORY = 1


class DenoiseDesc(C.Structure):  # rt_denoise_desc: a frame and its guides for rt_denoise / rt_denoise_host
    _fields_ = [("struct_bytes", u32), ("_p0", u32), ("width", u32), ("height", u32), ("iterations", u32),
                ("sigma_color", f32), ("sigma_normal", f32), ("sigma_point", f32), ("color", C.c_void_p),
                ("normal", C.c_void_p), ("point", C.c_void_p), ("albedo", C.c_void_p), ("emission", C.c_void_p),
                ("out", C.c_void_p)]


# The plane tables of the frame passes, in the order of their desc's fields:
# plane -> (numpy dtype, components per texel; 0: a plane of shape (H, W))
DENOISE_PLANES = {"color": ("<f4", 4), "normal": ("<f4", 3), "point": ("<f4", 3), "albedo": ("<f4", 4), "emission": ("<f4", 4),
                  "out": ("<f4", 4)}
DENOISE_HOST_MEMORY = 1


class VDenoiseDesc(C.Structure):  # rt_vdenoise_desc: a frame, its guides and its luminance moments for rt_denoise_variance / rt_luminance_moments
    _fields_ = [("struct_bytes", u32), ("_p0", u32), ("width", u32), ("height", u32), ("iterations", u32),
                ("sigma_luminance", f32), ("sigma_normal", f32), ("sigma_point", f32), ("min_history", f32), ("_p1", u32),
                ("color", C.c_void_p), ("normal", C.c_void_p), ("point", C.c_void_p), ("albedo", C.c_void_p),
                ("emission", C.c_void_p), ("moments", C.c_void_p), ("history", C.c_void_p), ("out", C.c_void_p),
                ("out_variance", C.c_void_p)]


VDENOISE_PLANES = {"color": ("<f4", 4), "normal": ("<f4", 3), "point": ("<f4", 3), "albedo": ("<f4", 4), "emission": ("<f4", 4),
                   "moments": ("<f4", 4), "history": ("<f4", 0), "out": ("<f4", 4), "out_variance": ("<f4", 0)}
VDENOISE_HOST_MEMORY = 1


class AdaptivePlanDesc(C.Structure):  # rt_adaptive_plan_desc: a variance plane and a ray budget for rt_adaptive_plan / rt_adaptive_plan_host
    _fields_ = [("struct_bytes", u32), ("_p0", u32), ("width", u32), ("height", u32), ("budget", u32), ("min_samples", u32),
                ("max_samples", u32), ("first_frame", u32), ("origin", f32 * 3), ("_p1", u32), ("variance", C.c_void_p),
                ("dir", C.c_void_p), ("counts", C.c_void_p), ("offsets", C.c_void_p), ("rays", C.c_void_p),
                ("totals", C.c_void_p)]


class AdaptiveMergeDesc(C.Structure):  # rt_adaptive_merge_desc: the traced samples and the accumulation for rt_adaptive_merge / rt_adaptive_merge_host
    _fields_ = [("struct_bytes", u32), ("_p0", u32), ("width", u32), ("height", u32), ("budget", u32), ("max_history", f32),
                ("radiance", C.c_void_p), ("counts", C.c_void_p), ("offsets", C.c_void_p), ("color", C.c_void_p),
                ("history", C.c_void_p), ("albedo", C.c_void_p), ("moments", C.c_void_p), ("out", C.c_void_p),
                ("out_history", C.c_void_p), ("out_moments", C.c_void_p)]


# the frame-shaped planes of the two descs; `rays` ((budget,) PATH_RAY_DTYPE), `totals` ((4,) uint32) and `radiance`
# ((budget, 4) float32) are not frame-shaped
ADAPTIVE_PLAN_PLANES = {"variance": ("<f4", 0), "dir": ("<f4", 3), "counts": ("<u4", 0), "offsets": ("<u4", 0)}
ADAPTIVE_MERGE_PLANES = {"counts": ("<u4", 0), "offsets": ("<u4", 0), "color": ("<f4", 4), "history": ("<f4", 0),
                         "albedo": ("<f4", 4), "moments": ("<f4", 4), "out": ("<f4", 4), "out_history": ("<f4", 0),
                         "out_moments": ("<f4", 4)}
ADAPTIVE_HOST_MEMORY = 1


class TemporalDesc(C.Structure):  # rt_temporal_desc: two frames for rt_temporal_accumulate / rt_temporal_accumulate_host
    _fields_ = [("struct_bytes", u32), ("_p0", u32), ("width", u32), ("height", u32), ("prev_camera", CameraUniform),
                ("max_history", f32), ("point_tolerance", f32), ("normal_cos", f32), ("color", C.c_void_p),
                ("point", C.c_void_p), ("normal", C.c_void_p), ("object", C.c_void_p), ("prev_color", C.c_void_p),
                ("prev_history", C.c_void_p), ("prev_point", C.c_void_p), ("prev_normal", C.c_void_p),
                ("prev_object", C.c_void_p), ("out", C.c_void_p), ("out_history", C.c_void_p), ("motion", C.c_void_p)]


TEMPORAL_PLANES = {"color": ("<f4", 4), "point": ("<f4", 3), "normal": ("<f4", 3), "object": ("<u4", 0),
                   "prev_color": ("<f4", 4), "prev_history": ("<f4", 0), "prev_point": ("<f4", 3), "prev_normal": ("<f4", 3),
                   "prev_object": ("<u4", 0), "out": ("<f4", 4), "out_history": ("<f4", 0), "motion": ("<f4", 2)}
TEMPORAL_HOST_MEMORY = 1


class ObjectMotion(C.Structure):  # rt_object_motion: one record of rt_temporal_accumulate_moving's table
    _fields_ = [("d", (f32 * 3) * 4), ("nt", (f32 * 3) * 3), ("moved", u32), ("_p", u32 * 2)]


class TemporalMotionDesc(C.Structure):  # rt_temporal_motion_desc: rt_temporal_desc's fields, then the motion table
    _fields_ = TemporalDesc._fields_ + [("motions", C.c_void_p), ("n_objects", u32), ("_p1", u32)]


# rt_temporal_accumulate_moving's planes: TEMPORAL_PLANES and the table, which is not frame-shaped -- (n_objects,)
# OBJECT_MOTION_DTYPE on the host, an (n_objects, 24) int32 tensor of the records' words on the device; the calls put its
# shape in
OBJECT_MOTION_DTYPE = np.dtype([("d", "<f4", (4, 3)), ("nt", "<f4", (3, 3)), ("moved", "<u4"), ("_p", "<u4", 2)])
assert OBJECT_MOTION_DTYPE.itemsize == C.sizeof(ObjectMotion) == 96
TEMPORAL_MOTION_PLANES = dict(TEMPORAL_PLANES, motions=(OBJECT_MOTION_DTYPE, None))
OBJECT_DEFORMED = 2   # rt_object_motion.moved of a mesh whose vertices moved (rt_temporal_accumulate_deforming)


class TemporalDeformDesc(C.Structure):  # rt_temporal_deform_desc: rt_temporal_motion_desc's fields, then the triangle side
    _fields_ = TemporalMotionDesc._fields_ + [("primitive", C.c_void_p), ("bary", C.c_void_p), ("flags", C.c_void_p),
                                              ("prev_triangles", C.c_void_p), ("tri_first", u32), ("n_prev_triangles", u32)]


class UpsampleDesc(C.Structure):  # rt_upsample_desc: a low frame and the G-buffers of both sizes for rt_upsample / rt_upsample_host
    _fields_ = [("struct_bytes", u32), ("_p0", u32), ("lo_width", u32), ("lo_height", u32), ("width", u32), ("height", u32),
                ("point_tolerance", f32), ("normal_cos", f32), ("lo_color", C.c_void_p), ("lo_point", C.c_void_p),
                ("lo_normal", C.c_void_p), ("lo_object", C.c_void_p), ("lo_albedo", C.c_void_p), ("depth", C.c_void_p),
                ("point", C.c_void_p), ("normal", C.c_void_p), ("object", C.c_void_p), ("albedo", C.c_void_p),
                ("emission", C.c_void_p), ("out", C.c_void_p), ("coverage", C.c_void_p)]


# rt_upsample's planes: those of the high frame are frame-shaped; the low frame's (lo_*) are not -- the calls put their
# shapes in, (h, w, n) or (h, w), as they do for the motion table
UPSAMPLE_PLANES = {"lo_color": ("<f4", None), "lo_point": ("<f4", None), "lo_normal": ("<f4", None), "lo_object": ("<u4", None),
                   "lo_albedo": ("<f4", None), "depth": ("<f4", 0), "point": ("<f4", 3), "normal": ("<f4", 3), "object": ("<u4", 0),
                   "albedo": ("<f4", 4), "emission": ("<f4", 4), "out": ("<f4", 4), "coverage": ("u1", 0)}
UPSAMPLE_LO_COMPONENTS = {"lo_color": 4, "lo_point": 3, "lo_normal": 3, "lo_object": 0, "lo_albedo": 4}
UPSAMPLE_HOST_MEMORY = 1
UPSAMPLE_RING1, UPSAMPLE_RING2, UPSAMPLE_HOLE = 2, 1, 0   # the bytes of `coverage`


class RectifyDesc(C.Structure):  # rt_rectify_desc: a frame, its reprojected history and the clipping rule for rt_temporal_rectify / rt_temporal_rectify_host
    _fields_ = [("struct_bytes", u32), ("_p0", u32), ("width", u32), ("height", u32), ("radius", u32), ("clip_sigma", f32),
                ("clip_history", f32), ("_p1", u32), ("color", C.c_void_p), ("history", C.c_void_p), ("history_length", C.c_void_p),
                ("object", C.c_void_p), ("moments", C.c_void_p), ("history_moments", C.c_void_p), ("out", C.c_void_p),
                ("out_history", C.c_void_p), ("out_moments", C.c_void_p), ("out_clipped", C.c_void_p)]


RECTIFY_PLANES = {"color": ("<f4", 4), "history": ("<f4", 4), "history_length": ("<f4", 0), "object": ("<u4", 0),
                  "moments": ("<f4", 4), "history_moments": ("<f4", 4), "out": ("<f4", 4), "out_history": ("<f4", 0),
                  "out_moments": ("<f4", 4), "out_clipped": ("u1", 0)}
RECTIFY_HOST_MEMORY = 1
RECTIFY_NO_HISTORY, RECTIFY_KEPT, RECTIFY_CLIPPED = 0, 1, 2   # the bytes of `out_clipped`


class DisplayDesc(C.Structure):  # rt_display_desc: a frame and how it becomes four bytes per texel, for rt_display / rt_display_host / rt_snapshot_display
    _fields_ = [("struct_bytes", u32), ("_p0", u32), ("width", u32), ("height", u32), ("tone", u32), ("transfer", u32), ("layout", u32),
                ("_p1", u32), ("exposure", f32), ("white", f32), ("color", C.c_void_p), ("exposure_scale", C.c_void_p), ("out", C.c_void_p)]


class AutoExposureDesc(C.Structure):  # rt_auto_exposure_desc: a frame and the meter's settings for rt_auto_exposure / rt_auto_exposure_host
    _fields_ = [("struct_bytes", u32), ("_p0", u32), ("width", u32), ("height", u32), ("low_permille", u32), ("high_permille", u32),
                ("key", f32), ("min_scale", f32), ("max_scale", f32), ("rate", f32), ("color", C.c_void_p), ("prev_scale", C.c_void_p),
                ("histogram", C.c_void_p), ("scale", C.c_void_p)]


# the planes of the two calls: `out` is four bytes per texel; the one-float planes and the histogram are not frame-shaped
DISPLAY_PLANES = {"color": ("<f4", 4), "exposure_scale": ("<f4", (1,)), "out": ("u1", 4)}
AUTO_EXPOSURE_PLANES = {"color": ("<f4", 4), "prev_scale": ("<f4", (1,)), "histogram": ("<u4", (256,)), "scale": ("<f4", (1,))}
DISPLAY_HOST_MEMORY = AUTO_EXPOSURE_HOST_MEMORY = 1
DISPLAY_TONE_CLAMP, DISPLAY_TONE_REINHARD = 0, 1
DISPLAY_SRGB, DISPLAY_LINEAR = 0, 1
DISPLAY_LAYOUT_BGRA, DISPLAY_LAYOUT_TOP_FIRST = 1, 2


EXPECTED_SIZES = {Params: 48, Material: 96, Sphere: 112, MeshUniform: 240, Node: 48,
                  PackedTriangle: 96, CameraUniform: 84, SceneUniform: 128}
for _t, _s in EXPECTED_SIZES.items():
    assert C.sizeof(_t) == _s, (_t, C.sizeof(_t), _s)

# numpy views of the array types (for fixtures and inspection)
NODE_DTYPE = np.dtype([("left", "<u4"), ("right", "<u4"), ("first", "<u4"), ("count", "<u4"),
                       ("aabb_min", "<f4", 3), ("_p1", "<f4"), ("aabb_max", "<f4", 3),
                       ("_p2", "<f4")])
TRI_DTYPE = np.dtype([("v1", "<f4", 3), ("uv10", "<f4"), ("v2", "<f4", 3), ("uv11", "<f4"),
                      ("v3", "<f4", 3), ("uv20", "<f4"), ("n1", "<f4", 3), ("uv21", "<f4"),
                      ("n2", "<f4", 3), ("uv30", "<f4"), ("n3", "<f4", 3), ("uv31", "<f4")])
MATERIAL_DTYPE = np.dtype([("color", "<f4", 4), ("emission_color", "<f4", 4),
                           ("specular_color", "<f4", 4), ("absorption", "<f4", 4),
                           ("absorption_strength", "<f4"), ("emission_strength", "<f4"),
                           ("smoothness", "<f4"), ("specular", "<f4"), ("ior", "<f4"),
                           ("flag", "<i4"), ("diffuse_index", "<i4"), ("normal_index", "<i4")])
MESH_DTYPE = np.dtype([("world_to_model", "<f4", (4, 4)), ("model_to_world", "<f4", (4, 4)),
                       ("node_offset", "<u4"), ("triangles", "<u4"), ("triangle_offset", "<u4"),
                       ("_p1", "<f4"), ("material", MATERIAL_DTYPE)])
SPHERE_DTYPE = np.dtype([("pos", "<f4", 3), ("radius", "<f4"), ("material", MATERIAL_DTYPE)])
assert NODE_DTYPE.itemsize == 48 and TRI_DTYPE.itemsize == 96
# rt_temporal_accumulate_deforming's planes: TEMPORAL_MOTION_PLANES, the G-buffer's primitive, bary and flags planes of the
# current frame and the previous triangles, which are not frame-shaped -- (n,) TRI_DTYPE on the host, an (n, 24) float32
# tensor on the device, as refit_triangles takes them; the calls put the shape in
TEMPORAL_DEFORM_PLANES = dict(TEMPORAL_MOTION_PLANES, primitive=("<u4", 0), bary=("<f4", 2), flags=("u1", 0),
                              prev_triangles=(TRI_DTYPE, None))
assert MESH_DTYPE.itemsize == 240 and SPHERE_DTYPE.itemsize == 112
RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("tmax", "<f4"), ("dir", "<f4", 3), ("_p0", "<u4")])
HIT_DTYPE = np.dtype([("t", "<f4"), ("object", "<u4"), ("primitive", "<u4"), ("flags", "<u4"), ("point", "<f4", 3),
                      ("bary_u", "<f4"), ("normal", "<f4", 3), ("bary_v", "<f4"), ("tex_u", "<f4"), ("tex_v", "<f4"),
                      ("_p1", "<f4", 2)])
assert RAY_DTYPE.itemsize == C.sizeof(Ray) == 32 and HIT_DTYPE.itemsize == C.sizeof(Hit) == 64
PATH_RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("seed", "<u4"), ("dir", "<f4", 3), ("_p0", "<u4")])
assert PATH_RAY_DTYPE.itemsize == C.sizeof(PathRay) == 32
HIT_HIT, HIT_BACKFACE = 1, 2
QUERY_HOST_MEMORY, QUERY_PRUNE_TMAX = 1, 2
REFIT_HOST_MEMORY = 1
RADIANCE_HOST_MEMORY = 1
MISS = 0xFFFFFFFF

# SceneLayout (csrc/rt_scene_format.h): the 12 words rt_test_scene_blob returns; the head of the blob is [0, wide_off)
SCENE_LAYOUT_FIELDS = ("mesh_off", "wide_off", "tri_off", "shade_off", "mat_off", "sphere_off", "item_off", "tlas_off",
                       "forest_off", "bytes", "_pad0", "_pad1")

# the fact words of rt_test_pack_scene (include/rt_test_abi.h), in order
PACK_FACT_FIELDS = ("n_items", "n_tlas_records", "n_forest_entries", "tlas_entries", "has_tlas", "has_forest", "plain_materials",
                    "have_defer", "defer_mesh", "defer_xform", "defer_internal", "max_height", "max_leaf_ref",
                    "top_mesh_records", "top_mesh_base", "roots_are_unions", "any_deep", "rerun_same")
# item kinds and record flags of the blob (csrc/rt_scene_format.h)
ITEM_TLAS, ITEM_NEW_XFORM, ITEM_FOREST, ITEM_FLAT2, ITEM_DEFER, ITEM_DEFER_CULL, ITEM_PRUNE = 1, 2, 4, 8, 16, 32, 64
DMESH_GLASS, DMESH_DEEP, FOREST_CULLABLE, TLAS_REF_GLASS = 2, 4, 0x100, 0x40000000

RT_OK = 0
MATERIAL_DEFAULT, MATERIAL_GLASS, MATERIAL_TEXTURE = 0, 1, 2


def make_params(width, height, bounces, spp, skybox=1, frames=0, accumulate=1, debug_flag=0,
                debug_scale=0):
    return Params(width, height, bounces, spp, skybox, frames, accumulate, debug_flag,
                  debug_scale, (f32 * 3)(0, 0, 0))
