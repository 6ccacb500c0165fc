// temporal_deform_driver.cpp -- rt_temporal_accumulate_deforming_host's restatement (csrc/host/temporal.cpp:
// rt2::temporal_deform_host) under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own
// (tests/test_temporal_deform_host.py builds and runs it; it is never loaded into Python).
//
//   temporal_deform_driver CASE OUT
//
// CASE: five u32 (width, height, n_objects, n_prev_triangles, tri_first), an rt_camera_uniform, three floats (max_history,
// point_tolerance, normal_cos), then the planes color, point, normal, object, prev_color, prev_history, prev_point,
// prev_normal, prev_object, primitive, bary, flags, the motion table and the previous triangles.  Every array goes into a heap
// block of exactly its size, so that a read or write one element outside it is reported.  OUT receives out, out_history and
// motion.  Then a 1 x 1 frame, made here: one deformed texel that takes its own history, and the same texel with its
// primitive word one past the range.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../ray_tracer_2_amd/csrc/rt_temporal_api.h"

namespace {

template <class T>
std::unique_ptr<T[]> block(FILE* f, size_t n) {
    std::unique_ptr<T[]> p(new T[n]);
    if (f && fread(p.get(), sizeof(T), n, f) != n) {
        fprintf(stderr, "short read\n");
        exit(2);
    }
    return p;
}

int fail(const char* what, const std::string& err) {
    fprintf(stderr, "%s: %s\n", what, err.c_str());
    return 1;
}

int one_texel() {
    rt_temporal_deform_desc d{};
    d.struct_bytes = sizeof(d);
    d.width = d.height = 1;
    for (int i = 0; i < 4; ++i) d.prev_camera.cam_to_world[i][i] = 1.0f;
    d.prev_camera.view_params[0] = 1.2f;
    d.prev_camera.view_params[1] = 0.8f;
    d.prev_camera.view_params[2] = 1.5f;
    d.max_history = 8.0f;
    d.point_tolerance = 0.01f;
    d.normal_cos = 0.9f;
    auto color = block<float>(nullptr, 4), point = block<float>(nullptr, 3), normal = block<float>(nullptr, 3);
    auto prev_color = block<float>(nullptr, 4), prev_history = block<float>(nullptr, 1), prev_point = block<float>(nullptr, 3);
    auto prev_normal = block<float>(nullptr, 3), out = block<float>(nullptr, 4), out_history = block<float>(nullptr, 1);
    auto motion = block<float>(nullptr, 2), bary = block<float>(nullptr, 2);
    auto object = block<uint32_t>(nullptr, 1), prev_object = block<uint32_t>(nullptr, 1), primitive = block<uint32_t>(nullptr, 1);
    auto flags = block<uint8_t>(nullptr, 1);
    auto motions = block<rt_object_motion>(nullptr, 1);
    auto tris = block<rt_packed_triangle>(nullptr, 1);
    for (int k = 0; k < 4; ++k) color[k] = 1.0f, prev_color[k] = 3.0f;
    // the G-buffer's point and normal of the deformed texel: somewhere else, facing elsewhere
    point[0] = 0.5f, point[1] = 0.25f, point[2] = 2.0f;
    normal[0] = 0.0f, normal[1] = 1.0f, normal[2] = 0.0f;
    prev_point[0] = 0.0f, prev_point[1] = 0.0f, prev_point[2] = 3.0f;
    prev_normal[0] = 0.0f, prev_normal[1] = 0.0f, prev_normal[2] = -1.0f;
    prev_history[0] = 3.0f;
    object[0] = prev_object[0] = 0u;
    primitive[0] = 7u;
    bary[0] = 0.25f, bary[1] = 0.5f;
    flags[0] = 1u | 2u;   // a backface hit: the triangle's normals point away
    std::memset(motions.get(), 0, sizeof(rt_object_motion));
    for (int r = 0; r < 3; ++r) motions[0].d[r][r] = motions[0].nt[r][r] = 1.0f;
    motions[0].moved = 2u;
    std::memset(tris.get(), 0, sizeof(rt_packed_triangle));
    // a triangle in the plane z = 3 whose point (u, v) = (0.25, 0.5) is the origin of that plane
    const float v1[3] = {-1.0f, -2.0f, 3.0f}, v2[3] = {4.0f, 0.0f, 3.0f}, v3[3] = {-1.5f, 1.0f, 3.0f};
    for (int r = 0; r < 3; ++r) tris[0].v1[r] = v1[r], tris[0].v2[r] = v2[r], tris[0].v3[r] = v3[r];
    tris[0].n1[2] = tris[0].n2[2] = tris[0].n3[2] = 2.0f;
    d.color = color.get(), d.point = point.get(), d.normal = normal.get(), d.object = object.get();
    d.prev_color = prev_color.get(), d.prev_history = prev_history.get(), d.prev_point = prev_point.get();
    d.prev_normal = prev_normal.get(), d.prev_object = prev_object.get();
    d.out = out.get(), d.out_history = out_history.get(), d.motion = motion.get();
    d.motions = motions.get(), d.n_objects = 1;
    d.primitive = primitive.get(), d.bary = bary.get(), d.flags = flags.get();
    d.prev_triangles = tris.get(), d.tri_first = 7u, d.n_prev_triangles = 1u;
    std::string err;
    if (rt2::temporal_deform_host(&d, err) != RT_OK) return fail("1x1", err);
    // history 3 -> w = 1/4: 3 * 0.75 + 1 * 0.25 = 2.5, history 4, the texel's own position
    if (out_history[0] != 4.0f || out[0] != 2.5f || out[3] != 2.5f || motion[0] != 0.0f || motion[1] != 0.0f) {
        fprintf(stderr, "1x1: out %g history %g motion %g %g\n", out[0], out_history[0], motion[0], motion[1]);
        return 1;
    }
    primitive[0] = 8u;   // one past the range: the triangle array is not read
    if (rt2::temporal_deform_host(&d, err) != RT_OK) return fail("1x1 past the range", err);
    if (out_history[0] != 1.0f || out[0] != 1.0f || !std::isnan(motion[0]) || !std::isnan(motion[1])) {
        fprintf(stderr, "1x1 past the range: out %g history %g\n", out[0], out_history[0]);
        return 1;
    }
    primitive[0] = 6u;   // one below it
    if (rt2::temporal_deform_host(&d, err) != RT_OK) return fail("1x1 below the range", err);
    if (out_history[0] != 1.0f) return fail("1x1 below the range", "history kept");
    d.n_prev_triangles = 0u;
    if (rt2::temporal_deform_host(&d, err) != RT_ERR_INVALID_ARGUMENT || err.empty()) return fail("1x1", "an empty triangle range was accepted");
    printf("1x1 ok\n");
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: temporal_deform_driver CASE OUT\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return fail(argv[1], "cannot open");
    uint32_t head[5];
    rt_temporal_deform_desc d{};
    float numbers[3];
    if (fread(head, 4, 5, f) != 5 || fread(&d.prev_camera, sizeof(d.prev_camera), 1, f) != 1 || fread(numbers, 4, 3, f) != 3) return fail(argv[1], "short head");
    const size_t n = (size_t)head[0] * head[1];
    d.struct_bytes = sizeof(d);
    d.width = head[0], d.height = head[1], d.n_objects = head[2], d.n_prev_triangles = head[3], d.tri_first = head[4];
    d.max_history = numbers[0], d.point_tolerance = numbers[1], d.normal_cos = numbers[2];
    auto color = block<float>(f, 4 * n), point = block<float>(f, 3 * n), normal = block<float>(f, 3 * n);
    auto object = block<uint32_t>(f, n);
    auto prev_color = block<float>(f, 4 * n), prev_history = block<float>(f, n), prev_point = block<float>(f, 3 * n), prev_normal = block<float>(f, 3 * n);
    auto prev_object = block<uint32_t>(f, n), primitive = block<uint32_t>(f, n);
    auto bary = block<float>(f, 2 * n);
    auto flags = block<uint8_t>(f, n);
    auto motions = block<rt_object_motion>(f, d.n_objects);
    auto tris = block<rt_packed_triangle>(f, d.n_prev_triangles);
    fclose(f);
    auto out = block<float>(nullptr, 4 * n), out_history = block<float>(nullptr, n), motion = block<float>(nullptr, 2 * n);
    d.color = color.get(), d.point = point.get(), d.normal = normal.get(), d.object = object.get();
    d.prev_color = prev_color.get(), d.prev_history = prev_history.get(), d.prev_point = prev_point.get();
    d.prev_normal = prev_normal.get(), d.prev_object = prev_object.get();
    d.out = out.get(), d.out_history = out_history.get(), d.motion = motion.get();
    d.motions = motions.get(), d.primitive = primitive.get(), d.bary = bary.get(), d.flags = flags.get(), d.prev_triangles = tris.get();
    std::string err;
    if (rt2::temporal_deform_host(&d, err) != RT_OK) return fail("the case", err);
    FILE* o = fopen(argv[2], "wb");
    if (!o) return fail(argv[2], "cannot open");
    fwrite(out.get(), 4, 4 * n, o);
    fwrite(out_history.get(), 4, n, o);
    fwrite(motion.get(), 4, 2 * n, o);
    fclose(o);
    printf("%ux%u ok\n", d.width, d.height);
    return one_texel();
}
