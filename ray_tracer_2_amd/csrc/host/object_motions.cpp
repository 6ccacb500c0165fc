// host/object_motions.cpp -- rt_object_motions and rt_object_motions_deforming (include/rt_abi.h, section 3): the motion
// table of rt_temporal_accumulate_moving / rt_temporal_accumulate_deforming from two states of one scene.  Plain C++ without a device; binary32, unfused
// (-ffp-contract=off), in the order the header states so that a numpy restatement gives the same bits.
#include <cstring>

#include "glam_math.h"
#include "rt_abi.h"

extern "C" int rt_object_motions(const rt_mesh_uniform* prev_meshes, const rt_mesh_uniform* meshes, uint32_t n_meshes,
                                 const rt_sphere* prev_spheres, const rt_sphere* spheres, uint32_t n_spheres, rt_object_motion* out) {
    using rt2::Mat4;
    if ((n_meshes && (!prev_meshes || !meshes)) || (n_spheres && (!prev_spheres || !spheres))) return RT_ERR_INVALID_ARGUMENT;
    if (!out && (n_meshes || n_spheres)) return RT_ERR_INVALID_ARGUMENT;
    for (uint32_t k = 0; k < n_meshes; ++k) {
        const rt_mesh_uniform &was = prev_meshes[k], &now = meshes[k];
        rt_object_motion& o = out[k];
        std::memset(&o, 0, sizeof(o));
        o.moved = std::memcmp(was.world_to_model, now.world_to_model, sizeof(Mat4)) != 0 ||
                  std::memcmp(was.model_to_world, now.model_to_world, sizeof(Mat4)) != 0;
        Mat4 was_m2w, was_w2m, now_m2w, now_w2m;
        std::memcpy(&was_m2w, was.model_to_world, sizeof(Mat4));
        std::memcpy(&was_w2m, was.world_to_model, sizeof(Mat4));
        std::memcpy(&now_m2w, now.model_to_world, sizeof(Mat4));
        std::memcpy(&now_w2m, now.world_to_model, sizeof(Mat4));
        const Mat4 D = rt2::mat4_mul(was_m2w, now_w2m);   // current world -> model -> previous world
        const Mat4 N = rt2::mat4_mul(now_m2w, was_w2m);   // its inverse: the normals go by the transpose of its 3 x 3
        for (int c = 0; c < 4; ++c)
            for (int r = 0; r < 3; ++r) o.d[c][r] = D.c[c][r];
        for (int c = 0; c < 3; ++c)
            for (int r = 0; r < 3; ++r) o.nt[c][r] = N.c[r][c];
    }
    for (uint32_t j = 0; j < n_spheres; ++j) {
        const rt_sphere &was = prev_spheres[j], &now = spheres[j];
        rt_object_motion& o = out[n_meshes + j];
        std::memset(&o, 0, sizeof(o));
        o.moved = std::memcmp(was.pos, now.pos, sizeof(was.pos)) != 0 || std::memcmp(&was.radius, &now.radius, sizeof(float)) != 0;
        const float s = was.radius / now.radius;
        for (int r = 0; r < 3; ++r) {
            o.d[r][r] = s;
            o.d[3][r] = was.pos[r] - s * now.pos[r];
            o.nt[r][r] = 1.0f;
        }
    }
    return RT_OK;
}

// rt_object_motions_deforming: that table, with the record of every mesh whose vertices moved replaced by the DEFORMED one
// -- the previous model_to_world for the points and, as the shader carries normals, its 3 x 3 for the directions.
extern "C" int rt_object_motions_deforming(const rt_mesh_uniform* prev_meshes, const rt_mesh_uniform* meshes, uint32_t n_meshes,
                                           const rt_sphere* prev_spheres, const rt_sphere* spheres, uint32_t n_spheres,
                                           const uint8_t* deformed, rt_object_motion* out) {
    if (n_meshes && !deformed) return RT_ERR_INVALID_ARGUMENT;
    if (const int rc = rt_object_motions(prev_meshes, meshes, n_meshes, prev_spheres, spheres, n_spheres, out); rc != RT_OK) return rc;
    for (uint32_t k = 0; k < n_meshes; ++k) {
        if (!deformed[k]) continue;
        rt_object_motion& o = out[k];
        std::memset(&o, 0, sizeof(o));
        o.moved = 2u;
        for (int c = 0; c < 4; ++c)
            for (int r = 0; r < 3; ++r) o.d[c][r] = prev_meshes[k].model_to_world[c][r];
        for (int c = 0; c < 3; ++c)
            for (int r = 0; r < 3; ++r) o.nt[c][r] = prev_meshes[k].model_to_world[c][r];
    }
    return RT_OK;
}
