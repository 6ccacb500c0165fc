"""The hand-built deep chain BVH of test_gpu_scenes.test_deep_bvh_reproduces_the_shader_stack_overflow, shared with the
tests that need a scene whose stacks take more than 64 KiB of dynamic LDS (36 levels with option stack_wide = 1:
36 entries x 128 dwords x 4 B x 4 waves = 73,728 B)."""
import numpy as np


def deep_chain_scene(rt, cornell, levels=36, trap=31):
    """A hand-built chain BVH `levels` deep.  Levels 0..trap-1: the leaf is a far triangle and
    the other child (the rest of the chain) is nearer, so every level leaves a pending far entry
    and the shader's 32-entry stack fills up.  At level `trap` the leaf's box is nearer but its
    triangle is off to the side, so with an overflowing stack (far = rest of the chain, written
    to slot 31 and overwritten by the near leaf) the nearer triangles below are never tested."""
    n = levels
    tris = np.zeros(n + 1, cornell.triangles.dtype)
    z = np.zeros(n + 1, np.float32)
    for k in range(n + 1):
        z[k] = -100.0 - k if k < trap else (-10.0 if k == trap else -20.0 - (k - trap))
    for k in range(n + 1):
        v1, v2, v3 = (-10, -10, z[k]), (10, -10, z[k]), (0, 10, z[k])
        if k == trap:
            v1, v2, v3 = (-10, -10, z[k]), (-9, -10, z[k]), (-10, -9, z[k])   # far from every camera ray
        tris[k]["v1"], tris[k]["v2"], tris[k]["v3"] = v1, v2, v3
        tris[k]["n1"] = tris[k]["n2"] = tris[k]["n3"] = (0, 0, 1)
    nodes = np.zeros(2 * n + 1, cornell.nodes.dtype)
    big_lo, big_hi = np.float32([-10, -10, 0]), np.float32([10, 10, 0])
    for k in range(n):
        internal, leaf = 2 * k, 2 * k + 1
        nodes[internal]["left"], nodes[internal]["right"] = leaf, 2 * k + 2
        zs = z[k:]
        nodes[internal]["aabb_min"] = (-10, -10, zs.min())
        nodes[internal]["aabb_max"] = (10, 10, zs.max())
        nodes[leaf]["first"], nodes[leaf]["count"] = k, 1
        nodes[leaf]["aabb_min"] = big_lo + np.float32([0, 0, z[k]])   # box of the full-size triangle, also for the trap
        nodes[leaf]["aabb_max"] = big_hi + np.float32([0, 0, z[k]])
    last = 2 * n
    nodes[last]["first"], nodes[last]["count"] = n, 1
    nodes[last]["aabb_min"], nodes[last]["aabb_max"] = big_lo + np.float32([0, 0, z[n]]), big_hi + np.float32([0, 0, z[n]])
    sc = rt.Scene()
    sc.set_camera((0, 0, 5), (0, 0, 0), fov=30.0)
    mesh = cornell.meshes[:1].copy()
    mesh["node_offset"], mesh["triangle_offset"], mesh["triangles"] = 0, 0, n + 1
    mesh["material"]["color"] = (0.8, 0.7, 0.6, 1.0)
    mesh["material"]["emission_strength"] = 0.5
    mesh["material"]["emission_color"] = (1, 1, 1, 1)
    u = sc.uniform()
    u.meshes, u.nodes, u.spheres = 1, len(nodes), 0
    return rt.SceneArrays(u, np.zeros(0, cornell.spheres.dtype), mesh, tris, nodes)
