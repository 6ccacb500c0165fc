"""Scenes and scene facts shared by the terminal skip's tests (tests/test_terminal_skip_rule_host.py on the CPU,
tests/test_gpu_terminal_skip.py on the GPU).  Nothing here calls the code under test except the host packer, whose layout
the tests read to know where the forest is."""
import os

import numpy as np

from conftest import GOLDEN

ITEM_FOREST, ITEM_FLAT2 = 4, 8   # csrc/rt_scene_format.h


def copy_of(rt, a):
    return rt.SceneArrays(a.uniform, a.spheres.copy(), a.meshes.copy(), a.triangles.copy(), a.nodes.copy(), a.textures)


def emissive(arrays):
    """the meshes that are not dark: a product emission_color * emission_strength that is not zero"""
    m = arrays.meshes["material"]
    return [i for i in range(len(m)) if np.any(m["emission_color"][i] * m["emission_strength"][i] != 0)]


def dark_mask(arrays):
    return ((1 << arrays.meshes.shape[0]) - 1) & ~sum(1 << i for i in emissive(arrays))


def items_of(rt, arrays, **pack):
    """[(kind, mesh indices)] of the packed mesh loop, in the kernels' order (csrc/rt_scene_format.h)"""
    blob, lay, facts = rt.RayTracer.pack_scene(arrays, **pack)
    words = blob.view(np.uint32)
    item_off, forest_off = int(lay[6]) // 4, int(lay[8]) // 4
    out = []
    for it in range(int(facts[0])):
        kind, a, _b, c = (int(w) for w in words[item_off + it * 8: item_off + it * 8 + 4])
        if kind & ITEM_FOREST:
            out.append((kind, [int(words[forest_off + (a + j) * 12 + 1]) for j in range(c)]))
        else:
            out.append((kind, [a]))
    return out


def cornell_with_the_light_behind(rt):
    """Cornell rebuilt from its raw meshes with the light in a transform run of its own (lowered by a millimetre) and as the
    last mesh: its item comes behind the forest of the two boxes, which stand between it and the floor."""
    from ray_tracer_2_amd import scenes
    raw = scenes.load_raw_meshes(os.path.join(GOLDEN, "cornell_raw.npz"))
    lights = [k for k, r in enumerate(raw) if r[4].emission_strength != 0.0]
    assert len(lights) == 1
    light = raw.pop(lights[0])
    sc = rt.Scene()
    sc.set_camera((0, 1, 2), (0, 1, 0))
    for _label, v, idx, t, m in raw:
        sc.add_mesh_from_data(v, idx, xform=t, mat=m)
    at = light[3]
    lowered = rt.transform(pos=(at.pos[0], at.pos[1] - 0.001, at.pos[2]), rot=tuple(at.rot), scale=tuple(at.scale))
    sc.add_mesh_from_data(light[1], light[2], xform=lowered, mat=light[4])
    sc.build()
    return rt.SceneArrays.from_scene(sc)
