"""The device blob against the host pack: after rt_upload_scene, and again after one rt_update_instances that moves a mesh
out of its run of shared transforms, rt_test_scene_blob returns exactly the bytes and the SceneLayout that
rt_test_pack_scene (no device) returns for the same arrays under the handle's options.  Scenes: the Cornell box (blob in
LDS, forest and flat items; the edit takes one of the forest's two members away, so the forest falls apart), the
36-level chain (a deep mesh) with two small meshes in its run that form a forest until the edit moves one of them, and
sponza_standin(24) (a top-level tree; the edit splits its run into two trees and a single mesh).  Every edit changes
the number of items and the size of the head, so the blob is a new allocation with the old tail copied on the device."""
import numpy as np
import pytest

import _scene_pack_cases as P
from test_gpu_scene_edits import clone, translated

pytestmark = pytest.mark.gpu

def deep_chain_with_a_forest(rt):
    """deep_chain_scene(levels=36) plus two meshes that share its transform and alias one five-node BVH (a root over a
    leaf and an internal node over two leaves, one far triangle each -- not the two-leaf shape, which would run as a flat
    item --, appended to the chain's nodes): the deep mesh is a single item, the two a forest."""
    a = P.deep_chain(rt)
    extra = np.zeros(5, a.nodes.dtype)
    for k, (left, right) in ((0, (1, 2)), (2, (3, 4))):
        extra[k]["left"], extra[k]["right"] = left, right
        extra[k]["aabb_min"], extra[k]["aabb_max"] = (-10, -10, -103), (10, 10, -100)
    for t, k in enumerate((1, 3, 4)):
        extra[k]["first"], extra[k]["count"] = t, 1
        extra[k]["aabb_min"], extra[k]["aabb_max"] = (-10, -10, -100 - t), (10, 10, -100 - t)
    small = a.meshes[:1].copy()
    small["node_offset"], small["triangles"] = len(a.nodes), 3
    out = clone(a, meshes=np.concatenate([a.meshes, small, small]))
    out.nodes = np.concatenate([a.nodes, extra])
    out.uniform.nodes = len(out.nodes)
    return out


# name -> (arrays, the mesh the edit moves: one of the two members of a forest, which then falls apart (Cornell box, chain);
# a mesh in the middle of the stand-in's tree)
SCENES = {"cornell_box": (P.cornell_box, 6), "deep_chain36": (deep_chain_with_a_forest, 2), "sponza24": (lambda rt: P.sponza(rt, 24), 12)}


def split_a_run(arrays, i):
    """`arrays` with mesh i moved by a little: it leaves its run of shared transforms, which splits around it."""
    m = arrays.meshes.copy()
    m[i] = translated(m[i], (0.03125, 0.0, 0.015625))
    return clone(arrays, meshes=m)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_device_blob_equals_the_host_pack_after_upload_and_after_an_update(rt, name):
    import ray_tracer_2_amd._abi as A
    n_items = A.PACK_FACT_FIELDS.index("n_items")
    make, moved = SCENES[name]
    arrays = make(rt)
    T = rt.RayTracer(device=0, max_width=64, max_height=40, lib=rt.load_test())
    try:
        T.load_scene(arrays)
        want, want_lay, facts = rt.RayTracer.pack_scene(arrays)
        blob, lay, _ = T.scene_blob()
        assert np.array_equal(lay, want_lay) and np.array_equal(blob, want)
        edited = split_a_run(arrays, moved)
        T.update_instances(edited)
        want2, want_lay2, facts2 = rt.RayTracer.pack_scene(edited)
        blob2, lay2, _ = T.scene_blob()
        assert np.array_equal(lay2, want_lay2) and np.array_equal(blob2, want2)
        assert int(facts2[n_items]) != int(facts[n_items]) and int(lay2[1]) != int(lay[1])   # (another item count and head size)
    finally:
        T.close()
