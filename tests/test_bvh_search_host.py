"""The host builder's SAH plane search (csrc/host/bvh.cpp: find_best_split through make_host_level_search) node by node
against tests/_sah_reference.py, a numpy restatement of the reference's bvh.rs:299-370 that shares nothing with the C++.
No GPU: rt_test_sah_search with device -1 (include/rt_test_abi.h).  Every GPU comparison of the BVH build trusts the
host builder; this pins it to something that is not C++.  Per query: the axis exactly, the position bit for bit, the
cost by value (== or both NaN); no query is left out.  The families are those of tests/test_gpu_bvh_search.py
(tests/_sah_cases.py).  Also: the level-wise builder with the host search against the recursive one, whole scenes."""
import numpy as np
import pytest

import _sah_cases as sc
from conftest import bits

INVALID, DEVICE = -1, -3


@pytest.mark.parametrize("name", list(sc.CASES))
def test_host_search_matches_the_reference(rt, name):
    tri9, order, levels = sc.CASES[name]()
    got = sc.search(rt, -1, tri9, order, levels)
    want = sc.reference(tri9, order, levels)
    zeros = sc.assert_same(got, want, name)
    print(f"{name}: {len(got)} queries in {len(levels)} level(s), all compared; zero costs of another sign: {zeros}")


def test_no_candidate_gives_infinite_cost_axis_0_position_0(rt):
    """Zero extent on all three axes: every axis is skipped (bvh.rs:329-331) and the initial values come back."""
    tri9 = np.tile(np.array([1, 2, 3] * 3, np.float32), (700, 1))
    order = np.arange(700, dtype=np.uint32)
    q = sc.queries(tri9, order, [(0, 2), (1, 512), (3, 513), (0, 700)])
    got = sc.search(rt, -1, tri9, order, [q])
    assert got["axis"].tolist() == [0] * 4 and bits(got["pos"]).tolist() == [0] * 4 and np.all(np.isposinf(got["cost"]))
    sc.assert_same(got, sc.reference(tri9, order, [q]), "points")


def test_the_entry_refuses_what_the_builder_never_asks(rt):
    """count < 2, a range past the end, an order entry that is no triangle: RT_ERR_INVALID_ARGUMENT with a text -- and
    before the device is touched: with a device ordinal that cannot exist the answer is still the argument's."""
    from ray_tracer_2_amd.lib import RtError
    rng = np.random.default_rng(1)
    tri9 = sc.soup(rng, 100)
    order = np.arange(100, dtype=np.uint32)
    box = sc.tight(tri9, order, 0, 100)
    for device in (-1, 9999):
        for start, count, text in ((0, 1, "count < 2"), (5, 0, "count < 2"), (99, 2, "exceeds"), (0, 101, "exceeds"),
                                   (0xffffffff, 2, "exceeds")):
            with pytest.raises(RtError) as e:
                sc.search(rt, device, tri9, order, [sc.queries(tri9, order, [(0, 100)]), sc.queries(tri9, order, [(start, count)], [box])])
            assert e.value.code == INVALID and text in str(e.value)
        bad = order.copy()
        bad[7] = 100
        with pytest.raises(RtError) as e:
            sc.search(rt, device, tri9, bad, [sc.queries(tri9, order, [(0, 100)])])
        assert e.value.code == INVALID and "order[7]" in str(e.value)
    with pytest.raises(RtError) as e:
        sc.search(rt, -2, tri9, order, [sc.queries(tri9, order, [(0, 100)])])
    assert e.value.code == INVALID


def test_a_hip_error_is_rt_err_device_with_its_text(rt):
    """As rt_scene_build_device: a HIP error comes back as RT_ERR_DEVICE, the text in rt_last_error(NULL).  (A device
    ordinal that cannot exist fails in hipSetDevice, with or without a GPU in the machine.)"""
    from ray_tracer_2_amd.lib import RtError
    tri9 = sc.soup(np.random.default_rng(2), 10)
    order = np.arange(10, dtype=np.uint32)
    with pytest.raises(RtError) as e:
        sc.search(rt, 9999, tri9, order, [sc.queries(tri9, order, [(0, 10)])])
    assert e.value.code == DEVICE and "HIP" in str(e.value)


def test_no_level_and_empty_levels(rt):
    tri9 = sc.soup(np.random.default_rng(3), 10)
    order = np.arange(10, dtype=np.uint32)
    assert len(sc.search(rt, -1, tri9, order, [])) == 0
    q = sc.queries(tri9, order, [(0, 10)])
    got = sc.search(rt, -1, tri9, order, [q[:0], q, q[:0]])
    sc.assert_same(got, sc.reference(tri9, order, [q]), "empty levels")


@pytest.mark.parametrize("name", list(sc.build_scenes()))
def test_level_wise_build_with_the_host_search_is_the_recursive_build(rt, name):
    """Scene.build(device=-1, min_triangles=...): bvh_build_levels over make_host_level_search against bvh_build -- nodes,
    triangles and meshes byte for byte (non-finite vertices are accepted by add_mesh_from_data and build, so they are
    in), a tree that is valid by rules of its own, and, for finite meshes, oracle/host_oracle.py's build."""
    whole_build(rt, name, -1)


def whole_build(rt, name, device):
    from test_refit_host import check_boxes
    meshes, min_triangles = sc.build_scenes()[name]
    scene = sc.make_scene(rt, meshes)
    ref = sc.built_bytes(rt, scene)
    assert sc.built_bytes(rt, scene, device=device, min_triangles=min_triangles) == ref
    a = rt.SceneArrays.from_scene(scene)   # (the level-wise build is the one loaded)
    assert len(a.meshes) == len(meshes)
    from oracle import host_oracle as ho
    for i, (v, idx, _pos) in enumerate(meshes):
        P = np.ascontiguousarray(v[:, :3], np.float32)[idx.reshape(-1)].reshape(-1, 3, 3)
        sc.check_tree(a, i, scene.triangle_order(i), P)
        if not np.isfinite(P).all():
            continue
        if len(P) <= 700:
            check_boxes(a, i)   # (tests/test_refit_host.py: the fold in array order, bit for bit -- no zeros of two signs here)
        order, nodes = ho.build_bvh(P)
        t0, n0 = int(a.meshes["triangle_offset"][i]), int(a.meshes["node_offset"][i])
        tri, nd = a.triangles[t0:t0 + len(order)], a.nodes[n0:n0 + len(nodes)]
        assert np.array_equal(bits(tri["v1"]), bits(P[order, 0])) and np.array_equal(bits(tri["v2"]), bits(P[order, 1]))
        assert nd["left"].tolist() == [x["left"] for x in nodes] and nd["right"].tolist() == [x["right"] for x in nodes]
        assert nd["first"].tolist() == [x["first"] for x in nodes] and nd["count"].tolist() == [x["count"] for x in nodes]
        assert np.array_equal(bits(nd["aabb_min"]), bits(np.array([x["mn"] for x in nodes], np.float32)))
        assert np.array_equal(bits(nd["aabb_max"]), bits(np.array([x["mx"] for x in nodes], np.float32)))
    # quality 0 (Quality::Low) never goes level-wise: the host build, whatever device is named
    assert sc.built_bytes(rt, scene, quality=0, device=device, min_triangles=min_triangles) == sc.built_bytes(rt, scene, quality=0)
