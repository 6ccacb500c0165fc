"""The SAH plane search on the GPU (csrc/rt_bvh_search.hip: sah_chunks_kernel, sah_combine_kernel and the host code that
cuts a level into 512-triangle chunks) node by node: rt_test_sah_search on device 0 against tests/_sah_reference.py
(numpy, from bvh.rs:299-370) AND against the host search (device -1).  Per query all three agree: the axis exactly, the
position bit for bit, the cost by value (== or both NaN); a zero cost of another sign is compared by value like any
other and counted in the printed line.  No query is left out.  Families: tests/_sah_cases.py -- sizes around the chunk
seam at odd starts, one node of 100,000 and one of 1,048,876 triangles (2,049 partials), 70,006 nodes in one level
(more workgroups than 65,535, one- and multi-chunk nodes shuffled), eleven levels through one search object (every
buffer reallocated, then reused below capacity), every plane count 1..50 at its integer boundaries, flat and loose boxes,
centroids on planes, ties, signed zeros, overflow, denormals, non-finite entries.  Then whole builds,
Scene.build(device=0, min_triangles=...) against Scene.build(), byte for byte."""
import os

import numpy as np
import pytest

import _sah_cases as sc
from conftest import ROOT
from test_bvh_search_host import whole_build

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(sc.CASES))
def test_device_search_matches_the_reference_and_the_host_search(rt, name):
    tri9, order, levels = sc.CASES[name]()
    dev = sc.search(rt, 0, tri9, order, levels)
    host = sc.search(rt, -1, tri9, order, levels)
    want = sc.reference(tri9, order, levels)
    z_ref = sc.assert_same(dev, want, name + ": device against the reference")
    z_host = sc.assert_same(dev, host, name + ": device against the host search")
    sc.assert_same(host, want, name + ": host search against the reference")
    print(f"{name}: {len(dev)} queries in {len(levels)} level(s), all compared; zero costs of another sign: "
          f"{z_host} against the host search, {z_ref} against the reference")


def test_no_candidate_gives_infinite_cost_axis_0_position_0(rt):
    tri9 = np.tile(np.array([1, 2, 3] * 3, np.float32), (700, 1))
    order = np.arange(700, dtype=np.uint32)
    q = sc.queries(tri9, order, [(0, 2), (1, 512), (3, 513), (0, 700)])
    got = sc.search(rt, 0, tri9, order, [q])
    assert got["axis"].tolist() == [0] * 4 and got["pos"].view(np.uint32).tolist() == [0] * 4 and np.all(np.isposinf(got["cost"]))


def test_the_same_levels_twice_through_one_search_object(rt):
    """The levels of the `levels` family, then the same ones in reverse order, in one call: what a level left in the
    device buffers (partials, multi-chunk lists) must not reach the next."""
    tri9, order, levels = sc.CASES["levels"]()
    both = levels + levels[::-1]
    sc.assert_same(sc.search(rt, 0, tri9, order, both), sc.reference(tri9, order, both), "levels, there and back")


@pytest.mark.parametrize("name", list(sc.build_scenes()))
def test_device_build_is_the_host_build(rt, name):
    """Meshes of exactly 2, 511, 512, 513, 1024 and 1025 triangles; a regular grid (centroids tie); one mesh twice; sizes
    at min_triangles - 1, min_triangles, min_triangles + 1 (the small ones take the host builder inside the same loop);
    non-finite vertices (the build accepts them); quality 0 with a device named."""
    whole_build(rt, name, 0)


@pytest.mark.slow
def test_the_million_triangle_device_build_is_the_host_build(rt):
    """The config 5 stand-in of tests/test_gpu_full_size.py (dragon.obj x121 inside the Cornell box, 1,054,152 + 32
    triangles; thousands of partials per node at the top levels): the device build against the host build, byte for byte,
    and a valid tree."""
    from ray_tracer_2_amd import scenes
    g = os.path.join(ROOT, "tests", "golden")
    scene = scenes.cornell_dragon(scenes.load_raw_meshes(os.path.join(g, "cornell_raw.npz")),
                                  scenes.load_raw_meshes(os.path.join(g, "dragon_raw.npz")), subdivide=11, device=0)
    a = rt.SceneArrays.from_scene(scene)
    assert a.triangles.shape[0] == 32 + 1054152
    dev = a.nodes.tobytes(), a.triangles.tobytes(), a.meshes.tobytes()
    raw = scene.raw_meshes()
    big = int(np.argmax(a.meshes["triangles"]))
    v, idx = raw[big][1], raw[big][2]
    P = np.ascontiguousarray(v[:, :3], np.float32)[idx.reshape(-1)].reshape(-1, 3, 3)
    assert sc.check_tree(a, big, scene.triangle_order(big), P) >= 3
    assert sc.built_bytes(rt, scene) == dev
