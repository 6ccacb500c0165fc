"""The single scatter pass of the FIXED persistent render kernels (rt_kernel.hip: single_settle, single_start,
single_scatter; RT_SINGLE_SCATTER).

The general kernels scatter twice per iteration: at the memoised primary hit of a lane that starts a sample, and again
behind the traversal, where most lanes end their path.  The FIXED kernels settle a traversed segment first -- the segment's
count, the light, and whether the path ends, decided from the generator's state -- start the fresh lanes and then scatter
once, every lane that goes on.  Nothing about the result may change.

Every case renders a batch in forced frame groups (as tests/test_gpu_frame_groups.py forces them: six tiles are too few
for the rule to give groups) twice, with the FIXED instantiation and with rt_test_fixed_switches off -- the general twin,
path_step's code -- and compares the image bit for bit, (segments, segments_reused) and the recorded tile costs between
the two, and the image and the segments against the oracle.  The shapes: 20 x 12 in 9 frames (groups of 4, 4, 1) and 24 x 16
in 20 frames (8, 8, 4), 3 x 2 tiles each, the right and top ones partly outside the frame."""
import ctypes as C

import numpy as np
import pytest

from _terminal_skip_scenes import copy_of, emissive, items_of
from conftest import bits

pytestmark = pytest.mark.gpu

SMALL, LARGE = (20, 12, 9, 4), (24, 16, 20, 8)   # width, height, frames of the batch, frames of a group
TILES = 3 * 2


@pytest.fixture(scope="module")
def single(rt, cornell):
    t = rt.RayTracer(device=0, max_width=64, max_height=64, lib=rt.load_test())
    t.set_option("pipeline", 0)
    t.set_option("frame_ahead", 0)
    t.set_option("batch_frames", 64)
    t.load_scene(cornell)
    yield t
    t.close()


@pytest.fixture(scope="module")
def scenes(rt, cornell):
    """name -> scene arrays: Cornell and its variants, the geometry and the layout of the mesh loop unchanged"""
    lit = emissive(cornell)
    assert len(lit) == 1
    boxes = items_of(rt, cornell)[-1][1]   # the forest's members: the two boxes
    dark = [i for i in range(cornell.meshes.shape[0]) if i not in lit]
    walls = [i for i in dark if i not in boxes]
    assert len(boxes) == 2 and walls
    out = {"cornell": cornell}
    # a colour component above every roulette value: no roulette kills, every path runs into the bounce limit
    out["never_kill"] = copy_of(rt, cornell)
    out["never_kill"].meshes["material"]["color"][dark] = (1.5, 1.25, 1.0, 1.0)
    # ... the same walls, and boxes whose throughput is zero: a segment that hits a box dies there, always
    out["boxes_kill"] = copy_of(rt, out["never_kill"])
    out["boxes_kill"].meshes["material"]["color"][boxes] = (0.0, 0.0, 0.0, 1.0)
    # zero everywhere: every sample dies at its primary hit, so every frame of every pixel ends in the start step
    out["all_kill"] = copy_of(rt, cornell)
    out["all_kill"].meshes["material"]["color"][:] = (0.0, 0.0, 0.0, 1.0)
    # the light absorbs everything: a sample that hits it dies there and has taken its emitted light
    out["light_absorbs"] = copy_of(rt, cornell)
    out["light_absorbs"].meshes["material"]["color"][lit] = (0.0, 0.0, 0.0, 1.0)
    # is_spec always on the walls, one draw in two on the boxes: both sides of the settle test's choice of colour
    spec = copy_of(rt, cornell)
    m = spec.meshes["material"]
    m["specular"][walls] = 1.0
    m["specular_color"][walls] = (0.9, 0.8, 0.85, 1.0)
    m["color"][walls] = (0.2, 0.1, 0.15, 1.0)
    m["specular"][boxes] = 0.5
    m["specular_color"][boxes] = (0.9, 0.6, 0.3, 1.0)
    m["color"][boxes] = (0.2, 0.1, 0.05, 1.0)
    m["smoothness"][dark] = 0.7
    out["specular"] = spec
    # a -0 in the camera's origin: no pixel has a memoised ray, every sample generates and traverses its primary ray
    u = type(cornell.uniform).from_buffer_copy(bytes(cornell.uniform))
    assert u.camera.cam_to_world[3][0] == 0.0
    u.camera.cam_to_world[3][0] = -0.0
    out["neg_zero_camera"] = rt.SceneArrays(u, cornell.spheres, cornell.meshes, cornell.triangles, cornell.nodes, cornell.textures)
    return out


@pytest.fixture(scope="module")
def references(rt, oracle, scenes):
    """(scene, width, height, bounces, spp) -> the oracle's image after each of the frames 0 .. n - 1 and its segments summed
    up to each; computed once, never modified"""
    cache = {}

    def get(name, w, h, bounces, spp, n):
        images, segs = cache.setdefault((name, w, h, bounces, spp), ([], []))
        while len(images) < n:
            f = len(images)
            start = images[-1] if images else np.zeros((h, w, 4), np.float32)
            img, st = oracle.render(rt.make_params(w, h, bounces, spp, skybox=1, frames=f), scenes[name], image=start.copy())
            img = img.copy()
            img.setflags(write=False)
            images.append(img)
            segs.append((segs[-1] if segs else 0) + int(st.segments))
        return images[n - 1], segs[n - 1]
    return get


def switch(t, on):
    t._check(t._L.rt_test_fixed_switches(t._h, int(on), None))


def ran_fixed(t):
    out = C.c_uint32()
    t._check(t._L.rt_test_fixed_switches(t._h, -1, C.byref(out)))
    assert bool(out.value) == t.last_launch()["fixed_switches"]
    return bool(out.value)


def tile_costs(t):
    out = (C.c_uint32 * TILES)()
    t._check(t._L.rt_test_tile_costs(t._h, out, TILES))
    return list(out)


def batch(rt, t, shape, bounces, spp, on):
    """frames 0 .. n - 1 as one batch in forced groups, behind a warm-up batch of the same shape that records the tile costs
    the counted batch is ordered and tapered by: the image, (segments, segments_reused), the tile costs, whether FIXED ran"""
    w, h, n, group = shape
    switch(t, on)
    t.set_option("tile_feedback_period", 1)   # (resets the tile history)
    t._check(t._L.rt_test_frame_group(t._h, group, None))
    try:
        p = rt.make_params(w, h, bounces, spp, skybox=1, frames=0)
        for _ in range(2):
            t.write_image(np.zeros((h, w, 4), np.float32))
            t.reset_timing()
            t.render_frames(p, n)
        s = t.stats()
        return t.read_image(w, h).copy(), (int(s.segments), int(s.segments_reused)), tile_costs(t), ran_fixed(t)
    finally:
        t._check(t._L.rt_test_frame_group(t._h, 0, None))
        t.set_option("tile_feedback_period", 8)
        switch(t, 1)


def both_kernels_equal_the_oracle(rt, t, references, name, shape, bounces, spp):
    w, h, n, _ = shape
    ref, ref_segments = references(name, w, h, bounces, spp, n)
    got = {}
    for on in (1, 0):
        img, counts, costs, fixed = batch(rt, t, shape, bounces, spp, on)
        assert fixed == bool(on), on
        assert np.array_equal(bits(img), bits(ref)), on
        assert counts[0] == ref_segments, on
        got[on] = (bits(img).tobytes(), counts, costs)
    assert got[1] == got[0]
    return got[1]


CASES = [
    ("cornell", LARGE, 4, 8), ("cornell", SMALL, 4, 8), ("cornell", SMALL, 1, 8), ("cornell", SMALL, 0, 8),
    ("cornell", SMALL, -1, 8), ("cornell", SMALL, 4, 1), ("cornell", LARGE, 1, 1),
    ("never_kill", SMALL, 4, 8), ("boxes_kill", SMALL, 4, 8), ("boxes_kill", LARGE, 1, 8), ("all_kill", SMALL, 4, 8),
    ("light_absorbs", LARGE, 4, 8), ("specular", SMALL, 4, 8), ("specular", LARGE, 4, 1),
    ("neg_zero_camera", SMALL, 4, 8), ("neg_zero_camera", SMALL, 0, 8),
]


@pytest.mark.parametrize("name,shape,bounces,spp", CASES,
                         ids=[f"{c[0]}-{c[1][0]}x{c[1][1]}x{c[1][2]}-{c[2]}_bounces-{c[3]}_spp" for c in CASES])
def test_single_scatter_equals_the_general_twin_and_the_oracle(rt, single, scenes, references, name, shape, bounces, spp):
    t = single
    t.load_scene(scenes[name])
    try:
        _, counts, costs = both_kernels_equal_the_oracle(rt, t, references, name, shape, bounces, spp)
        w, h, n, _ = shape
        if bounces <= 0 and name != "neg_zero_camera":   # nothing is traversed: every segment is served from the memo
            assert counts[0] == counts[1] == (w * h * spp * n if bounces == 0 else 0)
        if name == "neg_zero_camera":   # no memoised ray at all
            assert counts[1] == 0
        if bounces >= 0:
            assert sum(costs) > 0
    finally:
        t.load_scene(scenes["cornell"])


@pytest.mark.parametrize("shape", [SMALL, LARGE], ids=["20x12", "24x16"])
def test_cornell_has_a_tile_that_mixes_sky_box_and_light_pixels(rt, oracle, cornell, shape):
    """what the Cornell cases above rely on: at no bounce and one sample a texel is the light of its primary hit -- nothing on
    the dark meshes, the emission on the light, the sky's colour on a miss"""
    w, h = shape[:2]
    img, _ = oracle.render(rt.make_params(w, h, 0, 1, skybox=1, frames=0), cornell, image=np.zeros((h, w, 4), np.float32))
    lum = img[..., :3].sum(-1)
    m = cornell.meshes["material"][emissive(cornell)[0]]
    light = float((m["emission_color"][:3] * m["emission_strength"]).sum())
    mixed = [(ty, tx) for ty in range((h + 7) // 8) for tx in range((w + 7) // 8)
             for tile in [lum[ty * 8:ty * 8 + 8, tx * 8:tx * 8 + 8]]
             if (tile == 0).any() and np.isclose(tile, light).any() and ((tile != 0) & ~np.isclose(tile, light)).any()]
    assert mixed


def test_one_launch_per_frame_runs_the_ungrouped_kernel_with_the_same_result(rt, single, scenes, references):
    """five single frames on the persistent kernel (six tiles would else take the one-wave-per-tile one), FIXED and general"""
    t, (w, h), n = single, SMALL[:2], 5
    ref, ref_segments = references("cornell", w, h, 4, 8, n)
    got = {}
    t.set_option("kernel_variant", 0)
    t.set_option("tile_feedback_period", 1)
    try:
        for on in (1, 0):
            switch(t, on)
            t.render(rt.make_params(w, h, 4, 8, skybox=1, frames=0))   # (settles the tables)
            t.write_image(np.zeros((h, w, 4), np.float32))
            t.reset_timing()
            kernels = []
            for f in range(n):
                t.render(rt.make_params(w, h, 4, 8, skybox=1, frames=f))
                kernels.append(ran_fixed(t))
            s = t.stats()
            img, counts, costs = t.read_image(w, h).copy(), (int(s.segments), int(s.segments_reused)), tile_costs(t)
            assert kernels == [bool(on)] * n, (on, kernels)
            assert np.array_equal(bits(img), bits(ref)), on
            assert counts[0] == ref_segments, on
            assert sum(costs) > 0
            got[on] = (bits(img).tobytes(), counts, costs)
        assert got[1] == got[0]
    finally:
        t.set_option("tile_feedback_period", 8)
        t.set_option("kernel_variant", -1)
        switch(t, 1)
