"""Frame groups (RenderArgs::frame_group): with a group size G the work items of a batch are (tile, group) pairs and the
lane that took a pixel renders the group's frames of that pixel back to back.  Only the schedule may change: the image,
the segment and reuse counters and the tile costs of the batch's first frame must equal, bit for bit and count for count,
the same frames rendered one rt_render per frame -- at a frame of 20 x 12 (3 x 2 tiles, the right and bottom ones partly
outside the frame), with the group size forced through the test library, for batches of one group, a ragged last group
and a group as large as the batch, from frame 0 (the plain store) and from frame 5, under every option that changes
where the memo lives or what it holds."""
import ctypes as C

import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

W, H, BOUNCES, SPP = 20, 12, 4, 4
TILES = 3 * 2
GROUPS = (2, 3, 64)
BIG = 1 << 30   # tile_feedback_period: only a handle's first launch after a reset records costs, whatever follows


def batches_of(g):
    return (1, 2, g, g + 1, 2 * g + 1)


@pytest.fixture(scope="module")
def grouped(rt, cornell):
    """A handle of the test library (rt_test_frame_group, rt_test_tile_costs), persistent kernel throughout (the single
    frames of the reference would else take the one-wave-per-tile kernel, which records no per-pixel costs)."""
    t = rt.RayTracer(device=0, max_width=64, max_height=64, lib=rt.load_test())
    t.set_option("kernel_variant", 0)
    t.set_option("pipeline", 0)
    t.set_option("frame_ahead", 0)
    t.set_option("batch_frames", 64)
    t.load_scene(cornell)
    yield t
    t.close()


def force(t, g):
    t._check(t._L.rt_test_frame_group(t._h, g, None))


def last_group(t):
    out = C.c_uint32()
    t._check(t._L.rt_test_frame_group(t._h, -1, C.byref(out)))
    return out.value


def tile_costs(t, n_tiles=TILES):
    out = (C.c_uint32 * n_tiles)()
    t._check(t._L.rt_test_tile_costs(t._h, out, n_tiles))
    return list(out)


def start_image(f0, w=W, h=H):
    # frame 0 stores; a later frame blends with what the image holds
    return np.zeros((h, w, 4), np.float32) if f0 == 0 else np.random.RandomState(f0).rand(h, w, 4).astype(np.float32)


def counts(t):
    s = t.stats()
    return (s.segments, s.segments_reused, s.node_tests, s.triangle_tests)


def reference(rt, t, f0, ns, w=W, h=H, bounces=BOUNCES, spp=SPP, n_tiles=TILES):
    """{n: (image, counts)} after n single-frame launches from frame f0, and the tile costs of frame f0."""
    t.set_option("tile_feedback_period", BIG)   # (resets the tile history: the next launch records)
    t.write_image(start_image(f0, w, h))
    t.reset_timing()
    out, costs = {}, None
    for k in range(max(ns)):
        t.render(rt.make_params(w, h, bounces, spp, skybox=1, frames=f0 + k))
        if k == 0:
            costs = tile_costs(t, n_tiles)
        if k + 1 in ns:
            out[k + 1] = (t.read_image(w, h).copy(), counts(t))
    return out, costs


def batch(rt, t, f0, n, g, w=W, h=H, bounces=BOUNCES, spp=SPP, n_tiles=TILES):
    t.set_option("tile_feedback_period", BIG)
    force(t, g)
    try:
        t.write_image(start_image(f0, w, h))
        t.reset_timing()
        t.render_frames(rt.make_params(w, h, bounces, spp, skybox=1, frames=f0), n)
        return t.read_image(w, h).copy(), counts(t), tile_costs(t, n_tiles), last_group(t)
    finally:
        force(t, 0)


OPTIONS = [None, ("lds_scene", 0, 1), ("pixel_cache", 0, 1), ("pixel_cache", 2, 1), ("memo_in_table", 0, 1), ("roulette_skip", 0, 1),
           ("primary_hits", 0, 1), ("batch_tile_major", 0, 1)]


@pytest.mark.parametrize("f0", [0, 5])
@pytest.mark.parametrize("option", OPTIONS, ids=lambda o: "defaults" if o is None else f"{o[0]}={o[1]}")
def test_grouped_batches_equal_single_frames(rt, grouped, option, f0):
    t = grouped
    ns = sorted({n for g in GROUPS for n in batches_of(g)})
    if option:
        t.set_option(option[0], option[1])
    try:
        want, want_costs = reference(rt, t, f0, ns)
        assert sum(want_costs) > 0
        for g in GROUPS:
            for n in batches_of(g):
                img, cnt, costs, used = batch(rt, t, f0, n, g)
                what = (option, f0, g, n)
                assert np.array_equal(bits(img), bits(want[n][0])), what
                assert cnt == want[n][1], what
                assert costs == want_costs, what
                # what the last launch ran with: the forced size, at most its frames (65 frames are launches of 33 and
                # 32, 129 are three of 43); 1 for a single frame and for the frame-major order
                launches = -(-n // 64)
                last = n - -(-n // launches) * (launches - 1)
                # ... and for a scene read from global memory, whose kernels take no groups
                plain = option and option[0] in ("batch_tile_major", "lds_scene")
                assert used == (min(g, last) if n >= 2 and not plain else 1), what
    finally:
        if option:
            t.set_option(option[0], option[2])


def test_grouped_batch_against_the_oracle(rt, oracle, grouped, cornell):
    ref, segs = np.zeros((H, W, 4), np.float32), 0
    for f in range(5):
        ref, st = oracle.render(rt.make_params(W, H, BOUNCES, SPP, skybox=1, frames=f), cornell, image=ref)
        segs += st.segments
    img, cnt, _, used = batch(rt, grouped, 0, 5, 2)
    assert used == 2
    assert np.array_equal(bits(img), bits(ref)) and cnt[0] == segs


def test_grouped_counter_launch_against_the_oracle(rt, oracle, grouped, cornell):
    """count_tests: the counter instantiations re-intersect every memoised ray, so nothing is reused and the node and
    triangle tests are the shader's, frame by frame."""
    ref, seg, nt, tt = np.zeros((H, W, 4), np.float32), 0, 0, 0
    for f in range(7):
        ref, st = oracle.render(rt.make_params(W, H, BOUNCES, SPP, skybox=1, frames=f), cornell, image=ref)
        seg, nt, tt = seg + st.segments, nt + st.node_tests, tt + st.triangle_tests
    grouped.set_counters(True)
    try:
        img, cnt, _, used = batch(rt, grouped, 0, 7, 3)
    finally:
        grouped.set_counters(False)
    assert used == 3
    assert np.array_equal(bits(img), bits(ref)) and cnt == (seg, 0, nt, tt)


def test_grouped_strip_shares_assemble_to_the_full_frames(rt, grouped, cornell):
    w, h, world, n = 20, 28, 3, 5   # four strips, the last one ragged: ranks 0 / 1 / 2 own 2 / 1 / 1
    want, _ = reference(rt, grouped, 0, [n], w, h, n_tiles=3 * 4)
    pad = grouped.strip_texels(w, h, 0, world)
    gathered = np.zeros((world, pad, 4), np.float32)
    force(grouped, 2)
    try:
        for r in range(world):
            grouped.write_image(np.zeros((h, w, 4), np.float32))
            grouped.render_strips_frames(rt.make_params(w, h, BOUNCES, SPP, skybox=1, frames=0), n, r, world)
            assert last_group(grouped) == 2
            cnt = grouped.strip_texels(w, h, r, world)
            gathered[r, :cnt] = grouped.read_texels(cnt)
    finally:
        force(grouped, 0)
    stage = rt.RayTracer(0, world * pad, 1)
    try:
        stage.write_image(gathered.reshape(1, world * pad, 4))
        grouped.assemble_strips(stage.device_image_ptr, w, h, world)
        assert np.array_equal(bits(grouped.read_image(w, h)), bits(want[n][0]))
    finally:
        stage.close()


def settle(rt, t, w=W, h=H):
    """One frame after a scene with another camera: a single frame right behind a camera change renders without the primary
    table (a batch keeps it), which would show in the reference's reuse counter only."""
    t.render(rt.make_params(w, h, 1, 1, skybox=1, frames=0))


def test_many_mesh_textured_scene_ignores_the_forced_group(rt, grouped, cornell):
    """config 4's shape (many textured meshes under one transform, top-level tree kernels, scene in global memory): these
    kernels take no groups (groups of 4 measured 2.4 % slower there, profiles/frame_groups_ab.txt), so a forced size must
    change nothing, the reported size included."""
    from ray_tracer_2_amd import scenes
    w, h, n = 28, 20, 7
    grouped.load_scene(rt.SceneArrays.from_scene(scenes.sponza_standin(200)))
    settle(rt, grouped, w, h)
    try:
        want, want_costs = reference(rt, grouped, 0, [n], w, h, 3, 2, n_tiles=4 * 3)
        for g in (2, 3):
            img, cnt, costs, used = batch(rt, grouped, 0, n, g, w, h, 3, 2, n_tiles=4 * 3)
            assert used == 1   # (the many-mesh kernels take no groups, whatever is forced)
            assert np.array_equal(bits(img), bits(want[n][0])) and cnt == want[n][1] and costs == want_costs, g
    finally:
        grouped.load_scene(cornell)
        settle(rt, grouped)


def test_deferred_walk_rounds_ignore_the_forced_group(rt, grouped, cornell):
    """A deferred-walk sequence hands pixels from launch to launch through park records, so its launches take no groups
    whatever is forced: with defer_min_nodes = 1 the biggest BVH mesh of a seeded random scene (tests/test_gpu_scenes.py)
    is walked by rt_walk_kernel, the scene read from global memory."""
    from test_gpu_scenes import _random_scene
    t, n, w, h = grouped, 5, 28, 20
    try:
        t.set_option("lds_scene", 0)
        t.set_option("defer_min_nodes", 1)
        t.set_option("sort_rounds", 0)
        t.load_scene(_random_scene(rt, 2000))
        settle(rt, t, w, h)
        want, _ = reference(rt, t, 0, [n], w, h, 5, 3, n_tiles=4 * 3)
        t.set_option("sort_rounds", 2)
        img, cnt, _, used = batch(rt, t, 0, n, 3, w, h, 5, 3, n_tiles=4 * 3)
        assert t.last_launch()["deferred_walks"], "the rounds did not run"
        assert used == 1
        assert np.array_equal(bits(img), bits(want[n][0])) and cnt == want[n][1]
    finally:
        t.set_option("sort_rounds", -1)
        t.set_option("defer_min_nodes", 1024)
        t.set_option("lds_scene", 1)
        t.load_scene(cornell)
        settle(rt, t)
