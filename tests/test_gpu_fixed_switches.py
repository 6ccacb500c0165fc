"""The fixed switches (csrc/host/launch_options.h: FixedSwitches, fixed_switches_ok; rt_kernel.hip: the FIXED instantiations
of the persistent SIMPLE render kernels, grouped and ungrouped).

A grouped batch or a single frame whose wave-uniform switches have the values of every default launch runs a kernel with
those values compiled in: the same operations, branches whose condition is known.  Nothing about the result may change.
The frames are the ones of tests/test_gpu_frame_groups.py -- the Cornell scene at 20 x 12 (3 x 2 tiles, the right and top
ones partly outside the frame), 4 bounces -- at 8 samples per pixel, the group size forced through the test library (six
tiles are too few for the rule to give groups on a whole device) and the single frames kept on the persistent kernel.  With the switches on and off through rt_test_fixed_switches: the
image, the segment and reuse counters and the recorded tile costs are equal bit for bit and count for count, the image is
the oracle's, and rt_last_launch names the kernel that ran.  Every "no" of the rule that Python can reach runs the general
kernel and gives the oracle's image.  The rule's own cases are checked on the CPU in
tests/test_fixed_switches_rule_host.py."""
import ctypes as C

import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

W, H, BOUNCES, SPP = 20, 12, 4, 8
TILES = 3 * 2
TAPER_WORDS = 28   # RT_TEST_TAPER_WORDS


@pytest.fixture(scope="module")
def fixed(rt, cornell):
    t = rt.RayTracer(device=0, max_width=64, max_height=64, lib=rt.load_test())
    t.set_option("pipeline", 0)
    t.set_option("frame_ahead", 0)
    t.set_option("batch_frames", 64)
    t.load_scene(cornell)
    yield t
    t.close()


@pytest.fixture(scope="module")
def references(rt, oracle, cornell):
    """(spp, skybox) -> the oracle's image after each of the frames 0 .. n - 1 and its segments summed up to each; computed
    once, never modified"""
    cache = {}

    def get(n, spp=SPP, skybox=1):
        key = (spp, skybox)
        images, segs = cache.setdefault(key, ([], []))
        while len(images) < n:
            f = len(images)
            start = images[-1] if images else np.zeros((H, W, 4), np.float32)
            img, st = oracle.render(rt.make_params(W, H, BOUNCES, spp, skybox=skybox, frames=f), cornell, image=start.copy())
            img = img.copy()
            img.setflags(write=False)
            images.append(img)
            segs.append((segs[-1] if segs else 0) + int(st.segments))
        return images[n - 1], segs[n - 1]
    return get


def switch(t, on):
    t._check(t._L.rt_test_fixed_switches(t._h, int(on), None))


def ran_fixed(t):
    """whether the handle's last render launch ran the FIXED instantiation, by both reports"""
    out = C.c_uint32()
    t._check(t._L.rt_test_fixed_switches(t._h, -1, C.byref(out)))
    assert bool(out.value) == t.last_launch()["fixed_switches"]
    return bool(out.value)


def taper_of(t):
    out = (C.c_uint32 * TAPER_WORDS)()
    t._check(t._L.rt_test_frame_taper(t._h, -1, None, None, out))
    return list(out)


def tile_costs(t):
    out = (C.c_uint32 * TILES)()
    t._check(t._L.rt_test_tile_costs(t._h, out, TILES))
    return list(out)


def batch(rt, t, n, group, on, spp=SPP, skybox=1, warm=True):
    """frames 0 .. n - 1 as one batch in groups of `group`, behind a warm-up batch of the same shape: with a refresh period
    of one frame the warm-up records the tile costs (and has neither order nor taper), and the batch that counts is handed
    out in the order of those costs, carries their taper table and records costs of its own"""
    switch(t, on)
    t.set_option("tile_feedback_period", 1)   # (resets the tile history)
    t._check(t._L.rt_test_frame_group(t._h, group, None))
    try:
        p = rt.make_params(W, H, BOUNCES, spp, skybox=skybox, frames=0)
        kernels = []
        for _ in range(2 if warm else 1):
            t.write_image(np.zeros((H, W, 4), np.float32))
            t.reset_timing()
            t.render_frames(p, n)
            kernels.append(ran_fixed(t))
        s = t.stats()
        return t.read_image(W, H).copy(), (int(s.segments), int(s.segments_reused)), tile_costs(t), kernels, taper_of(t)
    finally:
        t._check(t._L.rt_test_frame_group(t._h, 0, None))
        t.set_option("tile_feedback_period", 8)
        switch(t, 1)


@pytest.mark.parametrize("n,group", [(20, 8), (5, 2)], ids=["20_frames_in_8_8_4", "5_frames_in_2_2_1"])
def test_fixed_and_general_kernels_give_the_same_batch(rt, fixed, references, n, group):
    ref, ref_segments = references(n)
    got = {}
    for on in (1, 0):
        img, counts, costs, kernels, taper = batch(rt, fixed, n, group, on)
        assert kernels == [bool(on), bool(on)], (on, kernels)   # the warm-up (no order, no taper yet) and the batch behind it
        assert taper[0] >= 1 and taper[2] == n and taper[3] == group, (on, taper)   # the batch that counts is tapered
        assert np.array_equal(bits(img), bits(ref)), on
        assert counts[0] == ref_segments, on
        assert sum(costs) > 0
        got[on] = (bits(img).tobytes(), counts, costs, taper)
    assert got[1] == got[0]


def singles(rt, t, n, on, pipeline):
    """frames 0 .. n - 1, one launch per frame on the persistent kernel (six tiles would else take the one-wave-per-tile one),
    in place or pipelined, behind one frame that settles the tables: the image, (segments, reused), the last frame's tile
    costs, which kernel each launch ran"""
    switch(t, on)
    t.set_option("kernel_variant", 0)
    t.set_option("pipeline", pipeline)
    t.set_option("pipeline_when_idle", 1 if pipeline else 0)
    t.set_option("tile_feedback_period", 1)
    try:
        t.render(rt.make_params(W, H, BOUNCES, SPP, skybox=1, frames=0))
        t.write_image(np.zeros((H, W, 4), np.float32))
        t.reset_timing()
        kernels = []
        for f in range(n):
            t.render(rt.make_params(W, H, BOUNCES, SPP, skybox=1, frames=f))
            kernels.append(ran_fixed(t))
        s = t.stats()
        return t.read_image(W, H).copy(), (int(s.segments), int(s.segments_reused)), tile_costs(t), kernels
    finally:
        t.set_option("tile_feedback_period", 8)
        t.set_option("pipeline_when_idle", 0)
        t.set_option("pipeline", 0)
        t.set_option("kernel_variant", -1)
        switch(t, 1)


@pytest.mark.parametrize("pipeline", [0, 3], ids=["in_place", "three_in_flight"])
def test_fixed_and_general_kernels_give_the_same_single_frames(rt, fixed, references, pipeline):
    n = 5
    ref, ref_segments = references(n)
    got = {}
    for on in (1, 0):
        img, counts, costs, kernels = singles(rt, fixed, n, on, pipeline)
        assert kernels == [bool(on)] * n, (on, kernels)
        assert np.array_equal(bits(img), bits(ref)), on
        assert counts[0] == ref_segments, on
        assert sum(costs) > 0
        got[on] = (bits(img).tobytes(), counts, costs)
    assert got[1] == got[0]


def no_case(rt, t, references, spp=SPP, skybox=1):
    """a batch of five frames in groups of two with the switches allowed: it must run the general kernel and give the oracle's
    image; counters apart, the same launch runs FIXED once the case's setting is taken back (the callers check)"""
    img, counts, _, kernels, _ = batch(rt, t, 5, 2, 1, spp, skybox)
    ref, ref_segments = references(5, spp, skybox)
    assert kernels == [False, False], kernels
    assert np.array_equal(bits(img), bits(ref))
    assert counts[0] == ref_segments


def runs_fixed_again(rt, t):
    assert batch(rt, t, 5, 2, 1, warm=False)[3] == [True]


@pytest.mark.parametrize("option,off,default", [("roulette_skip", 0, 1), ("fast_miss", 0, 1), ("cull_roots", 0, -1)])
def test_an_option_switched_off_runs_the_general_kernel(rt, fixed, references, option, off, default):
    fixed.set_option(option, off)
    try:
        no_case(rt, fixed, references)
    finally:
        fixed.set_option(option, default)
    runs_fixed_again(rt, fixed)


def test_no_skybox_runs_the_general_kernel(rt, fixed, references):
    no_case(rt, fixed, references, skybox=0)
    runs_fixed_again(rt, fixed)


def test_three_samples_per_pixel_run_the_general_kernel(rt, fixed, references):
    no_case(rt, fixed, references, spp=3)
    runs_fixed_again(rt, fixed)


def test_a_counter_launch_runs_the_general_kernel(rt, fixed, references):
    fixed.set_counters(True)
    try:
        no_case(rt, fixed, references)
    finally:
        fixed.set_counters(False)
    runs_fixed_again(rt, fixed)


def test_a_strip_share_of_two_runs_the_general_kernel(rt, fixed, references):
    t, world, n = fixed, 2, 5
    ref, _ = references(n)
    t._check(t._L.rt_test_frame_group(t._h, 2, None))
    try:
        for rank in range(world):   # 12 rows: strip 0 (rows 0 .. 7) is rank 0's, strip 1 (rows 8 .. 11) rank 1's
            t.write_image(np.zeros((H, W, 4), np.float32))
            t.render_strips_frames(rt.make_params(W, H, BOUNCES, SPP, skybox=1, frames=0), n, rank, world)
            assert not ran_fixed(t), rank
            rows = list(range(0, 8)) if rank == 0 else list(range(8, 12))
            mine = t.read_texels(t.strip_texels(W, H, rank, world)).reshape(-1, W, 4)
            assert np.array_equal(bits(mine[:len(rows)]), bits(ref[rows])), rank
    finally:
        t._check(t._L.rt_test_frame_group(t._h, 0, None))
    runs_fixed_again(rt, fixed)


def test_the_first_launch_after_set_camera_runs_the_general_kernel(rt, fixed, references, cornell):
    """A single frame right behind a camera change renders without the primary table: the general kernel, and the oracle's
    frame.  The frame behind it has its table and runs FIXED, and so does the batch behind that."""
    t = fixed
    cam_t = type(cornell.uniform.camera)
    moved = cam_t.from_buffer_copy(bytes(cornell.uniform.camera))
    moved.cam_to_world[3][0] += 0.21
    t.set_option("kernel_variant", 0)   # (the persistent kernel: six tiles would else take the one-wave-per-tile one)
    try:
        t.set_camera(moved)
        t.render(rt.make_params(W, H, BOUNCES, SPP, skybox=1, frames=0))
        t.set_camera(cam_t.from_buffer_copy(bytes(cornell.uniform.camera)))
        t.write_image(np.zeros((H, W, 4), np.float32))
        t.render(rt.make_params(W, H, BOUNCES, SPP, skybox=1, frames=0))
        assert not ran_fixed(t)
        assert np.array_equal(bits(t.read_image(W, H)), bits(references(1)[0]))
        t.render(rt.make_params(W, H, BOUNCES, SPP, skybox=1, frames=1))
        assert ran_fixed(t)
        assert np.array_equal(bits(t.read_image(W, H)), bits(references(2)[0]))
    finally:
        t.set_option("kernel_variant", -1)
    runs_fixed_again(rt, fixed)
