"""The rule that gives a launch a render kernel with its fixed switches compiled in (csrc/host/launch_options.h:
FixedSwitches, fixed_switches_ok), on the CPU.

The rule as the header states it: true exactly when every constant the kernel compiles in equals the launch's value; a
switch that the kernels only test against zero is compared as such; the grouped kernel has the batch's three switches
(a batch, tile-major, in groups) compiled in, the ungrouped kernel leaves those three to the launch.  The values of the
bench launch below are written out by hand from what a default batch of the Cornell scene launches with (rt_api.hip: one dword per stack entry, root boxes
culled, both skips and the fast miss on, the terminal skip's mask of the seven dark meshes, the memo in LDS, a complete
primary table, skybox on, 8 samples per pixel -- a power of two --, the whole frame, 64 frames in tile-major order, a head
of 64); nothing here is computed with the code under test.  The constants the library reports are the header's own
(rt2::FixedSwitches, which rt_kernel.hip's fix_switches compiles in): the test pins them against the same list."""
import ctypes as C

import pytest

NAMES = ("stack_wide", "forest_cull", "roulette_skip", "fast_miss", "terminal_dark", "pixel_cache", "primary", "primary_complete",
         "skybox", "rays_per_pixel", "spp_reciprocal", "strip_world", "batch_frames", "batch_tile_major", "frame_group")
BENCH = dict(stack_wide=0, forest_cull=1, roulette_skip=1, fast_miss=1, terminal_dark=0b11111101, pixel_cache=1, primary=1,
             primary_complete=1, skybox=1, rays_per_pixel=8, spp_reciprocal=1, strip_world=1, batch_frames=64, batch_tile_major=1,
             frame_group=64)
# what the kernel compiles in, in the order of NAMES (1 for "not zero" where only that is tested; frame_group: "more than one")
CONSTANTS = (0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1)
# the three switches of the batch, which only the grouped kernel compiles in
BATCH = ("batch_frames", "batch_tile_major", "frame_group")
# a single frame behind its table, as the one-launch-per-frame leg of the bench launches it: in place (no batch) or pipelined
SINGLE = dict(BENCH, batch_frames=0, batch_tile_major=1, frame_group=1)
PIPELINED = dict(BENCH, batch_frames=1, batch_tile_major=0, frame_group=1)
# one launch per input of the rule that differs from the bench launch in that input alone
ONE_DIFFERS = [("stack_wide", 1), ("forest_cull", 0), ("roulette_skip", 0), ("fast_miss", 0), ("terminal_dark", 0), ("pixel_cache", 0),
               ("pixel_cache", 2), ("pixel_cache", 4), ("primary", 0), ("primary_complete", 0), ("skybox", 0), ("rays_per_pixel", 0),
               ("rays_per_pixel", -1), ("spp_reciprocal", 0), ("strip_world", 2), ("strip_world", 8), ("batch_frames", 0),
               ("batch_tile_major", 0), ("frame_group", 1), ("frame_group", 0)]


def rule(rt, values):
    L, inp, out = rt.load_test(), (C.c_int64 * 15)(*[values[k] for k in NAMES]), (C.c_int64 * 17)()
    rc = L.rt_test_fixed_switches_rule(C.byref(inp), C.byref(out))
    assert rc == 0, (rc, L.rt_last_error(None))
    assert out[1] == 1, "these expectations are written for the default build (RT_FIXED_SWITCHES=1)"
    return bool(out[0] & 1), tuple(out[2:]), bool(out[0] & 2)   # (the grouped kernel's answer, the constants, the ungrouped kernel's)


def test_yes_for_the_bench_launch(rt):
    assert rule(rt, BENCH)[0]


def test_yes_for_the_single_frames_of_the_bench_on_the_ungrouped_kernel(rt):
    for values in (SINGLE, PIPELINED):
        grouped, _, ungrouped = rule(rt, values)
        assert ungrouped and not grouped   # (the grouped kernel is not theirs: launch_render never asks)


def test_the_constants_are_the_ones_of_the_shared_header(rt):
    assert rule(rt, BENCH)[1] == CONSTANTS


@pytest.mark.parametrize("name,value", ONE_DIFFERS, ids=[f"{n}={v}" for n, v in ONE_DIFFERS])
def test_no_when_a_single_input_differs(rt, name, value):
    assert BENCH[name] != value
    grouped, _, ungrouped = rule(rt, dict(BENCH, **{name: value}))
    assert not grouped
    assert ungrouped == (name in BATCH)   # the ungrouped kernel leaves the batch's switches to the launch, and those alone
    if name not in BATCH:
        for values in (SINGLE, PIPELINED):
            assert not rule(rt, dict(values, **{name: value}))[2], values


def test_every_input_of_the_rule_has_a_no(rt):
    assert {n for n, _ in ONE_DIFFERS} == set(NAMES)


def test_values_that_differ_only_where_the_kernel_does_not_look_stay_yes(rt):
    """a switch that is tested against zero keeps its own value in the launch: another mask, table, sample count, batch
    size or head is the same kernel"""
    for name, value in (("terminal_dark", 1), ("rays_per_pixel", 4), ("batch_frames", 20), ("batch_frames", 2), ("frame_group", 2),
                        ("frame_group", 20), ("forest_cull", 7), ("skybox", 2)):
        assert rule(rt, dict(BENCH, **{name: value}))[0], (name, value)
        assert rule(rt, dict(BENCH, **{name: value}))[2], (name, value)
