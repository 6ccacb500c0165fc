"""The head of a tapered launch (csrc/host/launch_options.h: frame_group_tapered_for; rt_api.hip: tile_feedback): a launch
that carries a taper table starts from frame groups longer than a launch without one may take -- up to a whole batch of 64
frames on one lane.  Only the schedule may change: with heads of 16, 32 and 64 frames and ragged, not monotone tables
forced through the test library, batches of 64 and of 33 frames must equal, bit for bit and count for count, the same
frames rendered one rt_render per frame -- the image, the segment and reuse counters and the tile costs of the batch's
first frame -- at the 20 x 12 frame of tests/test_gpu_frame_groups.py (3 x 2 tiles), under every option that changes where
the memo lives or what it holds.  The last test forces nothing: on a grid of one workgroup the two rules differ at this
frame size, and the launcher must take the long head exactly when the launch carries the table written for it."""
import ctypes as C

import numpy as np
import pytest

from conftest import bits
from test_gpu_frame_groups import BOUNCES, H, OPTIONS, SPP, TILES, W, batch, counts, last_group, reference, start_image, tile_costs
from test_gpu_frame_taper import WORDS, expected_table, last_table, tapered_batch

pytestmark = pytest.mark.gpu

HEADS = (16, 32, 64)
BATCHES = (64, 33)
# name: (first ranks, group sizes, the forced head) over the six tiles
TABLES = {
    "64 8 1": ((0, 2, 4), (64, 8, 1), 64),          # a whole batch on one lane, then the taper's own shape
    "32 64 2": ((0, 2, 4), (32, 64, 2), 32),        # not monotone: a group beyond the head in the middle
    "16 3 5": ((0, 1, 3), (16, 3, 5), 16),          # ragged at every level (33 = 16 + 16 + 1 = 11 x 3 = 6 x 5 + 3)
    "1 64": ((0, 5), (1, 64), 64),                  # single frames first, the longest item last
}


@pytest.fixture(scope="module")
def headed(rt, cornell):
    t = rt.RayTracer(device=0, max_width=64, max_height=64, lib=rt.load_test())
    t.set_option("kernel_variant", 0)
    t.set_option("pipeline", 0)
    t.set_option("frame_ahead", 0)
    t.set_option("batch_frames", 64)
    t.load_scene(cornell)
    yield t
    t.close()


_references = {}


def shared_reference(rt, t, f0):
    """The single-frame launches of the default options, rendered once per first frame for every test that compares with them."""
    if f0 not in _references:
        _references[f0] = reference(rt, t, f0, list(BATCHES))
    return _references[f0]


@pytest.mark.parametrize("f0", [0, 5])   # the plain store of frame 0, and an accumulation that goes on
def test_long_heads_equal_single_frames(rt, headed, f0):
    """No table (no tile order yet): every tile in groups of the forced head."""
    want, want_costs = shared_reference(rt, headed, f0)
    assert sum(want_costs) > 0
    for head in HEADS:
        for n in BATCHES:
            img, cnt, costs, used = batch(rt, headed, f0, n, head)
            assert used == min(head, n), (head, n)
            assert last_table(headed) == [0] * WORDS, (head, n)
            assert np.array_equal(bits(img), bits(want[n][0])), (head, n)
            assert cnt == want[n][1], (head, n)
            assert costs == want_costs, (head, n)


@pytest.mark.parametrize("f0", [0, 5])
@pytest.mark.parametrize("name", list(TABLES))
def test_forced_tables_under_long_heads_equal_single_frames(rt, headed, name, f0):
    ranks, sizes, head = TABLES[name]
    want, want_costs = shared_reference(rt, headed, f0)
    for n in BATCHES:
        img, cnt, costs, used, table = tapered_batch(rt, headed, f0, n, head, ranks, sizes)
        assert used == min(head, n), n
        assert table == expected_table(ranks, sizes, n, min(head, n), TILES), n
        assert np.array_equal(bits(img), bits(want[n][0])), n
        assert cnt == want[n][1], n
        assert costs == want_costs, n


@pytest.mark.parametrize("option", OPTIONS[1:], ids=lambda o: f"{o[0]}={o[1]}")
def test_every_memo_home_under_a_long_head(rt, headed, option):
    """Where the memo lives and what it holds: the lane that restarts a pixel for its next frame (memo_next_frame) does so
    up to 63 times in a row, inside items of 64, 32, 8, 2 and 1 frames."""
    t = headed
    t.set_option(option[0], option[1])
    try:
        want, want_costs = reference(rt, t, 5, list(BATCHES))
        plain = option[0] in ("batch_tile_major", "lds_scene")   # (launches that take no groups, hence no table)
        for name, n in (("64 8 1", 64), ("32 64 2", 33)):
            ranks, sizes, head = TABLES[name]
            img, cnt, costs, used, table = tapered_batch(rt, t, 5, n, head, ranks, sizes)
            assert used == (1 if plain else min(head, n)), (option, name)
            assert table == ([0] * WORDS if plain else expected_table(ranks, sizes, n, min(head, n), TILES)), (option, name)
            assert np.array_equal(bits(img), bits(want[n][0])), (option, name)
            assert cnt == want[n][1] and costs == want_costs, (option, name)
    finally:
        t.set_option(option[0], option[2])


# ---- nothing forced: which launches take the tapered head ----------------------------------------------------------------

FRAME_GROUP_TAPERED = 8      # RT_TEST_RULE_FRAME_GROUP_TAPERED
CAP_T, FLOOR_T = 64, 6       # the shipped RT_FRAME_GROUP_TAPERED and RT_FRAME_GROUP_FLOOR_TAPERED
# One workgroup = 4 resident waves, 6 tiles.  Without a table (cap 8, floor 24 items per wave = 96 items): 64 frames need 16
# groups per tile -> G = 4; 33 frames need 16 -> g = 2 (17 groups of 2).  With one (cap 64, floor 6 = 24 items): 64 frames
# need 4 groups per tile -> g = 21 (21 21 21 1), and 4 groups of 16 cover the batch: a head of 16.
OLD_64, OLD_33, HEAD_64 = 4, 2, 16


def test_the_tapered_head_runs_with_its_table_and_only_with_it(rt, cornell):
    L, inp, out = rt.load_test(), (C.c_int64 * 8)(64, TILES, 4, 1, 0, 0), (C.c_int64 * 2)()
    assert L.rt_test_launch_rule(FRAME_GROUP_TAPERED, C.byref(inp), C.byref(out)) == 0
    assert out[1] == CAP_T | FLOOR_T << 16, "these expectations are written for the shipped cap and floor"
    assert out[0] == HEAD_64
    t = rt.RayTracer(device=0, max_width=64, max_height=64, lib=rt.load_test())
    try:
        t.set_option("kernel_variant", 0)
        t.set_option("pipeline", 0)
        t.set_option("frame_ahead", 0)
        t.set_option("batch_frames", 64)
        t.set_option("persistent_blocks", 1)
        t.load_scene(cornell)
        plan = (64, 64, 33, 64)
        want, want_costs = reference(rt, t, 0, [sum(plan)])
        # A period of 100 frames: the first batch has no order and records costs, the second one sorts the tiles by them
        # and writes the table of (64 frames, head 16) behind the order; nothing is refreshed after that (97 frames old when
        # the third batch has run, and no costs recorded to refresh from).
        t.set_option("tile_feedback_period", 100)
        t.write_image(start_image(0))
        t.reset_timing()
        seen, f = [], 0
        for k, n in enumerate(plan):
            t.render_frames(rt.make_params(W, H, BOUNCES, SPP, skybox=1, frames=f), n)
            f += n
            seen.append((last_group(t), last_table(t)))
            if k == 0:
                assert tile_costs(t) == want_costs
        (g0, t0), (g1, t1), (g2, t2), (g3, t3) = seen
        assert g0 == OLD_64 and t0 == [0] * WORDS              # the first launch of the shape: no order, no table
        assert g1 == HEAD_64 and t1[2:4] == [64, HEAD_64]      # behind the order: the head and the table written for it
        assert 1 <= t1[0] <= 8 and t1[4:7] == [0, t1[5], 0] and all(1 <= g <= HEAD_64 for g in t1[5:4 + 3 * t1[0]:3])
        assert g2 == OLD_33 and t2 == [0] * WORDS              # another batch size than the table's: untapered, the old G
        assert g3 == HEAD_64 and t3 == t1                      # the table is still held: the head again
        assert np.array_equal(bits(t.read_image(W, H)), bits(want[sum(plan)][0]))
        assert counts(t) == want[sum(plan)][1]
    finally:
        t.close()
