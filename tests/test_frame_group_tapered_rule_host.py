"""The head of a launch that carries a taper table (csrc/host/launch_options.h: frame_group_tapered_for), on the CPU.

The rule is the sentence of frame_group_for under a cap and an item floor of its own: G = 1 for a batch of fewer than two
frames, for the frame-major order, for a launch with deferred-walk rounds planned and for a scene read from global memory
or walked by the many-mesh kernels.  Else take the LARGEST g that is at most the cap (RT_FRAME_GROUP_TAPERED, 64: a whole
batch), at most n, and leaves tiles x ceil(n / g) >= 6 x resident waves (g = 1 if no g >= 2 does); G is the smallest group
size that needs no more groups than g: ceil(n / ceil(n / g)).  Every expected value below was worked out by hand from
that sentence; nothing here is computed with the code under test.  frame_group_for with its default arguments stays the
rule of a launch without a table (cap 8, floor 24: tests/test_frame_group_rule_host.py)."""
import ctypes as C

import pytest

FRAME_GROUP, FRAME_GROUP_TAPERED = 6, 8    # RT_TEST_RULE_FRAME_GROUP, RT_TEST_RULE_FRAME_GROUP_TAPERED
CAP, FLOOR = 64, 6           # the shipped RT_FRAME_GROUP_TAPERED; items per resident wave, RT_FRAME_GROUP_FLOOR_TAPERED
WAVES = 256 * 5 * 4          # an MI355X: 1280 workgroups of four waves = 5120 resident waves -> 30720 items wanted
TILES_1080P = 240 * 135      # 32400
TILES_SHARE8 = 240 * 17      # 4080: the strip share of rank 0 of eight


def rule(rt, which, n, tiles, waves, tile_major=1, rounds=0, costly=0):
    L, inp, out = rt.load_test(), (C.c_int64 * 8)(n, tiles, waves, tile_major, rounds, costly), (C.c_int64 * 2)()
    rc = L.rt_test_launch_rule(which, C.byref(inp), C.byref(out))
    assert rc == 0, (rc, L.rt_last_error(None))
    return out[0], out[1]


def head(rt, *args, **kw):
    g, consts = rule(rt, FRAME_GROUP_TAPERED, *args, **kw)
    assert consts == CAP | FLOOR << 16, "these expectations are written for the shipped cap and floor"
    return g


def test_the_headline_shapes(rt):
    # the whole 1920 x 1080 frame: its 32400 tiles are more than the 30720 items wanted, so one group per tile will do and
    # the head is the batch itself
    for n in (64, 33, 32, 20, 10, 7, 2):
        assert head(rt, n, TILES_1080P, WAVES) == n, n


def test_the_strip_share_of_eight_ranks(rt):
    # 4080 tiles want 8 groups (7 x 4080 = 28560 falls short of 30720)
    assert head(rt, 28, TILES_SHARE8, WAVES) == 3     # g = 4 -> 7 groups; g = 3 -> 10 groups, which 3 frames each cover
    assert head(rt, 60, TILES_SHARE8, WAVES) == 8     # g = 9 -> 7 groups; g = 8 -> 8 groups (7 of 8 and one of 4)
    assert head(rt, 64, TILES_SHARE8, WAVES) == 8     # g = 10 -> 7 groups; g = 9 -> 8 groups, which 8 frames each cover


def test_both_sides_of_the_item_floor(rt):
    # 100 resident waves want 600 items; 16 frames: g = 16 -> 1 group, 15 .. 8 -> 2 groups (of 8), 7 and 6 -> 3 (of 6),
    # 5 and 4 -> 4 (of 4), 3 -> 6 (of 3), 2 -> 8 (of 2), 1 -> 16
    for tiles, g in ((600, 16), (599, 8), (300, 8), (299, 6), (200, 6), (199, 4), (150, 4), (149, 3), (100, 3), (99, 2), (75, 2), (74, 1), (38, 1), (37, 1)):
        assert head(rt, 16, tiles, 100) == g, tiles
    # ... and in the waves: 1000 tiles, 16 frames (1000 / 6 = 166.7, 2000 / 6 = 333.3, 3000 / 6 = 500, 4000 / 6 = 666.7,
    # 6000 / 6 = 1000, 8000 / 6 = 1333.3)
    for waves, g in ((166, 16), (167, 8), (333, 8), (334, 6), (500, 6), (501, 4), (666, 4), (667, 3), (1000, 3), (1001, 2), (1333, 2), (1334, 1)):
        assert head(rt, 16, 1000, waves) == g, waves
    assert head(rt, 16, 1000, 0) == 16    # (no resident waves known: nothing to starve)


def test_one_for_what_takes_no_groups(rt):
    assert head(rt, 1, TILES_1080P, WAVES) == 1 and head(rt, 0, TILES_1080P, WAVES) == 1      # a batch of one, a single frame
    assert head(rt, 64, TILES_1080P, WAVES, tile_major=0) == 1                                # frame-major order
    assert head(rt, 64, TILES_1080P, WAVES, rounds=1) == 1                                    # deferred-walk rounds planned
    assert head(rt, 64, TILES_1080P, WAVES, tile_major=0, rounds=1) == 1
    assert head(rt, 64, TILES_1080P, WAVES, costly=1) == 1        # a scene in global memory, the many-mesh kernels
    assert head(rt, 64, 1, WAVES) == 1 and head(rt, 64, 0, WAVES) == 1


def test_the_default_arguments_are_still_the_rule_without_a_table(rt):
    # cap 8, floor 24 (122880 items wanted): the values of tests/test_frame_group_rule_host.py
    for n, tiles, g in ((64, TILES_1080P, 8), (33, TILES_1080P, 7), (20, TILES_1080P, 5), (10, TILES_1080P, 3), (6, TILES_1080P, 1),
                        (28, TILES_SHARE8, 1), (60, TILES_SHARE8, 1), (64, TILES_SHARE8, 2)):
        assert rule(rt, FRAME_GROUP, n, tiles, WAVES) == (g, 8), (n, tiles)


@pytest.mark.parametrize("tiles,waves", [(TILES_1080P, WAVES), (TILES_SHARE8, WAVES), (6, WAVES), (6, 4), (1000, 100), (1, 1)])
def test_never_more_than_the_batch_and_the_groups_cover_the_batch(rt, tiles, waves):
    for n in range(1, 65):
        g = head(rt, n, tiles, waves)
        assert 1 <= g <= min(n, CAP), (n, g)
        n_groups = -(-n // g)
        assert n_groups * g >= n and (n_groups - 1) * g < n, (n, g)    # the last group is not empty
        assert g == -(-n // n_groups), (n, g)                          # ... and no smaller size covers the batch with as many
        if g > 1:
            assert tiles * n_groups >= FLOOR * waves, (n, g)
